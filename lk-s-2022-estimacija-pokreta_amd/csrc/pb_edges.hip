// Soft edge strength without a trained model: a Pb-style oriented half-disc histogram gradient (Martin, Fowlkes, Malik,
// PAMI 2004), this build's own definition (include/dflow.h, DESIGN.md "Pb edge strength").  Integers up to the chi^2 sum,
// one IEEE float32 operation per written operation after it (-ffp-contract=off).
//
// Two launches on the caller's stream, nothing read back:
//   pb_pack_kernel     the three channels' 4-bit bins of every pixel as one uint16 (bin0 | bin1 << 4 | bin2 << 8), 2 B / px
//   pb_main_kernel<R>  per 32x8 tile: the packed plane on the tile + R (clamped coordinates: replicate border) in LDS; one
//                      thread per pixel, one pass over the disc per channel.
// Everything about the disc is a compile-time constant of R (PbDisc): the offsets, ordered by the 8 side signs they have
// (the 8 lines through the centre cut the disc into 16 wedges and 16 rays; every half-disc is a union of them), in chunks
// of at most 15.  A chunk's histogram is one uint64 of sixteen 4-bit counters (+= 1 << 4 bin per offset: no indexed
// array); a finished chunk is widened to 8-bit counters (4 dwords) and added to the half-discs it belongs to: 8
// orientations x 2 sides x 4 dwords, all with static indices, so nothing is indexed dynamically and nothing spills.
#include <utility>
#include "dflow_common.h"

#define PB_TW 32
#define PB_TH 8
#define PB_THREADS (PB_TW * PB_TH)
#define PB_CHUNK 15          // a 4-bit counter holds it

// the integer normals of the 8 orientations
constexpr int PB_NX[8] = {1, 2, 1, 1, 0, -1, -1, -2};
constexpr int PB_NY[8] = {0, 1, 1, 2, 1, 2, 1, 1};

template <int R> struct PbDisc {
    static constexpr int CAP = (2 * R + 1) * (2 * R + 1);
    int n = 0;                          // offsets
    int dx[CAP] = {}, dy[CAP] = {};
    int side[CAP][8] = {};              // +1 side A, -1 side B, 0 neither; equal inside a chunk
    bool first[CAP] = {}, last[CAP] = {};   // of its chunk
    int N[8] = {};                      // offsets per side
};

constexpr int pb_sign(int v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }
constexpr int pb_signature(int dx, int dy)
{
    int s = 0;
    for (int o = 7; o >= 0; o--) s = s * 3 + pb_sign(dx * PB_NX[o] + dy * PB_NY[o]) + 1;
    return s;
}

template <int R> constexpr PbDisc<R> pb_make_disc()
{
    PbDisc<R> d;
    bool done[2 * R + 1][2 * R + 1] = {};
    for (int y0 = -R; y0 <= R; y0++)
        for (int x0 = -R; x0 <= R; x0++) {
            if (done[y0 + R][x0 + R] || x0 * x0 + y0 * y0 == 0 || x0 * x0 + y0 * y0 > R * R) continue;
            // every offset with the signature of (x0, y0) not taken yet, in chunks
            const int sig = pb_signature(x0, y0);
            int in_chunk = 0;
            for (int y = -R; y <= R; y++)
                for (int x = -R; x <= R; x++) {
                    if (done[y + R][x + R] || x * x + y * y == 0 || x * x + y * y > R * R || pb_signature(x, y) != sig) continue;
                    done[y + R][x + R] = true;
                    const int k = d.n++;
                    d.dx[k] = x; d.dy[k] = y;
                    for (int o = 0; o < 8; o++) {
                        d.side[k][o] = pb_sign(x * PB_NX[o] + y * PB_NY[o]);
                        if (d.side[k][o] > 0) d.N[o]++;
                    }
                    d.first[k] = in_chunk == 0;
                    if (k > 0 && d.first[k]) d.last[k - 1] = true;
                    in_chunk = in_chunk + 1 == PB_CHUNK ? 0 : in_chunk + 1;
                }
        }
    d.last[d.n - 1] = true;
    return d;
}

template <int R> struct PbTab { static constexpr PbDisc<R> D = pb_make_disc<R>(); };

// f(IntC<0>()), f(IntC<1>()), ..., f(IntC<N - 1>())
template <typename F, int... I> __device__ __forceinline__ static void pb_static_for(std::integer_sequence<int, I...>, F &&f)
{
    (f(IntC<I>()), ...);
}
template <int N, typename F> __device__ __forceinline__ static void pb_static_for(F &&f)
{
    pb_static_for(std::make_integer_sequence<int, N>(), f);
}

__global__ void __launch_bounds__(PB_THREADS) pb_pack_kernel(const uint8_t *__restrict__ bgr, int H, int W,
                                                             uint16_t *__restrict__ packed)
{
    const int p = blockIdx.x * PB_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const uint8_t *px = bgr + (size_t)p * 3;
    const int B = px[0], G = px[1], Rd = px[2];
    const int c0 = gray_u8(bgr, W, p / W, p % W);
    const int c1 = (Rd - G + 255) >> 1;
    const int c2 = (2 * B - Rd - G + 510) >> 2;
    packed[p] = (uint16_t)((c0 >> 4) | ((c1 >> 4) << 4) | ((c2 >> 4) << 8));
}

template <int R> __global__ void __launch_bounds__(PB_THREADS) pb_main_kernel(const uint16_t *__restrict__ packed, int H, int W,
                                                                              float *__restrict__ strength,
                                                                              float *__restrict__ orient)
{
    constexpr int LW = PB_TW + 2 * R, LH = PB_TH + 2 * R;
    __shared__ uint16_t tile[LH * LW];
    const int tid = threadIdx.x, x0 = blockIdx.x * PB_TW, y0 = blockIdx.y * PB_TH;
    for (int i = tid; i < LH * LW; i += PB_THREADS) {
        const int y = min(max(y0 - R + i / LW, 0), H - 1), x = min(max(x0 - R + i % LW, 0), W - 1);
        tile[i] = packed[y * W + x];
    }
    __syncthreads();
    const int lx = tid % PB_TW, ly = tid / PB_TW, X = x0 + lx, Y = y0 + ly;
    if (X >= W || Y >= H) return;
    const uint16_t *ctr = tile + (ly + R) * LW + lx + R;
    float m[8] = {};
#pragma unroll 1
    for (int c = 0; c < 3; c++) {
        const int sh = 4 * c;
        uint32_t hist[2][8][4] = {};        // [side A / B][orientation]: 16 8-bit counters, bin b in dword (b / 8) * 2 + b % 2
        uint64_t acc = 0;                   // the current chunk: 16 4-bit counters, bin b at bit 4 b
        pb_static_for<PbTab<R>::D.n>([&](auto ik) {
            constexpr int k = decltype(ik)::value;
            if constexpr (PbTab<R>::D.first[k]) acc = 0;
            const uint32_t v = ctr[PbTab<R>::D.dy[k] * LW + PbTab<R>::D.dx[k]];
            acc += 1ull << (((v >> sh) & 15u) * 4u);
            if constexpr (PbTab<R>::D.last[k]) {
                const uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
                const uint32_t u[4] = {lo & 0x0F0F0F0Fu, (lo >> 4) & 0x0F0F0F0Fu, hi & 0x0F0F0F0Fu, (hi >> 4) & 0x0F0F0F0Fu};
                pb_static_for<8>([&](auto io) {
                    constexpr int o = decltype(io)::value, sd = PbTab<R>::D.side[k][o];
                    if constexpr (sd != 0) {
#pragma unroll
                        for (int j = 0; j < 4; j++) hist[sd > 0 ? 0 : 1][o][j] += u[j];
                    }
                });
            }
        });
        pb_static_for<8>([&](auto io) {
            constexpr int o = decltype(io)::value;
            float s = 0.0f;
            pb_static_for<16>([&](auto ib) {
                constexpr int b = decltype(ib)::value, j = (b / 8) * 2 + b % 2, sft = ((b % 8) / 2) * 8;
                const int g = (int)((hist[0][o][j] >> sft) & 255u), h = (int)((hist[1][o][j] >> sft) & 255u);
                const int d = g - h, den = g + h;
                // an empty bin adds (+0) / 1 to a sum that is >= +0: the same bits as leaving it out
                s = s + (float)(d * d) / (float)(den > 0 ? den : 1);
            });
            const float chi = s / (float)(2 * PbTab<R>::D.N[o]);
            m[o] = c == 0 ? 2.0f * chi : m[o] + chi;
        });
    }
    float e = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; o++) {
        m[o] = m[o] / 4.0f;
        e = fmaxf(e, m[o]);
    }
    const size_t p = (size_t)Y * W + X;
    strength[p] = e;
    if (orient) {
#pragma unroll
        for (int o = 0; o < 8; o++) orient[p * 8 + o] = m[o];
    }
}

struct PbWs {
    uint16_t *packed;   // (H,W) the three 4-bit bins of every pixel
};

static PbWs pb_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    WsCarver c(ws);
    PbWs w;
    w.packed = c.take<uint16_t>((size_t)H * W);
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t pb_ws_bytes(int H, int W) { size_t b; pb_ws(nullptr, H, W, &b); return b; }

int launch_pb(int H, int W, const uint8_t *bgr, int radius, float *strength, float *orient, void *ws, hipStream_t s)
{
    const PbWs w = pb_ws(ws, H, W);
    const dim3 tiles((W + PB_TW - 1) / PB_TW, (H + PB_TH - 1) / PB_TH);
    pb_pack_kernel<<<(H * W + PB_THREADS - 1) / PB_THREADS, PB_THREADS, 0, s>>>(bgr, H, W, w.packed);
    switch (radius) {
#define PB_CASE(R) case R: pb_main_kernel<R><<<tiles, PB_THREADS, 0, s>>>(w.packed, H, W, strength, orient); break;
        PB_CASE(1) PB_CASE(2) PB_CASE(3) PB_CASE(4) PB_CASE(5) PB_CASE(6) PB_CASE(7)
#undef PB_CASE
        default: return dflow_set_error(DFLOW_EINVAL, "pb edges: no kernel for radius %d", radius);
    }
    return dflow_check_launch("pb edge kernels");
}
