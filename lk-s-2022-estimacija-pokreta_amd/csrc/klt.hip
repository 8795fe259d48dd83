// Sparse feature tracking (include/dflow_klt.h: dflow_klt_pyramid, dflow_corners, dflow_klt_track; DESIGN.md "Sparse feature
// tracking"): a grey pyramid, Shi-Tomasi corners and pyramidal Lucas-Kanade over a track set.  This build's definitions; the
// reference has no counterpart.  Everything is an integer sum or a fixed float chain (-ffp-contract=off: one IEEE operation per
// written operation), so no result depends on an order and every comparison with tests/klt_ref.py is bit for bit.
//
// klt_grey_kernel, klt_down_kernel: four pixels of level 0 per lane from three dwords of the picture; one pixel of a coarser
//   level per lane from its 25 taps.
// klt_response_kernel: a workgroup owns a KC_TW x KC_TH tile; the gradients of the tile and its halo of rc window positions
//   (each clamped into the frame, as the definition clamps them) go to LDS as int16 once, every lane sums its window from there;
//   the plane's maximum through block_reduce (plane_ops.h) and one integer atomicMax per block.
// klt_occupy_kernel, klt_select_kernel: a slot, then a pixel per lane; the four counts through block_count (plane_ops.h).
// klt_track_kernel: a 16-lane group per slot, 16 slots per block.  The template and its gradients sit in LDS as int16 (32 * grey
//   fits), a lane owns every 16th window pixel, keeps its partial sums as int64 and adds them to the group's sums with 64-bit LDS
//   atomics; every lane of the group then reads the sums and does the same float64 solve, so nothing has to be handed round.  The
//   level loop, the iteration loop and the two passes are uniform over the block: a slot that is done keeps walking with its flag
//   down, every barrier is met by all 256 threads, and the iteration loop is left on a block-wide vote.  The sums rotate through
//   three buffers: the one a phase adds to was cleared two phases earlier, so one barrier per phase is enough.
#include <math.h>
#include "plane_ops.h"
#include "../../include/dflow_klt.h"

#define KLT_THREADS 256
#define KLT_WAVES (KLT_THREADS / 64)
#define KLT_MAX_LEVELS 8
#define KLT_LIVE 1
#define KLT_LEFT 2
#define KLT_INCONSISTENT 5
#define KLT_FLAT DFLOW_TRACK_FLAT
#define KLT_RESIDUAL DFLOW_TRACK_RESIDUAL

// the levels of a pyramid: sizes and byte offsets into the one buffer (below 2^27)
struct KltLevels { int n; int h[KLT_MAX_LEVELS], w[KLT_MAX_LEVELS]; uint32_t off[KLT_MAX_LEVELS]; };

static KltLevels klt_levels(int H, int W, int levels)
{
    KltLevels L;
    L.n = levels;
    uint32_t off = 0;
    for (int l = 0; l < KLT_MAX_LEVELS; l++) {
        L.h[l] = H; L.w[l] = W; L.off[l] = off;
        off += (uint32_t)H * (uint32_t)W;
        H = (H + 1) / 2; W = (W + 1) / 2;
    }
    return L;
}

size_t klt_pyramid_bytes(int H, int W, int levels)
{
    const KltLevels L = klt_levels(H, W, levels);
    return (size_t)L.off[levels - 1] + (size_t)L.h[levels - 1] * L.w[levels - 1];
}

// ---- the pyramid
__device__ static inline uint32_t klt_grey(uint32_t b, uint32_t g, uint32_t r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }

// group i = pixels 4i .. 4i+3 of the flat plane: bytes 12i .. 12i+11 of the picture, one dword of level 0
__global__ void __launch_bounds__(KLT_THREADS) klt_grey_kernel(uint32_t n, const uint8_t *__restrict__ bgr, uint8_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * KLT_THREADS + threadIdx.x;
    if (i * 4u >= n) return;
    if (i * 4u + 4u <= n) {
        const Bgr4 q = reinterpret_cast<const Bgr4 *>(bgr)[i];
        uint32_t c[4], v = 0;
        bgr_unpack4(q, c);
#pragma unroll
        for (int k = 0; k < 4; k++) v |= klt_grey(c[k] & 255u, (c[k] >> 8) & 255u, (c[k] >> 16) & 255u) << (8 * k);
        reinterpret_cast<uint32_t *>(out)[i] = v;
    } else {
        for (uint32_t p = i * 4u; p < n; p++) out[p] = (uint8_t)klt_grey(bgr[(size_t)p * 3], bgr[(size_t)p * 3 + 1], bgr[(size_t)p * 3 + 2]);
    }
}

__global__ void __launch_bounds__(KLT_THREADS) klt_down_kernel(int h, int w, int hc, int wc, const uint8_t *__restrict__ in,
                                                               uint8_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * KLT_THREADS + threadIdx.x;
    if (i >= (uint32_t)hc * (uint32_t)wc) return;
    const int y = (int)(i / (uint32_t)wc), x = (int)(i % (uint32_t)wc);
    const int k[5] = {1, 4, 6, 4, 1};
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; j++) xs[j] = clampi(2 * x + j - 2, 0, w - 1);
    int sum = 0;
#pragma unroll
    for (int a = 0; a < 5; a++) {
        const uint8_t *row = in + (size_t)clampi(2 * y + a - 2, 0, h - 1) * w;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) s += k[j] * (int)row[xs[j]];
        sum += k[a] * s;
    }
    out[i] = (uint8_t)((sum + 128) >> 8);
}

int launch_klt_pyramid(int H, int W, int levels, const uint8_t *bgr, uint8_t *pyr, hipStream_t s)
{
    const KltLevels L = klt_levels(H, W, levels);
    const uint32_t n = (uint32_t)H * (uint32_t)W, groups = (n + 3u) / 4u;
    hipLaunchKernelGGL(klt_grey_kernel, dim3((groups + KLT_THREADS - 1) / KLT_THREADS), dim3(KLT_THREADS), 0, s, n, bgr, pyr);
    for (int l = 1; l < levels; l++) {
        const uint32_t nc = (uint32_t)L.h[l] * (uint32_t)L.w[l];
        hipLaunchKernelGGL(klt_down_kernel, dim3((nc + KLT_THREADS - 1) / KLT_THREADS), dim3(KLT_THREADS), 0, s, L.h[l - 1], L.w[l - 1],
                           L.h[l], L.w[l], pyr + L.off[l - 1], pyr + L.off[l]);
    }
    return dflow_check_launch("klt pyramid kernels");
}

// ---- corners
#define KC_TW 32
#define KC_TH 8
#define KC_RMAX 7
#define KC_HW (KC_TW + 2 * KC_RMAX)
#define KC_HH (KC_TH + 2 * KC_RMAX)
#define KC_COUNTS 4                                   // candidates, maxima, suppressed, corners

__global__ void __launch_bounds__(KLT_THREADS) klt_response_kernel(int h, int w, int rc, const uint8_t *__restrict__ Y,
                                                                   float *__restrict__ resp, uint32_t *rmax)
{
    __shared__ int16_t s_gx[KC_HH * KC_HW], s_gy[KC_HH * KC_HW];
    const int tx0 = blockIdx.x * KC_TW, ty0 = blockIdx.y * KC_TH;
    const int hw = KC_TW + 2 * rc, hh = KC_TH + 2 * rc;
    for (int idx = threadIdx.x; idx < hw * hh; idx += KLT_THREADS) {
        const int ty = idx / hw, tx = idx - ty * hw;
        const int y = clampi(ty0 - rc + ty, 0, h - 1), x = clampi(tx0 - rc + tx, 0, w - 1);
        const uint8_t *row = Y + (size_t)y * w;
        s_gx[ty * KC_HW + tx] = (int16_t)((int)row[min(x + 1, w - 1)] - (int)row[max(x - 1, 0)]);
        s_gy[ty * KC_HW + tx] = (int16_t)((int)Y[(size_t)min(y + 1, h - 1) * w + x] - (int)Y[(size_t)max(y - 1, 0) * w + x]);
    }
    __syncthreads();
    const int lx = threadIdx.x % KC_TW, ly = threadIdx.x / KC_TW, x = tx0 + lx, y = ty0 + ly;
    int bits = 0;
    if (x < w && y < h) {
        int a = 0, b = 0, c = 0;
        for (int i = 0; i <= 2 * rc; i++) {
            for (int j = 0; j <= 2 * rc; j++) {
                const int gx = s_gx[(ly + i) * KC_HW + lx + j], gy = s_gy[(ly + i) * KC_HW + lx + j];
                a += gx * gx; b += gx * gy; c += gy * gy;
            }
        }
        const long long dif = (long long)a - c, rad = dif * dif + 4ll * ((long long)b * b);
        const double lam = ((double)(a + c) - sqrt((double)rad)) * 0.5;
        const float R = (float)(lam > 0.0 ? lam : 0.0);
        resp[(size_t)y * w + x] = R;
        bits = __float_as_int(R);
    }
    bits = block_reduce<KLT_WAVES>(bits, [](int &p, const int &q) { p = max(p, q); });
    if (threadIdx.x == 0 && bits > 0) atomicMax(rmax, (uint32_t)bits);
}

// a LIVE track among the slots below n occupies its pixel; all writers of a pixel store the same value
__global__ void __launch_bounds__(KLT_THREADS) klt_occupy_kernel(int h, int w, int cap, const float2 *__restrict__ pos,
                                                                 const int32_t *__restrict__ state, const int32_t *__restrict__ d_n,
                                                                 uint8_t *__restrict__ occ)
{
    const int i = blockIdx.x * KLT_THREADS + threadIdx.x;
    if (i >= clampi(*d_n, 0, cap) || state[i] != KLT_LIVE) return;
    const float2 p = pos[i];
    if (!bgr_inside(p.x, p.y, w, h)) return;
    occ[(size_t)(int)rintf(p.y) * w + (int)rintf(p.x)] = 1;
}

__global__ void __launch_bounds__(KLT_THREADS) klt_select_kernel(int h, int w, int min_dist, int border, float quality, float min_response,
                                                                 const float *__restrict__ resp, const uint32_t *__restrict__ rmax,
                                                                 const uint8_t *__restrict__ occ, uint8_t *__restrict__ mask, int32_t *counts)
{
    const uint32_t i = blockIdx.x * KLT_THREADS + threadIdx.x;
    bool is[KC_COUNTS] = {false, false, false, false};
    if (i < (uint32_t)h * (uint32_t)w) {
        const int y = (int)(i / (uint32_t)w), x = (int)(i % (uint32_t)w);
        const float R = resp[i], thr = quality * __uint_as_float(*rmax);
        is[0] = x >= border && x <= w - 1 - border && y >= border && y <= h - 1 - border && R >= thr && R >= min_response && R > 0.0f;
        if (is[0]) {
            const int y_lo = max(y - min_dist, 0), y_hi = min(y + min_dist, h - 1), x_lo = max(x - min_dist, 0), x_hi = min(x + min_dist, w - 1);
            bool top = true, taken = false;
            for (int yy = y_lo; yy <= y_hi && top; yy++) {
                for (int xx = x_lo; xx <= x_hi; xx++) {
                    const uint32_t j = (uint32_t)yy * (uint32_t)w + (uint32_t)xx;
                    const float Rn = resp[j];
                    if (Rn > R || (Rn == R && j < i)) top = false;
                    if (occ && occ[j]) taken = true;
                }
            }
            is[1] = top;
            is[2] = top && taken;
            is[3] = top && !taken;
        }
        mask[i] = is[3] ? 255 : 0;
    }
    block_count<KC_COUNTS>(is, counts, 0);
}

int launch_corners(int H, int W, const uint8_t *grey, int rc, int min_dist, int border, float quality, float min_response, int cap,
                   const float *pos, const int32_t *state, const int32_t *d_n, float *resp, uint8_t *mask, uint8_t *occ, uint32_t *rmax,
                   int32_t *counts, hipStream_t s)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W;
    DFLOW_HIP(hipMemsetAsync(rmax, 0, sizeof(uint32_t), s));
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, KC_COUNTS * sizeof(int32_t), s));
    hipLaunchKernelGGL(klt_response_kernel, dim3((W + KC_TW - 1) / KC_TW, (H + KC_TH - 1) / KC_TH), dim3(KLT_THREADS), 0, s, H, W, rc, grey,
                       resp, rmax);
    if (occ) {
        DFLOW_HIP(hipMemsetAsync(occ, 0, (size_t)n, s));
        hipLaunchKernelGGL(klt_occupy_kernel, dim3((cap + KLT_THREADS - 1) / KLT_THREADS), dim3(KLT_THREADS), 0, s, H, W, cap,
                           reinterpret_cast<const float2 *>(pos), state, d_n, occ);
    }
    hipLaunchKernelGGL(klt_select_kernel, dim3((n + KLT_THREADS - 1) / KLT_THREADS), dim3(KLT_THREADS), 0, s, H, W, min_dist, border, quality,
                       min_response, resp, rmax, occ, mask, counts);
    return dflow_check_launch("corner kernels");
}

// ---- the tracker
#define KT_GROUP 16                                   // lanes of a slot
#define KT_SLOTS (KLT_THREADS / KT_GROUP)             // slots of a block
#define KT_NSUMS 3
#define KT_COUNTS 7                                   // live after, left, flat, residual, inconsistent, not live before, converged

struct KltTrackArgs {
    KltLevels L;
    const uint8_t *pyr[2];
    int cap, r, iters;
    float min_eig, max_err, fb;
    double eps2;
    const float2 *pos_in;
    const int32_t *state_in;
    float2 *pos_out, *back;
    int32_t *state_out, *counts;
    float *err;
};

// SAMPLE of include/dflow_klt.h: 32 * grey of level G at (x, y), the corners clamped into the level
__device__ static inline int klt_sample(const uint8_t *__restrict__ G, int wl, int hl, float x, float y)
{
    const float xf = floorf(x), yf = floorf(y);
    const float ax = x - xf, ay = y - yf, bx = 1.0f - ax, by = 1.0f - ay;
    const int w00 = (int)rintf((bx * by) * 16384.f), w01 = (int)rintf((ax * by) * 16384.f), w10 = (int)rintf((bx * ay) * 16384.f);
    const int w11 = 16384 - w00 - w01 - w10;
    const int x0 = (int)xf, y0 = (int)yf;
    const int xa = clampi(x0, 0, wl - 1), xb = clampi(x0 + 1, 0, wl - 1);
    const uint8_t *ra = G + (size_t)clampi(y0, 0, hl - 1) * wl, *rb = G + (size_t)clampi(y0 + 1, 0, hl - 1) * wl;
    return (w00 * (int)ra[xa] + w01 * (int)ra[xb] + w10 * (int)rb[xa] + w11 * (int)rb[xb] + 256) >> 9;
}

// (i, j), row and column of a lane's window pixel in a window `width` wide, moved on by the KT_GROUP pixels q * width + r
__device__ static inline void klt_step(int &i, int &j, int q, int r, int width)
{
    i += q; j += r;
    if (j >= width) { j -= width; i++; }
}

// pos_out / state_out may be pos_in / state_in: no __restrict__ on the four.  Dynamic LDS: per slot T (2r+3)^2, Ix and Iy (2r+1)^2
// int16, padded to 8 bytes; then the three rotating sets of KT_NSUMS int64 sums per slot.
__global__ void __launch_bounds__(KLT_THREADS) klt_track_kernel(KltTrackArgs a)
{
    extern __shared__ unsigned long long klt_lds[];
    const int r = a.r, tw = 2 * r + 3, win = 2 * r + 1, n = win * win;
    const int per_slot = (tw * tw + 2 * n + 3) / 4;                                   // unsigned long longs of int16 data per slot
    const int tw_q = KT_GROUP / tw, tw_r = KT_GROUP % tw, win_q = KT_GROUP / win, win_r = KT_GROUP % win;
    const int g = threadIdx.x / KT_GROUP, ln = threadIdx.x % KT_GROUP;
    int16_t *T = reinterpret_cast<int16_t *>(klt_lds + (size_t)g * per_slot), *Ix = T + tw * tw, *Iy = Ix + n;
    unsigned long long *sums = klt_lds + (size_t)KT_SLOTS * per_slot;                 // [3][KT_SLOTS][KT_NSUMS]
    if (threadIdx.x < 3 * KT_SLOTS * KT_NSUMS) sums[threadIdx.x] = 0ull;
    int ph = 0;                                                                       // the phase: uniform over the block
    const int slot = blockIdx.x * KT_SLOTS + g;
    const bool have = slot < a.cap;
    const float2 p0 = have ? a.pos_in[slot] : make_float2(0.0f, 0.0f);
    const int st0 = have ? a.state_in[slot] : 0;
    int st = st0;                                                                     // the slot's state so far
    bool run = have && st0 == KLT_LIVE;                                               // the current pass is under way
    if (run && !bgr_inside(p0.x, p0.y, a.L.w[0], a.L.h[0])) { st = KLT_LEFT; run = false; }
    float2 p = p0, fwd_q = p0;
    float fwd_err = -1.0f;
    float2 back = make_float2(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000));
    bool converged = false;
    const int npass = a.fb > 0.0f ? 2 : 1;
    __syncthreads();

    for (int pass = 0; pass < npass; pass++) {
        const uint8_t *Pa = a.pyr[pass], *Pb = a.pyr[1 - pass];
        float dx = 0.0f, dy = 0.0f;
        int res = KLT_LIVE;                                                           // what this pass has come to
        float2 q = p;
        float perr = -1.0f;
        for (int l = a.L.n - 1; l >= 0; l--) {
            const int wl = a.L.w[l], hl = a.L.h[l];
            const uint8_t *Ga = Pa + a.L.off[l], *Gb = Pb + a.L.off[l];
            const float s = 1.0f / (float)(1 << l), plx = p.x * s, ply = p.y * s;
            if (l < a.L.n - 1) { dx = 2.0f * dx; dy = 2.0f * dy; }
            // 1. the template, its gradients and the matrix
            if (run) {
                for (int idx = ln, i = ln / tw, j = ln % tw; idx < tw * tw; idx += KT_GROUP) {
                    T[idx] = (int16_t)klt_sample(Ga, wl, hl, plx + (float)(j - r - 1), ply + (float)(i - r - 1));
                    klt_step(i, j, tw_q, tw_r, tw);
                }
            }
            __syncthreads();
            unsigned long long *acc = sums + ((ph % 3) * KT_SLOTS + g) * KT_NSUMS;
            if (run) {
                long long sa = 0, sb = 0, sc = 0;
                for (int idx = ln, i = ln / win, j = ln % win; idx < n; idx += KT_GROUP) {
                    const int c = (i + 1) * tw + j + 1;
                    const int gx = (int)T[c + 1] - (int)T[c - 1], gy = (int)T[c + tw] - (int)T[c - tw];
                    Ix[idx] = (int16_t)gx; Iy[idx] = (int16_t)gy;
                    sa += gx * gx; sb += gx * gy; sc += gy * gy;
                    klt_step(i, j, win_q, win_r, win);
                }
                atomicAdd(&acc[0], (unsigned long long)sa); atomicAdd(&acc[1], (unsigned long long)sb); atomicAdd(&acc[2], (unsigned long long)sc);
            }
            __syncthreads();
            const double A = (double)(long long)acc[0], B = (double)(long long)acc[1], C = (double)(long long)acc[2];
            if (ln == 0) { unsigned long long *z = sums + (((ph + 2) % 3) * KT_SLOTS + g) * KT_NSUMS; z[0] = 0ull; z[1] = 0ull; z[2] = 0ull; }
            ph++;
            const double D = A * C - B * B;
            const double lam = ((A + C) - sqrt((A - C) * (A - C) + 4.0 * (B * B))) * 0.5 / (4096.0 * (double)n);
            const bool flat = lam < (double)a.min_eig || !(D > 0.0);
            if (run && flat && l == 0) { res = KLT_FLAT; run = false; }
            // 2. the iterations: `on` while this slot iterates at this level
            bool on = run && !flat;
            float qx = 0.0f, qy = 0.0f;
            for (int it = 0; it < a.iters; it++) {
                acc = sums + ((ph % 3) * KT_SLOTS + g) * KT_NSUMS;
                if (on) {
                    qx = plx + dx; qy = ply + dy;
                    if (l > 0) {
                        qx = fminf(fmaxf(qx, 0.0f), (float)(wl - 1)); qy = fminf(fmaxf(qy, 0.0f), (float)(hl - 1));
                        dx = qx - plx; dy = qy - ply;
                    } else if (!bgr_inside(qx, qy, wl, hl)) { res = KLT_LEFT; run = false; on = false; }
                }
                if (on) {
                    long long sx = 0, sy = 0;
                    for (int idx = ln, i = ln / win, j = ln % win; idx < n; idx += KT_GROUP) {
                        const int e = klt_sample(Gb, wl, hl, qx + (float)(j - r), qy + (float)(i - r)) - (int)T[(i + 1) * tw + j + 1];
                        sx += e * (int)Ix[idx]; sy += e * (int)Iy[idx];
                        klt_step(i, j, win_q, win_r, win);
                    }
                    atomicAdd(&acc[0], (unsigned long long)sx); atomicAdd(&acc[1], (unsigned long long)sy);
                }
                if (!__syncthreads_or(on)) break;                                     // nobody added anything: the buffers stay as they are
                if (on) {
                    const double bx = (double)(long long)acc[0], by = (double)(long long)acc[1];
                    const double ex = -2.0 * ((C * bx - B * by) / D), ey = -2.0 * ((A * by - B * bx) / D);
                    dx += (float)ex; dy += (float)ey;
                    if (ex * ex + ey * ey < a.eps2) {
                        on = false;
                        if (l == 0 && pass == 0) converged = true;
                    }
                }
                if (ln == 0) { unsigned long long *z = sums + (((ph + 2) % 3) * KT_SLOTS + g) * KT_NSUMS; z[0] = 0ull; z[1] = 0ull; z[2] = 0ull; }
                ph++;
            }
        }
        // 3. the end position and its residual (T is level 0's)
        unsigned long long *acc = sums + ((ph % 3) * KT_SLOTS + g) * KT_NSUMS;
        if (run) {
            q.x = p.x + dx; q.y = p.y + dy;
            if (!bgr_inside(q.x, q.y, a.L.w[0], a.L.h[0])) { res = KLT_LEFT; run = false; }
        }
        if (run) {
            long long se = 0;
            for (int idx = ln, i = ln / win, j = ln % win; idx < n; idx += KT_GROUP) {
                const int e = klt_sample(Pb, a.L.w[0], a.L.h[0], q.x + (float)(j - r), q.y + (float)(i - r)) - (int)T[(i + 1) * tw + j + 1];
                se += e < 0 ? -e : e;
                klt_step(i, j, win_q, win_r, win);
            }
            atomicAdd(&acc[0], (unsigned long long)se);
        }
        __syncthreads();
        if (run) {
            perr = (float)((double)(long long)acc[0] / (32.0 * (double)n));
            if (a.max_err > 0.0f && perr > a.max_err) { res = KLT_RESIDUAL; run = false; }
        }
        if (ln == 0) { unsigned long long *z = sums + (((ph + 2) % 3) * KT_SLOTS + g) * KT_NSUMS; z[0] = 0ull; z[1] = 0ull; z[2] = 0ull; }
        ph++;
        if (pass == 0) {
            fwd_err = perr;
            if (have && st0 == KLT_LIVE && st == KLT_LIVE) {
                st = res;
                if (res == KLT_LIVE) { fwd_q = q; p = q; }                            // run is still up: the backward pass starts at q
            }
        } else if (have && st0 == KLT_LIVE && st == KLT_LIVE) {
            if (res == KLT_LIVE) {
                back = q;
                const float ddx = q.x - p0.x, ddy = q.y - p0.y;
                if (ddx * ddx + ddy * ddy > a.fb * a.fb) st = KLT_INCONSISTENT;
            } else st = KLT_INCONSISTENT;
            run = false;
        }
    }

    bool is[KT_COUNTS] = {false, false, false, false, false, false, false};
    if (have && ln == 0) {
        a.pos_out[slot] = st == KLT_LIVE && st0 == KLT_LIVE ? fwd_q : p0;
        a.state_out[slot] = st;
        if (a.err) a.err[slot] = fwd_err;
        if (a.back) a.back[slot] = back;
        is[0] = st0 == KLT_LIVE && st == KLT_LIVE; is[1] = st0 == KLT_LIVE && st == KLT_LEFT; is[2] = st0 == KLT_LIVE && st == KLT_FLAT;
        is[3] = st0 == KLT_LIVE && st == KLT_RESIDUAL; is[4] = st0 == KLT_LIVE && st == KLT_INCONSISTENT; is[5] = st0 != KLT_LIVE;
        is[6] = converged;
    }
    block_count<KT_COUNTS>(is, a.counts, 0);
}

int launch_klt_track(int H, int W, int levels, const uint8_t *pyr1, const uint8_t *pyr2, int cap, const float *pos_in,
                     const int32_t *state_in, int r, int iters, float eps, float min_eig, float max_err, float fb, float *pos_out,
                     int32_t *state_out, float *err, float *back, int32_t *counts, hipStream_t s)
{
    KltTrackArgs a;
    a.L = klt_levels(H, W, levels);
    a.pyr[0] = pyr1; a.pyr[1] = pyr2;
    a.cap = cap; a.r = r; a.iters = iters;
    a.min_eig = min_eig; a.max_err = max_err; a.fb = fb;
    a.eps2 = (double)eps * (double)eps;
    a.pos_in = reinterpret_cast<const float2 *>(pos_in); a.state_in = state_in;
    a.pos_out = reinterpret_cast<float2 *>(pos_out); a.back = reinterpret_cast<float2 *>(back);
    a.state_out = state_out; a.counts = counts; a.err = err;
    const int tw = 2 * r + 3, n = (2 * r + 1) * (2 * r + 1), per_slot = (tw * tw + 2 * n + 3) / 4;
    const size_t lds = ((size_t)KT_SLOTS * per_slot + 3 * KT_SLOTS * KT_NSUMS) * sizeof(unsigned long long);   // r = 10: 46.3 KB
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int32_t), s));
    hipLaunchKernelGGL(klt_track_kernel, dim3((cap + KT_SLOTS - 1) / KT_SLOTS), dim3(KLT_THREADS), lds, s, a);
    return dflow_check_launch("klt_track_kernel");
}
