// Looking at a flow without a ground truth (include/dflow.h, DESIGN.md "Flow pictures and the warp check"):
//   dflow_flow_color  the Middlebury colour-wheel picture of a flow field, in double, one IEEE operation per written operation
//   dflow_warp_eval   the second image warped back onto the first (bilinear, the operation order of var_warp_kernel,
//                     variational.hip), the photometric error per pixel and its statistics, in float32
// Built like flow_eval.hip, from the same helpers (plane_ops.h; -ffp-contract=off; hipcc's sqrt and / are correctly rounded):
// the planes as flat arrays of h*w pixels, four pixels per lane and step with 16-byte loads of the flow and 12- / 16-byte
// stores, the last group of a field whose h*w is no multiple of 4 pixel by pixel, grid-stride over at most PLANE_MAX_BLOCKS
// blocks, every block's partial result (block_reduce) into the workspace, a one-block final launch that adds the partials in a
// fixed order.  Nothing is read back, no atomics.
//   color_max_kernel<LAYOUT>, color_max_final_kernel   only for max_flow == 0: the largest float32 |(U,V)| of the known pixels
//   color_kernel<LAYOUT>                                the picture; the radius from the argument or from the workspace
//   warp_main_kernel<LAYOUT>, warp_final_kernel         the warp, the planes and *d_stats
// The grid is a function of h*w alone, so the order of every double addition is fixed: the same inputs give the same bits
// of sum_err on every call.
#include "plane_ops.h"
#include "flow_wheel.h"

#define PIC_THREADS PLANE_THREADS     // plane_blocks counts blocks of this size
#define PIC_WAVES (PIC_THREADS / 64)

__constant__ uint32_t pic_wheel[FLOW_WHEEL_N] = {FLOW_WHEEL_VALUES};

// a pixel whose flow can be drawn and followed: valid, finite, and no larger than 1e9 (a NaN compares false everywhere)
__device__ __forceinline__ static bool pic_known(float U, float V, float valid)
{
    return valid > 0.5f && fabsf(U) <= 1e9f && fabsf(V) <= 1e9f;
}

// ---- the colour picture ---------------------------------------------------------------------------------------------
__device__ __forceinline__ static void max_merge(float &a, float b) { a = fmaxf(a, b); }

__device__ __forceinline__ static float color_radius(float U, float V, float valid)
{
    return pic_known(U, V, valid) ? sqrtf(U * U + V * V) : 0.0f;
}

template <int LAYOUT>
__global__ void __launch_bounds__(PIC_THREADS) color_max_kernel(const float *__restrict__ flow, unsigned npix, float *__restrict__ partials)
{
    float m = 0.0f;
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    for (unsigned g = blockIdx.x * PIC_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * PIC_THREADS) {
        if (g < nfull) {
            float U[4], V[4], valid[4];
            flow_load4<LAYOUT>(flow, g, U, V, valid);
#pragma unroll
            for (int k = 0; k < 4; k++) m = fmaxf(m, color_radius(U[k], V[k], valid[k]));
        } else {
            for (unsigned p = g * 4u; p < npix; p++) {
                float U, V, valid;
                flow_load1<LAYOUT>(flow, p, U, V, valid);
                m = fmaxf(m, color_radius(U, V, valid));
            }
        }
    }
    m = block_reduce<PIC_WAVES>(m, max_merge);
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// one block: the largest partial, 1 when it is 0 (no known pixel, or all of them at rest), into *radius
__global__ void __launch_bounds__(PIC_THREADS) color_max_final_kernel(const float *__restrict__ partials, int nblocks, float *__restrict__ radius)
{
    float m = 0.0f;
    for (int b = threadIdx.x; b < nblocks; b += PIC_THREADS) m = fmaxf(m, partials[b]);
    m = block_reduce<PIC_WAVES>(m, max_merge);
    if (threadIdx.x == 0) *radius = m > 0.0f ? m : 1.0f;
}

// one pixel's picture entry (b | g << 8 | r << 16); wheel: the 55 entries as double (r, g, b) / 255
__device__ __forceinline__ static uint32_t color_pixel(float U, float V, float valid, double maxrad, const double *wheel)
{
    if (!pic_known(U, V, valid)) return 0u;
    const double fx = (double)U / maxrad, fy = (double)V / maxrad;
    const double rad = sqrt(fx * fx + fy * fy);
    const double a = atan2(-fy, -fx) / 3.14159265358979323846;
    const double fk = (a + 1.0) / 2.0 * (double)(FLOW_WHEEL_N - 1);
    const int k0 = min(FLOW_WHEEL_N - 1, (int)floor(fk));
    const int k1 = k0 + 1 == FLOW_WHEEL_N ? 0 : k0 + 1;
    const double f = fk - (double)k0;
    uint32_t out = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {                                    // r, g, b
        const double c0 = wheel[3 * k0 + ch], c1 = wheel[3 * k1 + ch];
        double col = c0 + f * (c1 - c0);
        col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
        out |= (uint32_t)(int)(255.0 * col) << (16 - 8 * ch);
    }
    return out;
}

template <int LAYOUT>
__global__ void __launch_bounds__(PIC_THREADS) color_kernel(const float *__restrict__ flow, unsigned npix, float fixed_radius,
                                                            const float *__restrict__ auto_radius, uint8_t *__restrict__ bgr,
                                                            float *__restrict__ maxrad_out)
{
    __shared__ double wheel_s[3 * FLOW_WHEEL_N];
    if (threadIdx.x < 3 * FLOW_WHEEL_N) {
        const int k = threadIdx.x / 3, ch = threadIdx.x % 3;
        wheel_s[threadIdx.x] = (double)((pic_wheel[k] >> (16 - 8 * ch)) & 255u) / 255.0;
    }
    __syncthreads();
    const float radius = fixed_radius > 0.0f ? fixed_radius : *auto_radius;       // uniform
    if (maxrad_out && blockIdx.x == 0 && threadIdx.x == 0) *maxrad_out = radius;
    const double maxrad = (double)radius;
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    for (unsigned g = blockIdx.x * PIC_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * PIC_THREADS) {
        if (g < nfull) {
            float U[4], V[4], valid[4];
            uint32_t c[4];
            flow_load4<LAYOUT>(flow, g, U, V, valid);
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = color_pixel(U[k], V[k], valid[k], maxrad, wheel_s);
            reinterpret_cast<Bgr4 *>(bgr)[g] = bgr_pack4(c);
        } else {
            for (unsigned p = g * 4u; p < npix; p++) {
                float U, V, valid;
                flow_load1<LAYOUT>(flow, p, U, V, valid);
                bgr_store1(bgr, p, color_pixel(U, V, valid, maxrad, wheel_s));
            }
        }
    }
}

// ---- the warp check -------------------------------------------------------------------------------------------------
// what a lane, a wave or a block has seen; a block of a 8192 x 8192 field sees at most 2^26 pixels: 32-bit counts
struct WarpPartial {
    double sum;
    uint32_t n, n_outside, n_unknown, n_above;
    float max_err;
    uint32_t pad;
};

__device__ __forceinline__ static void warp_merge(WarpPartial &a, const WarpPartial &b)
{
    a.sum = a.sum + b.sum;
    a.n += b.n; a.n_outside += b.n_outside; a.n_unknown += b.n_unknown; a.n_above += b.n_above;
    a.max_err = fmaxf(a.max_err, b.max_err);
}

struct WarpArgs {
    const uint8_t *I1, *I2;
    int w, h;
    float err_thresh, err_max;
};

// pixel (x, y) with the first image's entry i1 (b | g << 8 | r << 16): counts it into `acc` and returns its error (-1 when
// the pixel is not inside), its warped entry and its error-picture entry
__device__ __forceinline__ static void warp_pixel(const WarpArgs &A, int x, int y, float U, float V, float valid, uint32_t i1,
                                                  const uint32_t *lut, WarpPartial &acc, float &err_out, uint32_t &warped_out,
                                                  uint32_t &bgr_out)
{
    err_out = -1.0f; warped_out = 0u; bgr_out = 0u;
    if (!pic_known(U, V, valid)) { acc.n_unknown++; return; }
    const float xs = (float)x + U, ys = (float)y + V;
    if (!bgr_inside(xs, ys, A.w, A.h)) { acc.n_outside++; return; }
    float wv[3], own[3];                                                // b, g, r
    bgr_bilinear(A.I2, A.w, A.h, xs, ys, wv);
    bgr_entry_floats(i1, own);
    warped_out = bgr_round_entry(wv);
    const float err = bgr_mean_abs_diff(wv, own);
    err_out = err;
    acc.n++;
    acc.sum = acc.sum + (double)err;
    acc.max_err = fmaxf(acc.max_err, err);
    acc.n_above += err > A.err_thresh;
    if (lut) {
        const float t = fminf(err, A.err_max) / A.err_max;
        bgr_out = lut[min(255, (int)(t * 256.0f))];
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(PIC_THREADS) warp_main_kernel(WarpArgs A, const float *__restrict__ flow, unsigned npix,
                                                                uint8_t *__restrict__ warped, float *__restrict__ err,
                                                                uint8_t *__restrict__ bgr, WarpPartial *__restrict__ partials)
{
    __shared__ uint32_t lut_s[256];
    const uint32_t *lut = nullptr;
    if (bgr) {                                          // uniform
        lut_s[threadIdx.x] = plane_jet_lut[threadIdx.x];
        __syncthreads();
        lut = lut_s;
    }
    WarpPartial acc = {};
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    for (unsigned g = blockIdx.x * PIC_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * PIC_THREADS) {
        int y = (int)(g * 4u / (unsigned)A.w), x = (int)(g * 4u - (unsigned)y * (unsigned)A.w);
        if (g < nfull) {
            float U[4], V[4], valid[4], e[4];
            uint32_t wp[4], c[4], i1[4];
            flow_load4<LAYOUT>(flow, g, U, V, valid);
            bgr_unpack4(reinterpret_cast<const Bgr4 *>(A.I1)[g], i1);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                warp_pixel(A, x, y, U[k], V[k], valid[k], i1[k], lut, acc, e[k], wp[k], c[k]);
                if (++x == A.w) { x = 0; y++; }
            }
            if (warped) reinterpret_cast<Bgr4 *>(warped)[g] = bgr_pack4(wp);
            if (err) reinterpret_cast<float4 *>(err)[g] = make_float4(e[0], e[1], e[2], e[3]);
            if (bgr) reinterpret_cast<Bgr4 *>(bgr)[g] = bgr_pack4(c);
        } else {
            // the 1..3 pixels after the last whole group
            for (unsigned p = g * 4u; p < npix; p++) {
                float U, V, valid, e1;
                uint32_t w1, c1;
                flow_load1<LAYOUT>(flow, p, U, V, valid);
                const uint8_t *q = A.I1 + (size_t)p * 3;
                warp_pixel(A, x, y, U, V, valid, (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), lut, acc, e1, w1, c1);
                if (++x == A.w) { x = 0; y++; }
                if (warped) bgr_store1(warped, p, w1);
                if (err) err[p] = e1;
                if (bgr) bgr_store1(bgr, p, c1);
            }
        }
    }
    acc = block_reduce<PIC_WAVES>(acc, warp_merge);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(PIC_THREADS) warp_final_kernel(const WarpPartial *__restrict__ partials, int nblocks,
                                                                 int accumulate, dflow_photo_stats *__restrict__ stats)
{
    WarpPartial acc = {};
    // counts of the whole field: up to 2^26, and 32 bits hold them
    for (int b = threadIdx.x; b < nblocks; b += PIC_THREADS) warp_merge(acc, partials[b]);
    acc = block_reduce<PIC_WAVES>(acc, warp_merge);
    if (threadIdx.x != 0) return;
    dflow_photo_stats s = {};
    if (accumulate) s = *stats;
    s.n += acc.n; s.n_outside += acc.n_outside; s.n_unknown += acc.n_unknown; s.n_above += acc.n_above;
    s.sum_err = s.sum_err + acc.sum;
    s.max_err = fmaxf(s.max_err, acc.max_err);
    s.reserved = 0;
    *stats = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct ColorWs {
    float *partials;         // one maximum per block of color_max_kernel
    float *radius;           // what color_max_final_kernel leaves for color_kernel
};

static ColorWs color_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    WsCarver c(ws);
    ColorWs w;
    w.partials = c.take<float>((size_t)plane_blocks(H, W));
    w.radius = c.take<float>(1);
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t flow_color_ws_bytes(int H, int W) { size_t b; color_ws(nullptr, H, W, &b); return b; }

int launch_flow_color(int H, int W, const float *flow, int layout, float max_flow, uint8_t *bgr, float *maxrad, void *ws,
                      hipStream_t s)
{
    const ColorWs w = color_ws(ws, H, W);
    const int nblocks = plane_blocks(H, W);
    const unsigned npix = (unsigned)H * (unsigned)W;
    const bool uvv = layout == DFLOW_EVAL_UVV;
    if (!(max_flow > 0.0f)) {
        if (uvv) color_max_kernel<DFLOW_EVAL_UVV><<<nblocks, PIC_THREADS, 0, s>>>(flow, npix, w.partials);
        else color_max_kernel<DFLOW_EVAL_DYDX><<<nblocks, PIC_THREADS, 0, s>>>(flow, npix, w.partials);
        color_max_final_kernel<<<1, PIC_THREADS, 0, s>>>(w.partials, nblocks, w.radius);
    }
    if (uvv) color_kernel<DFLOW_EVAL_UVV><<<nblocks, PIC_THREADS, 0, s>>>(flow, npix, max_flow, w.radius, bgr, maxrad);
    else color_kernel<DFLOW_EVAL_DYDX><<<nblocks, PIC_THREADS, 0, s>>>(flow, npix, max_flow, w.radius, bgr, maxrad);
    return dflow_check_launch("flow colour kernels");
}

struct WarpWs {
    WarpPartial *partials;   // one per block of the main kernel
};

static WarpWs warp_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    WsCarver c(ws);
    WarpWs w;
    w.partials = c.take<WarpPartial>((size_t)plane_blocks(H, W));
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t warp_eval_ws_bytes(int H, int W) { size_t b; warp_ws(nullptr, H, W, &b); return b; }

int launch_warp_eval(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *flow, int layout, float err_thresh,
                     float err_max, uint32_t flags, dflow_photo_stats *stats, uint8_t *warped, float *err, uint8_t *err_bgr,
                     void *ws, hipStream_t s)
{
    const WarpWs w = warp_ws(ws, H, W);
    const int nblocks = plane_blocks(H, W);
    const unsigned npix = (unsigned)H * (unsigned)W;
    const WarpArgs A = {bgr1, bgr2, W, H, err_thresh, err_max};
    if (layout == DFLOW_EVAL_UVV)
        warp_main_kernel<DFLOW_EVAL_UVV><<<nblocks, PIC_THREADS, 0, s>>>(A, flow, npix, warped, err, err_bgr, w.partials);
    else
        warp_main_kernel<DFLOW_EVAL_DYDX><<<nblocks, PIC_THREADS, 0, s>>>(A, flow, npix, warped, err, err_bgr, w.partials);
    warp_final_kernel<<<1, PIC_THREADS, 0, s>>>(w.partials, nblocks, (flags & DFLOW_WARP_FLAG_ACCUMULATE) != 0, stats);
    return dflow_check_launch("warp evaluation kernels");
}
