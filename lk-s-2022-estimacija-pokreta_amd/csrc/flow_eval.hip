// Flow evaluation, after errorImage of visualization.py:128-156: end-point error statistics of a test flow against a ground
// truth, the per-pixel error plane and the reference's colour error picture (include/dflow.h, DESIGN.md "Flow evaluation").
// One IEEE float32 operation per written operation (-ffp-contract=off; hipcc's sqrtf and / are correctly rounded).
//
// Two launches on the caller's stream, nothing read back, no atomics:
//   eval_main_kernel<LAYOUT>  the planes as flat arrays of h*w pixels, four pixels per lane and step: three (DYDX: two)
//                             16-byte loads of the test field, three of the ground truth, one 16-byte store of err, one
//                             12-byte store of the picture.  The last group of a field whose h*w is no multiple of 4 goes
//                             pixel by pixel.  Grid-stride over at most EVAL_MAX_BLOCKS blocks; every lane keeps its own
//                             counts, maximum and double sum, which are reduced across the wave by shuffles in a fixed tree,
//                             across the block's waves through LDS in wave order, and written as the block's partial.
//   eval_final_kernel         one block: thread t adds the partials t, t + 256, ... in that order, the same block
//                             reduction, and thread 0 writes or (DFLOW_EVAL_FLAG_ACCUMULATE) adds to *d_stats.
// The grid is a function of h*w alone, so the order of every double addition is fixed: the same inputs give the same
// bits of sum_err on every call.
#include "dflow_common.h"
#include "jet_lut.h"

#define EVAL_THREADS 256
#define EVAL_WAVES (EVAL_THREADS / 64)
#define EVAL_MAX_BLOCKS 1024          // 4 blocks of 256 threads on each of the 256 CUs

__constant__ uint32_t eval_jet_lut[256] = {JET_LUT_VALUES};

// what a lane, a wave or a block has seen; a block of a 8192 x 8192 field sees at most 2^26 pixels: 32-bit counts
struct EvalPartial {
    double sum;
    uint32_t n, n_out_abs, n_out_kitti, n_nonfinite, n_gt_valid, n_test_valid;
    float max_err;
    uint32_t pad;
};

__device__ __forceinline__ static void eval_merge(EvalPartial &a, const EvalPartial &b)
{
    a.sum = a.sum + b.sum;
    a.n += b.n; a.n_out_abs += b.n_out_abs; a.n_out_kitti += b.n_out_kitti;
    a.n_nonfinite += b.n_nonfinite; a.n_gt_valid += b.n_gt_valid; a.n_test_valid += b.n_test_valid;
    a.max_err = fmaxf(a.max_err, b.max_err);
}

// the block's total in thread 0: a shuffle tree per wave (64 lanes: offsets 32 .. 1), then the waves in order
__device__ static EvalPartial eval_block_reduce(EvalPartial a)
{
    __shared__ EvalPartial wave_part[EVAL_WAVES];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        EvalPartial b;
        b.sum = __shfl_down(a.sum, off, 64);
        b.n = __shfl_down(a.n, off, 64); b.n_out_abs = __shfl_down(a.n_out_abs, off, 64);
        b.n_out_kitti = __shfl_down(a.n_out_kitti, off, 64); b.n_nonfinite = __shfl_down(a.n_nonfinite, off, 64);
        b.n_gt_valid = __shfl_down(a.n_gt_valid, off, 64); b.n_test_valid = __shfl_down(a.n_test_valid, off, 64);
        b.max_err = __shfl_down(a.max_err, off, 64);
        eval_merge(a, b);
    }
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < EVAL_WAVES; k++) eval_merge(a, wave_part[k]);
    }
    return a;
}

// one pixel: counts it into `acc` and returns its err (-1 when it is not compared) and its picture entry (b | g << 8 | r << 16)
__device__ __forceinline__ static void eval_pixel(float tU, float tV, float tvalid, float gU, float gV, float gvalid,
                                                  float abs_thresh, const uint32_t *lut, EvalPartial &acc, float &err_out,
                                                  uint32_t &bgr_out)
{
    const bool gv = gvalid > 0.5f, tv = tvalid > 0.5f;
    acc.n_gt_valid += gv; acc.n_test_valid += tv;
    err_out = -1.0f; bgr_out = 0u;
    if (!(gv && tv)) return;
    const float dfu = tU - gU, dfv = tV - gV;
    const float err = sqrtf(dfu * dfu + dfv * dfv);
    // one NaN for every NaN, whatever produced it; chosen on the bits (the compiler may drop a float select between NaNs)
    const uint32_t ebits = __float_as_uint(err);
    err_out = __uint_as_float((ebits & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : ebits);
    if (!(fabsf(err) < INFINITY)) { acc.n_nonfinite++; return; }       // NaN or Inf
    acc.n++;
    acc.sum = acc.sum + (double)err;
    acc.max_err = fmaxf(acc.max_err, err);
    acc.n_out_abs += err > abs_thresh;
    acc.n_out_kitti += err > 3.0f && err > 0.05f * sqrtf(gU * gU + gV * gV);
    if (lut) {
        const float t = fminf(err, 3.0f) / 3.0f;
        bgr_out = lut[min(255, (int)(t * 256.0f))];
    }
}

struct EvalBgr4 { uint32_t a, b, c; };      // four (b, g, r) pixels: 12 bytes

template <int LAYOUT>
__global__ void __launch_bounds__(EVAL_THREADS) eval_main_kernel(const float *__restrict__ test, const float *__restrict__ gt,
                                                                 unsigned npix, float abs_thresh, float *__restrict__ err,
                                                                 uint8_t *__restrict__ bgr, EvalPartial *__restrict__ partials)
{
    __shared__ uint32_t lut_s[256];
    const uint32_t *lut = nullptr;
    if (bgr) {                                          // uniform
        lut_s[threadIdx.x] = eval_jet_lut[threadIdx.x];
        __syncthreads();
        lut = lut_s;
    }
    EvalPartial acc = {};
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    for (unsigned g = blockIdx.x * EVAL_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * EVAL_THREADS) {
        float e[4];
        uint32_t c[4];
        if (g < nfull) {
            const float4 *gp = reinterpret_cast<const float4 *>(gt) + (size_t)g * 3;
            const float4 g0 = gp[0], g1 = gp[1], g2 = gp[2];
            const float G[12] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
            if constexpr (LAYOUT == DFLOW_EVAL_UVV) {
                const float4 *tp = reinterpret_cast<const float4 *>(test) + (size_t)g * 3;
                const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
                const float T[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
                for (int k = 0; k < 4; k++)
                    eval_pixel(T[3 * k], T[3 * k + 1], T[3 * k + 2], G[3 * k], G[3 * k + 1], G[3 * k + 2], abs_thresh, lut, acc, e[k], c[k]);
            } else {
                const float4 *tp = reinterpret_cast<const float4 *>(test) + (size_t)g * 2;
                const float4 t0 = tp[0], t1 = tp[1];
                const float T[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};       // [dy,dx]: U = dx, V = dy
#pragma unroll
                for (int k = 0; k < 4; k++)
                    eval_pixel(T[2 * k + 1], T[2 * k], 1.0f, G[3 * k], G[3 * k + 1], G[3 * k + 2], abs_thresh, lut, acc, e[k], c[k]);
            }
            if (err) reinterpret_cast<float4 *>(err)[g] = make_float4(e[0], e[1], e[2], e[3]);
            if (bgr) {
                EvalBgr4 v;
                v.a = c[0] | (c[1] << 24);
                v.b = (c[1] >> 8) | (c[2] << 16);
                v.c = (c[2] >> 16) | (c[3] << 8);
                reinterpret_cast<EvalBgr4 *>(bgr)[g] = v;
            }
        } else {
            // the 1..3 pixels after the last whole group
            for (unsigned p = g * 4u; p < npix; p++) {
                const float *gq = gt + (size_t)p * 3;
                float tU, tV, tvalid = 1.0f, e1;
                uint32_t c1;
                if constexpr (LAYOUT == DFLOW_EVAL_UVV) { tU = test[(size_t)p * 3]; tV = test[(size_t)p * 3 + 1]; tvalid = test[(size_t)p * 3 + 2]; }
                else { tU = test[(size_t)p * 2 + 1]; tV = test[(size_t)p * 2]; }
                eval_pixel(tU, tV, tvalid, gq[0], gq[1], gq[2], abs_thresh, lut, acc, e1, c1);
                if (err) err[p] = e1;
                if (bgr) {
                    bgr[(size_t)p * 3] = (uint8_t)c1; bgr[(size_t)p * 3 + 1] = (uint8_t)(c1 >> 8); bgr[(size_t)p * 3 + 2] = (uint8_t)(c1 >> 16);
                }
            }
        }
    }
    acc = eval_block_reduce(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(EVAL_THREADS) eval_final_kernel(const EvalPartial *__restrict__ partials, int nblocks,
                                                                  int accumulate, dflow_eval_stats *__restrict__ stats)
{
    EvalPartial acc = {};
    // counts of the whole field: up to 2^26, and 32 bits hold them
    for (int b = threadIdx.x; b < nblocks; b += EVAL_THREADS) eval_merge(acc, partials[b]);
    acc = eval_block_reduce(acc);
    if (threadIdx.x != 0) return;
    dflow_eval_stats s = {};
    if (accumulate) s = *stats;
    s.n += acc.n; s.n_out_abs += acc.n_out_abs; s.n_out_kitti += acc.n_out_kitti; s.n_nonfinite += acc.n_nonfinite;
    s.n_gt_valid += acc.n_gt_valid; s.n_test_valid += acc.n_test_valid;
    s.sum_err = s.sum_err + acc.sum;
    s.max_err = fmaxf(s.max_err, acc.max_err);
    s.reserved = 0;
    *stats = s;
}

static int eval_blocks(int H, int W)
{
    const size_t ngroups = ((size_t)H * W + 3) / 4;
    const size_t b = (ngroups + EVAL_THREADS - 1) / EVAL_THREADS;
    return (int)(b < EVAL_MAX_BLOCKS ? b : EVAL_MAX_BLOCKS);
}

struct EvalWs {
    EvalPartial *partials;   // one per block of the main kernel
};

static EvalWs eval_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    WsCarver c(ws);
    EvalWs w;
    w.partials = c.take<EvalPartial>((size_t)eval_blocks(H, W));
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t eval_ws_bytes(int H, int W) { size_t b; eval_ws(nullptr, H, W, &b); return b; }

int launch_flow_eval(int H, int W, const float *test, int layout, const float *gt, float abs_thresh, uint32_t flags,
                     dflow_eval_stats *stats, float *err, uint8_t *bgr, void *ws, hipStream_t s)
{
    const EvalWs w = eval_ws(ws, H, W);
    const int nblocks = eval_blocks(H, W);
    const unsigned npix = (unsigned)H * (unsigned)W;
    if (layout == DFLOW_EVAL_UVV)
        eval_main_kernel<DFLOW_EVAL_UVV><<<nblocks, EVAL_THREADS, 0, s>>>(test, gt, npix, abs_thresh, err, bgr, w.partials);
    else
        eval_main_kernel<DFLOW_EVAL_DYDX><<<nblocks, EVAL_THREADS, 0, s>>>(test, gt, npix, abs_thresh, err, bgr, w.partials);
    eval_final_kernel<<<1, EVAL_THREADS, 0, s>>>(w.partials, nblocks, (flags & DFLOW_EVAL_FLAG_ACCUMULATE) != 0, stats);
    return dflow_check_launch("flow evaluation kernels");
}
