// Flow evaluation, after errorImage of visualization.py:128-156: end-point error statistics of a test flow against a ground
// truth, the per-pixel error plane and the reference's colour error picture (include/dflow.h, DESIGN.md "Flow evaluation").
// One IEEE float32 operation per written operation (-ffp-contract=off; hipcc's sqrtf and / are correctly rounded).
//
// Two launches on the caller's stream, nothing read back, no atomics:
//   eval_main_kernel<LAYOUT>  the planes as flat arrays of h*w pixels, four pixels per lane and step: three (DYDX: two)
//                             16-byte loads of the test field, three of the ground truth, one 16-byte store of err, one
//                             12-byte store of the picture (flow_load4, bgr_pack4: plane_ops.h).  The last group of a field
//                             whose h*w is no multiple of 4 goes pixel by pixel.  Grid-stride over at most PLANE_MAX_BLOCKS
//                             blocks; every lane keeps its own counts, maximum and double sum, which block_reduce
//                             (plane_ops.h) adds in a fixed order, and thread 0 writes the block's partial.
//   eval_final_kernel         one block: thread t adds the partials t, t + 256, ... in that order, the same block
//                             reduction, and thread 0 writes or (DFLOW_EVAL_FLAG_ACCUMULATE) adds to *d_stats.
// The grid is a function of h*w alone, so the order of every double addition is fixed: the same inputs give the same
// bits of sum_err on every call.
#include "plane_ops.h"

#define EVAL_THREADS PLANE_THREADS    // plane_blocks counts blocks of this size
#define EVAL_WAVES (EVAL_THREADS / 64)

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

template <int LAYOUT>
__global__ void __launch_bounds__(EVAL_THREADS) eval_main_kernel(const float *__restrict__ test, const float *__restrict__ gt,
                                                                 unsigned npix, float abs_thresh, float *__restrict__ err,
                                                                 uint8_t *__restrict__ bgr, EvalPartial *__restrict__ partials)
{
    __shared__ uint32_t lut_s[256];
    const uint32_t *lut = nullptr;
    if (bgr) {                                          // uniform
        lut_s[threadIdx.x] = plane_jet_lut[threadIdx.x];
        __syncthreads();
        lut = lut_s;
    }
    EvalPartial acc = {};
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    for (unsigned g = blockIdx.x * EVAL_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * EVAL_THREADS) {
        float e[4];
        uint32_t c[4];
        if (g < nfull) {
            float tU[4], tV[4], tvalid[4], gU[4], gV[4], gvalid[4];
            flow_load4<DFLOW_EVAL_UVV>(gt, g, gU, gV, gvalid);
            flow_load4<LAYOUT>(test, g, tU, tV, tvalid);
#pragma unroll
            for (int k = 0; k < 4; k++) eval_pixel(tU[k], tV[k], tvalid[k], gU[k], gV[k], gvalid[k], abs_thresh, lut, acc, e[k], c[k]);
            if (err) reinterpret_cast<float4 *>(err)[g] = make_float4(e[0], e[1], e[2], e[3]);
            if (bgr) reinterpret_cast<Bgr4 *>(bgr)[g] = bgr_pack4(c);
        } else {
            // the 1..3 pixels after the last whole group
            for (unsigned p = g * 4u; p < npix; p++) {
                float tU, tV, tvalid, gU, gV, gvalid, e1;
                uint32_t c1;
                flow_load1<LAYOUT>(test, p, tU, tV, tvalid);
                flow_load1<DFLOW_EVAL_UVV>(gt, p, gU, gV, gvalid);
                eval_pixel(tU, tV, tvalid, gU, gV, gvalid, abs_thresh, lut, acc, e1, c1);
                if (err) err[p] = e1;
                if (bgr) bgr_store1(bgr, p, c1);
            }
        }
    }
    acc = block_reduce<EVAL_WAVES>(acc, eval_merge);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(EVAL_THREADS) eval_final_kernel(const EvalPartial *__restrict__ partials, int nblocks,
                                                                  int accumulate, dflow_eval_stats *__restrict__ stats)
{
    EvalPartial acc = {};
    // counts of the whole field: up to 2^26, and 32 bits hold them
    for (int b = threadIdx.x; b < nblocks; b += EVAL_THREADS) eval_merge(acc, partials[b]);
    acc = block_reduce<EVAL_WAVES>(acc, eval_merge);
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

struct EvalWs {
    EvalPartial *partials;   // one per block of the main kernel
};

static EvalWs eval_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    WsCarver c(ws);
    EvalWs w;
    w.partials = c.take<EvalPartial>((size_t)plane_blocks(H, W));
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t eval_ws_bytes(int H, int W) { size_t b; eval_ws(nullptr, H, W, &b); return b; }

int launch_flow_eval(int H, int W, const float *test, int layout, const float *gt, float abs_thresh, uint32_t flags,
                     dflow_eval_stats *stats, float *err, uint8_t *bgr, void *ws, hipStream_t s)
{
    const EvalWs w = eval_ws(ws, H, W);
    const int nblocks = plane_blocks(H, W);
    const unsigned npix = (unsigned)H * (unsigned)W;
    if (layout == DFLOW_EVAL_UVV)
        eval_main_kernel<DFLOW_EVAL_UVV><<<nblocks, EVAL_THREADS, 0, s>>>(test, gt, npix, abs_thresh, err, bgr, w.partials);
    else
        eval_main_kernel<DFLOW_EVAL_DYDX><<<nblocks, EVAL_THREADS, 0, s>>>(test, gt, npix, abs_thresh, err, bgr, w.partials);
    eval_final_kernel<<<1, EVAL_THREADS, 0, s>>>(w.partials, nblocks, (flags & DFLOW_EVAL_FLAG_ACCUMULATE) != 0, stats);
    return dflow_check_launch("flow evaluation kernels");
}
