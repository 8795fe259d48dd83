// Motion-compensated frame interpolation (include/dflow.h: dflow_frame_interp; DESIGN.md "Frame interpolation"): the frame at
// time t between two frames from the forward flow, or from both flows.  This build's definition; the reference has no counterpart.
//
//   fi_claim_kernel    one source per lane, blockIdx.z the side (0: a pixel of frame 1 with its forward vector, 1: a pixel of
//                      frame 2 with its backward vector).  A source whose end point is inside the other frame forms its
//                      photometric error there (bgr_bilinear, bgr_mean_abs_diff: plane_ops.h, dflow_warp_eval's) and claims the
//                      pixel it crosses at time t with a 64-bit atomicMin of error bits << 32 | source id
//   fi_resolve_kernel  one target per lane: the winner's vector, read again from its flow, into the motion plane
//   fi_fill_kernel     one Jacobi round: an unknown pixel takes the first known of up, left, right, down of the round's input
//   fi_render_kernel   one pixel per lane: both frames sampled along the pixel's motion, the occlusion switch, the frame, the
//                      provenance plane and the counts (block_count: plane_ops.h)
// 3 + fill_rounds launches and two memsets whatever the field holds.  The provenance of a pixel is not stored between the
// launches: a key names its side, and a known pixel without a key was filled.  One pixel per lane as in consistency.hip: the
// flows need only 4-byte alignment and every access but a lane's own pixel is a gather or a scatter.  One IEEE float32 operation
// per written operation (-ffp-contract=off).
#include <math.h>
#include "plane_ops.h"
#include "wave_ops.h"

#define FI_THREADS 256
#define FI_FREE 0xFFFFFFFFFFFFFFFFull
#define FI_COUNTS 8                                   // from frame 1, from frame 2, filled, unknown | blended, one-sided, fallback | lost

struct FiArgs {
    int h, w;
    float t, s, occl;                                 // s = 1 - t, formed once on the host
    const uint8_t *img[2];                            // frame 1, frame 2
    const float *flow[2];                             // forward, backward (NULL: forward only)
    int layout[2];
    unsigned long long *keys;
    int32_t *counts;                                  // NULL or FI_COUNTS
};

__global__ void __launch_bounds__(FI_THREADS) fi_claim_kernel(FiArgs a)
{
    const int side = blockIdx.z, h = a.h, w = a.w;
    const uint8_t *__restrict__ own = a.img[side];
    const uint8_t *__restrict__ other = a.img[side ^ 1];
    const float *__restrict__ flow = a.flow[side];
    const float step = side ? a.s : a.t;              // the share of the vector the source has travelled at time t
    const uint32_t n = (uint32_t)h * (uint32_t)w, i = blockIdx.x * FI_THREADS + threadIdx.x;
    bool part = false;
    float U, V;
    if (i < n && flow_good(flow, a.layout[side], (size_t)i, U, V)) {
        const int y = (int)(i / (uint32_t)w), x = (int)(i % (uint32_t)w);
        const float xs = (float)x + U, ys = (float)y + V;
        if (bgr_inside(xs, ys, w, h)) {
            const float px = rintf((float)x + step * U), py = rintf((float)y + step * V);      // ties to even
            if (px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1)) {
                float there[3], here[3];
                bgr_bilinear(other, w, h, xs, ys, there);
                const uint8_t *q = own + (size_t)i * 3;
                bgr_entry_floats((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), here);
                const float e = bgr_mean_abs_diff(there, here);                                // >= +0: its bits order like its value
                const unsigned long long key = ((unsigned long long)__float_as_uint(e) << 32) | (side ? n + i : i);
                atomicMin(&a.keys[(size_t)(int)py * w + (int)px], key);
                part = true;
            }
        }
    }
    // counts[7] holds the claimants until the resolve kernel takes the winners off
    const bool is[1] = {part};
    block_count<1>(is, a.counts, FI_COUNTS - 1);
}

__global__ void __launch_bounds__(FI_THREADS) fi_resolve_kernel(FiArgs a, float *__restrict__ motion)
{
    __shared__ int s_won;
    if (threadIdx.x == 0) s_won = 0;
    __syncthreads();
    const uint32_t n = (uint32_t)a.h * (uint32_t)a.w, i = blockIdx.x * FI_THREADS + threadIdx.x;
    bool won = false;
    if (i < n) {
        const unsigned long long key = a.keys[i];
        FlowOut m = {0.0f, 0.0f, 0.0f};
        if (key != FI_FREE) {
            const uint32_t id = (uint32_t)key;
            const int side = id >= n;
            float U, V;
            if (flow_good(a.flow[side], a.layout[side], (size_t)(side ? id - n : id), U, V)) {   // it was when it claimed
                m.u = side ? -U : U; m.v = side ? -V : V; m.valid = 1.0f;
                won = true;
            }
        }
        reinterpret_cast<FlowOut *>(motion)[i] = m;
    }
    if (a.counts) {
        const int c = wave_count(won);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_won, c);
        __syncthreads();
        if (threadIdx.x == 0 && s_won) atomicSub(&a.counts[FI_COUNTS - 1], s_won);
    }
}

__global__ void __launch_bounds__(FI_THREADS) fi_fill_kernel(int h, int w, const float *__restrict__ in, float *__restrict__ out)
{
    const uint32_t n = (uint32_t)h * (uint32_t)w, i = blockIdx.x * FI_THREADS + threadIdx.x;
    if (i >= n) return;
    const FlowOut *__restrict__ f = reinterpret_cast<const FlowOut *>(in);
    const int y = (int)(i / (uint32_t)w), x = (int)(i % (uint32_t)w);
    FlowOut m = f[i];
    if (m.valid == 0.0f) {
        // up, left, right, down: the first that was known before this round
        const bool has[4] = {y > 0, x > 0, x < w - 1, y < h - 1};
        const uint32_t at[4] = {i - (uint32_t)w, i - 1u, i + 1u, i + (uint32_t)w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (m.valid == 0.0f && has[k]) {
                const FlowOut q = f[at[k]];
                if (q.valid != 0.0f) m = q;
            }
        }
    }
    reinterpret_cast<FlowOut *>(out)[i] = m;
}

__global__ void __launch_bounds__(FI_THREADS) fi_render_kernel(FiArgs a, const float *__restrict__ motion, uint8_t *__restrict__ out,
                                                               uint8_t *__restrict__ source)
{
    const int h = a.h, w = a.w;
    const uint32_t n = (uint32_t)h * (uint32_t)w, i = blockIdx.x * FI_THREADS + threadIdx.x;
    bool is[FI_COUNTS - 1] = {};
    if (i < n) {
        const int y = (int)(i / (uint32_t)w), x = (int)(i % (uint32_t)w);
        const FlowOut m = reinterpret_cast<const FlowOut *>(motion)[i];
        const unsigned long long key = a.keys[i];
        const bool known = m.valid != 0.0f;
        const int src = key != FI_FREE ? ((uint32_t)key >= n ? 2 : 1) : (known ? 3 : 0);
        float v[3];
        int how = 2;                                                                    // 0 blended, 1 one-sided, 2 fallback
        if (known) {
            const float x1 = (float)x - a.t * m.u, y1 = (float)y - a.t * m.v;
            const float x2 = (float)x + a.s * m.u, y2 = (float)y + a.s * m.v;
            const bool use1 = bgr_inside(x1, y1, w, h), use2 = bgr_inside(x2, y2, w, h);
            float c1[3], c2[3];
            if (use1) bgr_bilinear(a.img[0], w, h, x1, y1, c1);
            if (use2) bgr_bilinear(a.img[1], w, h, x2, y2, c2);
            if (use1 && use2) {
                if (bgr_mean_abs_diff(c1, c2) <= a.occl) {
                    how = 0;
#pragma unroll
                    for (int c = 0; c < 3; c++) v[c] = a.s * c1[c] + a.t * c2[c];
                } else {
                    // the two frames disagree: the claimant's frame; a filled pixel takes the frame nearer in time
                    how = 1;
                    const bool first = src == 1 || (src == 3 && a.t <= 0.5f);
#pragma unroll
                    for (int c = 0; c < 3; c++) v[c] = first ? c1[c] : c2[c];
                }
            } else if (use1 || use2) {
                how = 1;
#pragma unroll
                for (int c = 0; c < 3; c++) v[c] = use1 ? c1[c] : c2[c];
            }
        }
        if (how == 2) {
            const uint8_t *p = a.img[0] + (size_t)i * 3, *q = a.img[1] + (size_t)i * 3;
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = a.s * (float)p[c] + a.t * (float)q[c];
        }
        bgr_store1(out, (size_t)i, bgr_round_entry(v));
        if (source) source[i] = (uint8_t)src;
        const int from = src == 0 ? 3 : src - 1;
#pragma unroll
        for (int k = 0; k < 4; k++) is[k] = from == k;
#pragma unroll
        for (int k = 0; k < 3; k++) is[4 + k] = how == k;
    }
    block_count<FI_COUNTS - 1>(is, a.counts, 0);
}

int launch_frame_interp(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *fwd, int layout_fwd, const float *bwd,
                        int layout_bwd, float t, int fill_rounds, float occl_thresh, uint8_t *out, uint64_t *keys, float *motion,
                        float *motion_tmp, uint8_t *source, int32_t *counts, hipStream_t s)
{
    const size_t n = (size_t)H * W;
    DFLOW_HIP(hipMemsetAsync(keys, 0xFF, n * sizeof(uint64_t), s));
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, FI_COUNTS * sizeof(int32_t), s));
    FiArgs a;
    a.h = H; a.w = W; a.t = t; a.s = 1.0f - t; a.occl = occl_thresh;
    a.img[0] = bgr1; a.img[1] = bgr2; a.flow[0] = fwd; a.flow[1] = bwd; a.layout[0] = layout_fwd; a.layout[1] = layout_bwd;
    a.keys = reinterpret_cast<unsigned long long *>(keys); a.counts = counts;
    const unsigned blocks = (unsigned)((n + FI_THREADS - 1) / FI_THREADS);
    hipLaunchKernelGGL(fi_claim_kernel, dim3(blocks, 1, bwd ? 2 : 1), dim3(FI_THREADS), 0, s, a);
    // the rounds alternate between the two planes and the last one writes d_motion: an odd number of them starts in d_motion_tmp
    float *cur = (fill_rounds & 1) ? motion_tmp : motion, *nxt = (fill_rounds & 1) ? motion : motion_tmp;
    hipLaunchKernelGGL(fi_resolve_kernel, dim3(blocks), dim3(FI_THREADS), 0, s, a, cur);
    for (int r = 0; r < fill_rounds; r++) {
        hipLaunchKernelGGL(fi_fill_kernel, dim3(blocks), dim3(FI_THREADS), 0, s, H, W, (const float *)cur, nxt);
        float *tmp = cur; cur = nxt; nxt = tmp;
    }
    hipLaunchKernelGGL(fi_render_kernel, dim3(blocks), dim3(FI_THREADS), 0, s, a, (const float *)cur, out, source);
    return dflow_check_launch("frame interpolation kernels");
}
