// The forward/backward check in image coordinates (include/dflow.h: dflow_flow_consistency; DESIGN.md "Forward/backward check in
// image coordinates"): the vector at p against the other direction's vector at p + f(p).  This build's definition; the reference's
// check (post.hip, dflow_fb_consistency) adds U to the row and V to the column and stays what it is.
//
// consistency_kernel: one pixel per lane, blockIdx.z the direction (0: d_fwd checked against d_bwd, 1: the roles swapped).  The
// lane's own vector and the one (nearest) or up to four (bilinear) vectors at its target through flow_good (dflow_common.h),
// 12 bytes out, 4 more with an error plane; the five counts through block_count_class (plane_ops.h).  One IEEE float32
// operation per written operation (-ffp-contract=off; hipcc's sqrtf is correctly rounded).
#include <math.h>
#include "plane_ops.h"

#define FBC_THREADS 256
#define FBC_CLASSES 5                                 // CONSISTENT, ABOVE, BWD_INVALID, OUTSIDE, FWD_INVALID

struct FbcArgs {
    int h, w;
    float thresh;
    uint32_t flags;
    const float *src[2];                              // per direction: the field that is checked ...
    const float *other[2];                            // ... and the one it is checked against
    int layout_src[2], layout_other[2];
    float *out[2], *err[2];
    int32_t *counts;                                  // NULL, or FBC_CLASSES per direction
};

__global__ void __launch_bounds__(FBC_THREADS) consistency_kernel(FbcArgs a)
{
    const int dir = blockIdx.z;
    const float *__restrict__ src = a.src[dir];
    const float *__restrict__ other = a.other[dir];
    const int ls = a.layout_src[dir], lo = a.layout_other[dir];
    const int h = a.h, w = a.w;
    const uint32_t n = (uint32_t)h * (uint32_t)w, i = blockIdx.x * FBC_THREADS + threadIdx.x;
    int kind = -1;
    if (i < n) {
        const int y = (int)(i / (uint32_t)w), x = (int)(i % (uint32_t)w);
        float U = 0.0f, V = 0.0f, bu = 0.0f, bv = 0.0f;
        kind = 4;                                                                       // FWD_INVALID
        if (flow_good(src, ls, (size_t)i, U, V)) {
            kind = 3;                                                                   // OUTSIDE
            if (a.flags & DFLOW_FBC_BILINEAR) {
                const float py = (float)y + V, px = (float)x + U;
                if (py >= 0.0f && py <= (float)(h - 1) && px >= 0.0f && px <= (float)(w - 1)) {
                    // 0 <= y0 <= h-1, and ay > 0 only below h-1: every corner that is read lies inside the frame
                    const int y0 = (int)floorf(py), x0 = (int)floorf(px);
                    const float ay = py - (float)y0, ax = px - (float)x0;
                    const int y1 = ay > 0.0f ? y0 + 1 : y0, x1 = ax > 0.0f ? x0 + 1 : x0;
                    float u00, v00, u01, v01, u10, v10, u11, v11;
                    const bool g00 = flow_good(other, lo, (size_t)y0 * w + x0, u00, v00);
                    const bool g01 = flow_good(other, lo, (size_t)y0 * w + x1, u01, v01);
                    const bool g10 = flow_good(other, lo, (size_t)y1 * w + x0, u10, v10);
                    const bool g11 = flow_good(other, lo, (size_t)y1 * w + x1, u11, v11);
                    kind = 2;                                                           // BWD_INVALID
                    if (g00 && g01 && g10 && g11) {
                        const float tu = u00 + ax * (u01 - u00), bu_ = u10 + ax * (u11 - u10);
                        const float tv = v00 + ax * (v01 - v00), bv_ = v10 + ax * (v11 - v10);
                        bu = tu + ay * (bu_ - tu);
                        bv = tv + ay * (bv_ - tv);
                        kind = 1;
                    }
                }
            } else {
                const float ry = rintf(V), rx = rintf(U);                               // ties to even
                if (fabsf(ry) <= 32767.0f && fabsf(rx) <= 32767.0f) {
                    const int ty = y + (int)ry, tx = x + (int)rx;
                    if (ty >= 0 && ty < h && tx >= 0 && tx < w) {
                        kind = flow_good(other, lo, (size_t)ty * w + tx, bu, bv) ? 1 : 2;
                    }
                }
            }
        }
        FlowOut o = {0.0f, 0.0f, 0.0f};
        float err = -1.0f;
        if (kind == 1) {                                                                // ABOVE unless err <= thresh (a NaN is above)
            const float du = U + bu, dv = V + bv;
            err = sqrtf(du * du + dv * dv);
            if (err <= a.thresh) { o.u = U; o.v = V; o.valid = 1.0f; kind = 0; }
        }
        reinterpret_cast<FlowOut *>(a.out[dir])[i] = o;
        if (a.err[dir]) a.err[dir][i] = err;
    }
    block_count_class<FBC_CLASSES>(kind, a.counts, dir * FBC_CLASSES);
}

int launch_flow_consistency(int H, int W, const float *fwd, int layout_fwd, const float *bwd, int layout_bwd, float thresh,
                            uint32_t flags, float *out_fwd, float *out_bwd, float *err_fwd, float *err_bwd, int32_t *counts,
                            hipStream_t s)
{
    const int ndir = out_bwd ? 2 : 1;
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, ndir * FBC_CLASSES * sizeof(int32_t), s));
    FbcArgs a;
    a.h = H; a.w = W; a.thresh = thresh; a.flags = flags; a.counts = counts;
    a.src[0] = fwd; a.other[0] = bwd; a.layout_src[0] = layout_fwd; a.layout_other[0] = layout_bwd;
    a.src[1] = bwd; a.other[1] = fwd; a.layout_src[1] = layout_bwd; a.layout_other[1] = layout_fwd;
    a.out[0] = out_fwd; a.out[1] = out_bwd; a.err[0] = err_fwd; a.err[1] = err_bwd;
    const unsigned n = (unsigned)H * (unsigned)W;
    hipLaunchKernelGGL(consistency_kernel, dim3((n + FBC_THREADS - 1) / FBC_THREADS, 1, ndir), dim3(FBC_THREADS), 0, s, a);
    return dflow_check_launch("consistency_kernel");
}
