// What the random-sample fits of a flow field share (motion_fit.hip, epipolar.hip), whatever the model is: the arguments every
// kernel of a fit takes, the test whether a pixel takes part, the grid of scored pixels, a model's nine coefficients, and the
// block's count of a flag.  One definition each; the models, their solves and their score loops are the files' own.
#pragma once
#include "plane_ops.h"
#include "philox.h"

struct MfArgs {
    int h, w, layout, model, n_hyp, step, ws;         // ws: scored columns, ceil(w / step)
    uint32_t n, ns;                                   // pixels, grid points (y % step == 0 && x % step == 0)
    uint32_t k0, k1;
    float thresh;
    double cx, cy, s, inv;                            // the centre, 1 / P and P, P the power of two >= max(h, w)
    const float *flow;
    const uint8_t *exclude;
    float *cur;                                       // d_model: the current model
    float *models;
    int32_t *hyp_counts;
    unsigned long long *state;
};

__device__ static inline bool mf_part(const MfArgs &a, uint32_t i, float &U, float &V)
{
    return flow_good(a.flow, a.layout, (size_t)i, U, V) && !(a.exclude && a.exclude[i]);
}

__device__ static inline void mf_load_model(const float *__restrict__ p, float (&m)[9])
{
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = p[k];
}

// grid point c -> its pixel
__device__ static inline uint32_t mf_grid_pixel(const MfArgs &a, uint32_t c, int &x, int &y)
{
    y = (int)(c / (uint32_t)a.ws) * a.step; x = (int)(c % (uint32_t)a.ws) * a.step;
    return (uint32_t)y * (uint32_t)a.w + (uint32_t)x;
}

// how many lanes of the block have `is`, added to *slot: ballots -> LDS -> one 64-bit integer atomic per block
__device__ static inline void mf_block_add(bool is, unsigned long long *slot)
{
    __shared__ int s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const int c = __popcll(__ballot(is));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_c) atomicAdd(slot, (unsigned long long)s_c);
    __syncthreads();
}
