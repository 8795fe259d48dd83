// What the fits of a flow field share (motion_fit.hip, epipolar.hip, the segment fit of superpixels.hip, two_view.hip), whatever
// the model is.  One definition each of:
//   the constants     FIT_THREADS, FIT_CHUNK, FIT_ATTEMPTS, FIT_PIVOT_MIN, FIT_DEGENERATE, FIT_NSUMS, FIT_RANGE
//                     (the packed pair of float32 the score loops use is dflow_common.h's dflow_f2)
//   the arguments     MfArgs, and on the host fit_frame (frame, grid of scored pixels, normalisation) and fit_clear (the memsets)
//   a pixel           mf_part (takes part), mf_grid_pixel (the grid of scored pixels), mf_load_model (nine coefficients)
//   a sample point    fit_draw: the Philox attempts, takes part, no duplicate, accepted by the caller's predicate
//   a chunk           fit_stage_chunk: the scored pixels of a block in LDS as packed pairs
//   the best key      fit_key and its three fields, fit_offer (the best kernels), fit_adopt (the select kernels), fit_counts
//   the classes       fit_class, fit_scored (the apply kernels)
//   the affine solve  fit_affine_from_sums: step E of the motion fit (include/dflow.h), which the segment fit uses too
//   the block's sums  fit_block_add
// None of them knows which file calls it; the models, their solves, their score loops and their kernels are the files' own.
#pragma once
#include <math.h>
#include "plane_ops.h"
#include "philox.h"

#define FIT_THREADS 256
#define FIT_CHUNK 2048                                // scored pixels a block stages: 32 KiB of LDS, four blocks per CU
#define FIT_ATTEMPTS 16
#define FIT_PIVOT_MIN 9.094947017729282e-13           // 2^-40, in coordinates scaled to [-1/2, 1/2]
#define FIT_DEGENERATE INT32_MIN
#define FIT_NSUMS 12
#define FIT_RANGE 32768.0f                            // |target| or |flow| above it stays out of the int64 sums
#define FIT_S_BEST 0                                  // d_state[0] of a random-sample fit: the best key

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

// the frame, the grid of scored pixels and the normalisation; every other field zero, for the caller to set
static inline MfArgs fit_frame(int H, int W, int layout, int step, const float *flow, int64_t *state)
{
    MfArgs a = {};
    a.h = H; a.w = W; a.layout = layout; a.step = step; a.ws = (W + step - 1) / step;
    a.n = (uint32_t)H * (uint32_t)W; a.ns = (uint32_t)((H + step - 1) / step) * (uint32_t)a.ws;
    double P = 1.0;
    while (P < (double)(H > W ? H : W)) P *= 2.0;
    a.cx = (double)(W - 1) * 0.5; a.cy = (double)(H - 1) * 0.5; a.s = 1.0 / P; a.inv = P;
    a.flow = flow; a.state = reinterpret_cast<unsigned long long *>(state);
    return a;
}

// d_state (int64[32]) and, where given, d_counts (int32[8]) zeroed
static inline int fit_clear(int64_t *state, int32_t *counts, hipStream_t s)
{
    DFLOW_HIP(hipMemsetAsync(state, 0, 32 * sizeof(int64_t), s));
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int32_t), s));
    return DFLOW_OK;
}

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

// SAMPLE (include/dflow.h): point k of sample j, STRIDE the counter slots a round reserves per sample.  Up to FIT_ATTEMPTS
// draws, the first that takes part, is none of idx[0..k-1] and, in a round > 0, that accept(xf, yf, U, V) takes; it becomes idx[k]
template <int STRIDE, int M, typename Accept>
__device__ __forceinline__ static bool fit_draw(const MfArgs &a, int j, int round, int k, uint32_t (&idx)[M], float &xf, float &yf,
                                                float &U, float &V, Accept accept)
{
    bool found = false;
    for (int att = 0; att < FIT_ATTEMPTS && !found; att++) {
        uint32_t u, u1;
        philox4x32_10((uint32_t)j, (uint32_t)((round * STRIDE + k) * FIT_ATTEMPTS + att), a.k0, a.k1, u, u1);
        const uint32_t i = (uint32_t)(((uint64_t)u * (uint64_t)a.n) >> 32);
        if (!mf_part(a, i, U, V)) continue;
        bool dup = false;
        for (int q = 0; q < k; q++) dup |= idx[q] == i;
        if (dup) continue;
        xf = (float)(int)(i % (uint32_t)a.w); yf = (float)(int)(i / (uint32_t)a.w);
        if (round > 0 && !accept(xf, yf, U, V)) continue;
        idx[k] = i;
        found = true;
    }
    return found;
}

// A block's chunk of CHUNK grid points into s_px, the pixels that take no part dropped: pixel t of the chunk is the four values
// coords(x, y, U, V, v) gives, v[c] at float 8 (t / 2) + 2 c + t % 2, so that a pair of pixels is two 16-byte words.  An odd
// count is padded with a pixel whose v[2] and v[3] are NaN (no inlier of anything).  Returns the count; ends in a barrier.
template <int CHUNK, int THREADS, typename Coords>
__device__ __forceinline__ static int fit_stage_chunk(const MfArgs &a, float4 (&s_px)[CHUNK], int &s_n, Coords coords)
{
    float *px = reinterpret_cast<float *>(s_px);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)CHUNK;
    for (int t = threadIdx.x; t < CHUNK; t += THREADS) {
        const uint32_t c = base + (uint32_t)t;
        if (c >= a.ns) break;
        int x, y;
        const uint32_t i = mf_grid_pixel(a, c, x, y);
        float U, V;
        if (mf_part(a, i, U, V)) {
            float v[4];
            coords(x, y, U, V, v);
            const int slot = atomicAdd(&s_n, 1);                      // at most CHUNK grid points per block
            float *q = px + (slot >> 1) * 8 + (slot & 1);
            q[0] = v[0]; q[2] = v[1]; q[4] = v[2]; q[6] = v[3];
        }
    }
    __syncthreads();
    const int np = s_n;
    if (threadIdx.x == 0 && (np & 1)) {                               // the other half of the last pair
        float *q = px + (np >> 1) * 8 + 1;
        q[0] = 0.0f; q[2] = 0.0f; q[4] = __builtin_nanf(""); q[6] = __builtin_nanf("");
    }
    __syncthreads();
    return np;
}

// N counts a wave has summed from its ballots, added to slots[0..N-1]: -> LDS -> one 64-bit integer atomic per block and count.
// A single flag: fit_block_add({wave_count(is)}, slot), with wave_ops.h's count.  Calls may follow one another without a barrier
// between them: outside the two barriers word k is touched by thread k alone, which reads it here before it clears it in the next
// call, and no wave of the next call adds before thread k has come to that call's first barrier.  (Calls with another N have
// words of their own.)
template <int N> __device__ __forceinline__ static void fit_block_add(const int (&w)[N], unsigned long long *slots)
{
    __shared__ int s_c[N];
    if (threadIdx.x < N) s_c[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++)
            if (w[k]) atomicAdd(&s_c[k], w[k]);
    }
    __syncthreads();
    if (threadIdx.x < N && s_c[threadIdx.x]) atomicAdd(&slots[threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
}

// BEST (include/dflow.h): the most inliers, ties to the earlier round, then to the smaller index; 0: no model yet
__device__ __forceinline__ static unsigned long long fit_key(uint32_t count, int round, int j)
{
    return ((unsigned long long)count << 32) | (0xFFFFFFFFu - (uint32_t)(round * 65536 + j));
}
__device__ __forceinline__ static int fit_key_round(unsigned long long key) { return (int)((0xFFFFFFFFu - (uint32_t)key) >> 16); }
__device__ __forceinline__ static int fit_key_index(unsigned long long key) { return (int)((0xFFFFFFFFu - (uint32_t)key) & 0xFFFFu); }
__device__ __forceinline__ static uint32_t fit_key_count(unsigned long long key) { return (uint32_t)(key >> 32); }

// hypothesis j < n of this round after its scoring: a degenerate one gets the count 0 (true), any other offers its key
__device__ __forceinline__ static bool fit_offer(const MfArgs &a, int j, int n, int round)
{
    if (j >= n) return false;
    const int32_t c = a.hyp_counts[j];
    if (c < 0) { a.hyp_counts[j] = 0; return true; }
    atomicMax(&a.state[FIT_S_BEST], fit_key((uint32_t)c, round, j));
    return false;
}

// the best key is this round's: its model becomes the current one (true)
__device__ __forceinline__ static bool fit_adopt(const MfArgs &a, unsigned long long key, int round)
{
    if (fit_key_round(key) != round) return false;
    for (int k = 0; k < 9; k++) a.cur[k] = a.models[(size_t)fit_key_index(key) * 9 + k];
    return true;
}

// counts[0..5]: scored, final inliers, degenerate, the winner's round, index (-1: none) and count
__device__ __forceinline__ static void fit_counts(const MfArgs &a, int32_t *__restrict__ counts, int scored, int final, int degen)
{
    const unsigned long long key = a.state[FIT_S_BEST];
    counts[0] = (int32_t)a.state[scored];
    counts[1] = (int32_t)a.state[final];
    counts[2] = (int32_t)a.state[degen];
    counts[3] = key ? fit_key_round(key) : -1;
    counts[4] = key ? fit_key_index(key) : -1;
    counts[5] = (int32_t)fit_key_count(key);
}

// CLASS (include/dflow.h), and whether the pixel (x, y) is one of the scored
__device__ __forceinline__ static uint8_t fit_class(bool good, bool excluded, bool in)
{
    return (uint8_t)(!good ? 0 : excluded ? 3 : in ? 1 : 2);
}
__device__ __forceinline__ static bool fit_scored(const MfArgs &a, bool good, bool excluded, int x, int y)
{
    return good && !excluded && y % a.step == 0 && x % a.step == 0;
}

// E (include/dflow.h): the affine model from the twelve sums n, a, b, aa, ab, bb, p, ap, bp, q, aq, bq over a = 2x - (w-1),
// b = 2y - (h-1) and the right-hand sides p, q in 1/64; false: a singular system or a coefficient that is not finite
__device__ static inline bool fit_affine_from_sums(const double (&S)[FIT_NSUMS], int w, int h, float (&m)[6])
{
    const double n = S[0], sa = S[1], sb = S[2], saa = S[3], sab = S[4], sbb = S[5];
    const double c00 = sbb * n - sb * sb, c01 = sb * sa - sab * n, c02 = sab * sb - sbb * sa;
    const double c11 = saa * n - sa * sa, c12 = sa * sab - saa * sb, c22 = saa * sbb - sab * sab;
    const double det = (saa * c00 + sab * c01) + sa * c02;
    if (det == 0.0 || !isfinite(det)) return false;
    bool ok = true;
    for (int row = 0; row < 2; row++) {
        const double r2 = S[6 + 3 * row], r0 = S[7 + 3 * row], r1 = S[8 + 3 * row];      // sum p, sum a p, sum b p
        const double x0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det, x1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double x2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        // p / 64 = x0 (2x - (w-1)) + x1 (2y - (h-1)) + x2
        const float m0 = (float)(x0 * 0.03125), m1 = (float)(x1 * 0.03125);
        const float m2 = (float)(((x2 - x0 * (double)(w - 1)) - x1 * (double)(h - 1)) * 0.015625);
        ok &= isfinite(m0) && isfinite(m1) && isfinite(m2);
        m[3 * row] = m0; m[3 * row + 1] = m1; m[3 * row + 2] = m2;
    }
    return ok;
}
