// Leaf device helpers of the image-plane stages (flow_eval.hip, flow_picture.hip, bcd_stats.hip, pyramid.hip, consistency.hip,
// segments.hip, prior.hip, frame_interp.hip, flow_wmedian.hip, label_conf.hip, tracks.hip, superpixels.hip and, through fit_common.h,
// the fits; union_find.h's root step): a block's reduction and class counts, a wave's lanes grouped by key, the rank of a block's
// flagged threads, the one-block scan of block sums, the four-pixel access to a flow plane and a (b, g, r) picture, and the bilinear
// sample of a picture with its photometric error.  They load, pack, sample, reduce, rank or count; every kernel keeps its own
// loop, launch function and workspace.  What else happens inside one wave (the scan, the count and rank of a
// ballot, the exchanges and the minimum of a 16-lane DPP row that prior.hip and label_conf.hip use) is wave_ops.h's, included here.
#pragma once
#include "dflow_common.h"
#include "jet_lut.h"
#include "wave_ops.h"

// ---- block reduce: the block's total of `a` in thread 0 (the other threads hold partial results).  A shuffle tree per wave
// (64 lanes: offsets 32 .. 1), then lane 0 of every wave through LDS and thread 0 merges waves 1 .. WAVES - 1 in that order:
// the order of every merge is fixed, so a double sum keeps its bits from call to call.  T travels dword by dword.  The tree stays
// written out here, not a function of wave_ops.h: through a call mf_sums_kernel (motion_fit.hip) gets other device code
// ("Wave primitives").
template <int WAVES, typename T, typename Merge> __device__ static T block_reduce(T a, Merge merge)
{
    static_assert(sizeof(T) % 4 == 0, "block_reduce shuffles whole dwords");
    __shared__ T wave_part[WAVES];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        uint32_t d[sizeof(T) / 4];
        __builtin_memcpy(d, &a, sizeof(T));
#pragma unroll
        for (unsigned k = 0; k < sizeof(T) / 4; k++) d[k] = __shfl_down(d[k], off, 64);
        T b;
        __builtin_memcpy(&b, d, sizeof(T));
        merge(a, b);
    }
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < WAVES; k++) merge(a, wave_part[k]);
    }
    return a;
}

// ---- block class counts: how many lanes of the block have is[k], added to counts[offset + k]: ballots -> per-block LDS
// counters -> one integer atomic per block and non-zero counter.  Every thread of the block calls it; counts may be NULL
// (uniform: nothing is counted).  The second form counts the lanes whose class is k (a lane of no class passes -1).
template <int N> __device__ static inline void block_count(const bool (&is)[N], int32_t *counts, int offset)
{
    __shared__ int s_cnt[N];
    if (!counts) return;
    if (threadIdx.x < N) s_cnt[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int c = wave_count(is[k]);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt[k], c);
    }
    __syncthreads();
    if (threadIdx.x < N && s_cnt[threadIdx.x]) atomicAdd(&counts[offset + threadIdx.x], s_cnt[threadIdx.x]);
}

template <int N> __device__ static inline void block_count_class(int kind, int32_t *counts, int offset)
{
    bool is[N];
#pragma unroll
    for (int k = 0; k < N; k++) is[k] = kind == k;
    block_count<N>(is, counts, offset);
}

// ---- a wave's lanes grouped by key (union_find.h's root step; superpixels.hip: sf_acc_kernel, sf_apply_kernel): one round per
// distinct key among the lanes that have `pending`, in the order of each key's first lane.  f(key, mine, is_leader) is called by
// every lane of the wave in every round (it may ballot and shuffle): `mine` for the lanes that hold the round's key, `is_leader`
// for the first of them.  Terminates: a round retires the first pending lane and every lane that shares its key, so there are at
// most 64 rounds.  The loop's trip count depends on other lanes: every lane of the wave must arrive here.
template <typename F> __device__ static inline void wave_each_key(bool pending, int key, F f)
{
    const int lane = threadIdx.x & 63;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int r = __shfl(key, leader);
        const bool mine = pending && key == r;
        f(r, mine, lane == leader);
        if (mine) pending = false;
    }
}

// `c` added to slot[key] once per wave and distinct key among the lanes that have `on`
__device__ static inline void wave_add_by_key(bool on, int key, int *slot, int c)
{
    wave_each_key(on, key, [&](int r, bool mine, bool is_leader) {
        const int cnt = wave_count(mine);
        if (is_leader) atomicAdd(&slot[r], cnt * c);
    });
}

// ---- the flagged threads of a block in thread order (superpixels.hip: sp_merge_kernel, sp_number_kernel; tracks.hip:
// seed_block_flags): the number of flagged lanes below the caller's in its wave, and s_wave[wave] = the wave's count.  No barrier
// here: s_wave (one int per wave) is the caller's, valid after the caller's next __syncthreads, so that several rounds share one.
__device__ static inline int block_rank(bool flag, int *s_wave)
{
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(b);
    return (int)lane_rank(b);
}

// ---- one block of WAVES waves: sums[0 .. nb) become their exclusive prefix sums (a contiguous chunk per thread, the chunks'
// totals scanned through the waves); the total is returned in every thread (superpixels.hip: sp_scan_kernel; tracks.hip:
// track_seed_scan_kernel).  Every thread of the block calls it.
template <int WAVES> __device__ static inline int block_scan_sums(int nb, int32_t *__restrict__ sums)
{
    __shared__ int s_part[WAVES];
    const int chunk = (nb + WAVES * 64 - 1) / (WAVES * 64), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lo = min((int)threadIdx.x * chunk, nb), hi = min(lo + chunk, nb);
    int sum = 0;
    for (int j = lo; j < hi; j++) sum += sums[j];
    const int incl = (int)wave_scan_add((uint32_t)sum);
    if (lane == 63) s_part[wave] = incl;
    __syncthreads();
    int before = incl - sum, total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; k++) {
        if (k < wave) before += s_part[k];
        total += s_part[k];
    }
    for (int j = lo; j < hi; j++) {
        const int v = sums[j];
        sums[j] = before;
        before += v;
    }
    return total;
}

// ---- a plane as a flat array of h*w pixels, four pixels per lane and step, grid-stride over at most PLANE_MAX_BLOCKS blocks
#define PLANE_THREADS 256
#define PLANE_MAX_BLOCKS 1024         // 4 blocks of 256 threads on each of the 256 CUs

static int plane_blocks(int H, int W)
{
    const size_t ngroups = ((size_t)H * W + 3) / 4;
    const size_t b = (ngroups + PLANE_THREADS - 1) / PLANE_THREADS;
    return (int)(b < PLANE_MAX_BLOCKS ? b : PLANE_MAX_BLOCKS);
}

// the four pixels of group g of a flow plane as U, V, valid: three (DYDX: two) 16-byte loads
template <int LAYOUT>
__device__ __forceinline__ static void flow_load4(const float *__restrict__ flow, unsigned g, float (&U)[4], float (&V)[4], float (&valid)[4])
{
    if constexpr (LAYOUT == DFLOW_EVAL_UVV) {
        const float4 *tp = reinterpret_cast<const float4 *>(flow) + (size_t)g * 3;
        const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
        const float T[12] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w};
#pragma unroll
        for (int k = 0; k < 4; k++) { U[k] = T[3 * k]; V[k] = T[3 * k + 1]; valid[k] = T[3 * k + 2]; }
    } else {
        const float4 *tp = reinterpret_cast<const float4 *>(flow) + (size_t)g * 2;
        const float4 t0 = tp[0], t1 = tp[1];
        const float T[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};           // [dy,dx]: U = dx, V = dy
#pragma unroll
        for (int k = 0; k < 4; k++) { U[k] = T[2 * k + 1]; V[k] = T[2 * k]; valid[k] = 1.0f; }
    }
}

// the one pixel p of the tail (the 1..3 pixels after the last whole group)
template <int LAYOUT>
__device__ __forceinline__ static void flow_load1(const float *__restrict__ flow, unsigned p, float &U, float &V, float &valid)
{
    if constexpr (LAYOUT == DFLOW_EVAL_UVV) { U = flow[(size_t)p * 3]; V = flow[(size_t)p * 3 + 1]; valid = flow[(size_t)p * 3 + 2]; }
    else { U = flow[(size_t)p * 2 + 1]; V = flow[(size_t)p * 2]; valid = 1.0f; }
}

// four (b, g, r) pixels, 12 bytes, and a pixel as the entry b | g << 8 | r << 16
struct Bgr4 { uint32_t a, b, c; };

__device__ __forceinline__ static Bgr4 bgr_pack4(const uint32_t (&c)[4])
{
    Bgr4 v;
    v.a = c[0] | (c[1] << 24);
    v.b = (c[1] >> 8) | (c[2] << 16);
    v.c = (c[2] >> 16) | (c[3] << 8);
    return v;
}

// the inverse; bits 24..31 of an entry hold a neighbour's byte
__device__ __forceinline__ static void bgr_unpack4(const Bgr4 &q, uint32_t (&c)[4])
{
    c[0] = q.a; c[1] = (q.a >> 24) | (q.b << 8); c[2] = (q.b >> 16) | (q.c << 16); c[3] = q.c >> 8;
}

__device__ __forceinline__ static void bgr_store1(uint8_t *__restrict__ bgr, size_t p, uint32_t c)
{
    bgr[p * 3] = (uint8_t)c; bgr[p * 3 + 1] = (uint8_t)(c >> 8); bgr[p * 3 + 2] = (uint8_t)(c >> 16);
}

// ---- the bilinear sample of a (h,w,3) picture and the photometric error (include/dflow.h: dflow_warp_eval), float32, one IEEE
// operation per written operation: what flow_picture.hip's warp check and frame_interp.hip sample and compare with
// a position INSIDE the frame (a NaN is not)
__device__ __forceinline__ static bool bgr_inside(float xs, float ys, int w, int h)
{
    return xs >= 0.0f && xs <= (float)(w - 1) && ys >= 0.0f && ys <= (float)(h - 1);
}

// the three channels (b, g, r) of picture I at the inside position (xs, ys)
__device__ __forceinline__ static void bgr_bilinear(const uint8_t *__restrict__ I, int w, int h, float xs, float ys, float (&wv)[3])
{
    const float xf = floorf(xs), yf = floorf(ys);
    const float ax = xs - xf, ay = ys - yf;
    const int x0 = (int)xf, y0 = (int)yf, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const uint8_t *p00 = I + ((size_t)y0 * w + x0) * 3, *p01 = I + ((size_t)y0 * w + x1) * 3;
    const uint8_t *p10 = I + ((size_t)y1 * w + x0) * 3, *p11 = I + ((size_t)y1 * w + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float top = (1.0f - ax) * (float)p00[c] + ax * (float)p01[c];
        const float bot = (1.0f - ax) * (float)p10[c] + ax * (float)p11[c];
        wv[c] = (1.0f - ay) * top + ay * bot;
    }
}

// ((|a_b - b_b| + |a_g - b_g|) + |a_r - b_r|) / 3
__device__ __forceinline__ static float bgr_mean_abs_diff(const float (&a)[3], const float (&b)[3])
{
    return ((fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + fabsf(a[2] - b[2])) / 3.0f;
}

// the channels of the entry b | g << 8 | r << 16 as floats, and (int)floorf(v + 0.5f) per channel back into an entry
__device__ __forceinline__ static void bgr_entry_floats(uint32_t e, float (&v)[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = (float)((e >> (8 * c)) & 255u);
}

__device__ __forceinline__ static uint32_t bgr_round_entry(const float (&v)[3])
{
    uint32_t e = 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) e |= (uint32_t)(int)floorf(v[c] + 0.5f) << (8 * c);
    return e;
}

// the colour table of both error pictures (flow_eval.hip, flow_picture.hip)
static __constant__ uint32_t plane_jet_lut[256] = {JET_LUT_VALUES};
