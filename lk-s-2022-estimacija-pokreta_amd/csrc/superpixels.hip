// Superpixels and per-segment affine flow models (include/dflow.h: dflow_superpixels, dflow_segment_fit; DESIGN.md "Superpixels"):
// an integer variant of gSLIC whose segments are 4-connected and compactly numbered, and a trimmed least-squares affine model of
// the flow per segment of any label plane.  This build's definitions; the reference has no counterpart.
//
// dflow_superpixels, 8 + 2 iters launches whatever the image holds, and no workgroup waits for another:
//   sp_init_kernel     a thread per centre: the grid centres at 1/16 resolution, the sums zeroed
//   sp_assign_kernel   the hot one, once per iteration.  One workgroup per SP_TW x SP_TH pixel tile; the centres of the cells the
//                      tile touches and their neighbours (at most SP_LCW x SP_LCH) staged in LDS once; a pixel's nine candidate
//                      keys (D' << 22 | k, 64-bit) from two 32-bit squared distances; the tile's partial sums in LDS by 32-bit
//                      integer atomics; one global integer atomic per (tile, centre, field) that is non-zero
//   sp_update_kernel   a thread per centre: the rounded 64-bit integer mean, the sums zeroed for the next iteration
//   sp_tile_kernel, sp_border_kernel, sp_root_kernel   the components of equal SLIC label: union_find.h's tile, border and root
//                      steps (uf_tile_step, uf_border_pair, uf_root_step) with "same label" as the join test
//   sp_merge_kernel    a lane per component root: the end of its chain of targets, the count of final roots per block
//                      (block_rank, plane_ops.h)
//   sp_scan_kernel     one block: the block counts become their exclusive prefix sums (block_scan_sums, plane_ops.h)
//   sp_number_kernel   final roots take their number (block_rank again), the others add their size to their final root's
//   sp_write_kernel    a lane per pixel: the final number, the raw label, the counts
// dflow_segment_fit, 2 rounds + 1 launches:
//   sf_acc_kernel      a lane per pixel, a wave per 8 x 8 square: the twelve int64 sums of its segment, a wave's adds aggregated
//                      per distinct label first (wave_each_key, plane_ops.h; a shuffle tree per sum), then 64-bit integer atomics
//   sf_solve_kernel    a thread per segment: the two 3x3 normal systems in float64 (step E of the motion fit, fit_common.h's
//                      fit_affine_from_sums, with the flow as the right-hand side), or the translation, or nothing
//   sf_apply_kernel    a lane per pixel: the model's flow, the class, the counts
// Every count and sum is an integer (exact in any order of arrival); every float32 and float64 chain is one IEEE operation per
// written operation (-ffp-contract=off).
#include "fit_common.h"
#include "union_find.h"
#include "wave_ops.h"

#define SP_TW 32
#define SP_TH 8
#define SP_THREADS (SP_TW * SP_TH)
#define SP_WAVES (SP_THREADS / 64)
#define SP_MIN_STEP 4
// SP_TW pixels in a row touch at most (SP_TW - 1) / S + 2 cells, and one more on either side is reachable
#define SP_LCW ((SP_TW - 1) / SP_MIN_STEP + 4)
#define SP_LCH ((SP_TH - 1) / SP_MIN_STEP + 4)
#define SP_NLC (SP_LCW * SP_LCH)
#define SP_FIELDS 6                                   // n, sum x, sum y, sum b, sum g, sum r
#define SP_ROW 8                                      // int32 per centre in d_centers and d_sums
#define SP_KEY_BITS 22
#define SP_COUNTS 8

struct SpGrid { int h, w, S, gw, gh, K; };

__global__ void __launch_bounds__(SP_THREADS) sp_init_kernel(SpGrid g, const uint8_t *__restrict__ bgr, int32_t *__restrict__ centers,
                                                             uint32_t *__restrict__ sums, int32_t *__restrict__ counts)
{
    const int k = blockIdx.x * SP_THREADS + threadIdx.x;
    if (k >= g.K) return;
    const int gy = k / g.gw, gx = k - gy * g.gw;
    const int x = min(gx * g.S + g.S / 2, g.w - 1), y = min(gy * g.S + g.S / 2, g.h - 1);
    const uint8_t *p = bgr + ((size_t)y * g.w + x) * 3;
    int32_t *c = centers + (size_t)k * SP_ROW;
    c[0] = 16 * x; c[1] = 16 * y; c[2] = 16 * p[0]; c[3] = 16 * p[1]; c[4] = 16 * p[2]; c[5] = 0; c[6] = 0; c[7] = 0;
#pragma unroll
    for (int f = 0; f < SP_ROW; f++) sums[(size_t)k * SP_ROW + f] = 0u;
    if (k == 0 && counts) counts[0] = g.K;
}

// label: NULL but in the last iteration
__global__ void __launch_bounds__(SP_THREADS) sp_assign_kernel(SpGrid g, uint32_t S2, uint32_t m2, const uint8_t *__restrict__ bgr,
                                                               const int32_t *__restrict__ centers, uint32_t *__restrict__ sums,
                                                               int32_t *__restrict__ label)
{
    __shared__ int s_c[SP_NLC][5];                    // cx16, cy16, b16, g16, r16
    __shared__ int s_k[SP_NLC];                       // the centre's k, -1: no such cell
    __shared__ unsigned s_sum[SP_NLC * SP_FIELDS];
    const int t = threadIdx.x, x0 = blockIdx.x * SP_TW, y0 = blockIdx.y * SP_TH;
    const int lcx0 = x0 / g.S - 1, lcy0 = y0 / g.S - 1;               // the cell of local centre (0, 0); may be -1
    for (int j = t; j < SP_NLC * SP_FIELDS; j += SP_THREADS) s_sum[j] = 0u;
    if (t < SP_NLC) {
        const int cy = lcy0 + t / SP_LCW, cx = lcx0 + t % SP_LCW;
        int k = -1;
        if (cy >= 0 && cy < g.gh && cx >= 0 && cx < g.gw) {
            k = cy * g.gw + cx;
            const int32_t *c = centers + (size_t)k * SP_ROW;
#pragma unroll
            for (int f = 0; f < 5; f++) s_c[t][f] = c[f];
        }
        s_k[t] = k;
    }
    __syncthreads();
    const int x = x0 + t % SP_TW, y = y0 + t / SP_TW;
    if (x < g.w && y < g.h) {
        const uint8_t *p = bgr + ((size_t)y * g.w + x) * 3;
        const int pb = p[0], pg = p[1], pr = p[2];
        const int b16 = 16 * pb, g16 = 16 * pg, r16 = 16 * pr, x16 = 16 * x, y16 = 16 * y;
        // the pixel's own cell is local (1..SP_LCH-2, 1..SP_LCW-2): its eight neighbours are inside the staged block
        const int lc = (y / g.S - lcy0) * SP_LCW + (x / g.S - lcx0);
        unsigned long long best = ~0ull;
        int bl = lc;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                const int l = lc + dy * SP_LCW + dx, k = s_k[l];
                if (k < 0) continue;
                // every difference is below 4*S*16 <= 2^12 in magnitude (colours: 2^12 as well): the squares' sums fit 32 bits
                const uint32_t d0 = (uint32_t)(b16 - s_c[l][2]), d1 = (uint32_t)(g16 - s_c[l][3]), d2 = (uint32_t)(r16 - s_c[l][4]);
                const uint32_t e0 = (uint32_t)(x16 - s_c[l][0]), e1 = (uint32_t)(y16 - s_c[l][1]);
                const uint32_t dc2 = d0 * d0 + d1 * d1 + d2 * d2, ds2 = e0 * e0 + e1 * e1;
                const unsigned long long D = (unsigned long long)S2 * dc2 + (unsigned long long)m2 * ds2;      // < 2^42
                const unsigned long long key = (D << SP_KEY_BITS) | (unsigned long long)(uint32_t)k;
                if (key < best) { best = key; bl = l; }
            }
        if (label) label[(size_t)y * g.w + x] = (int32_t)(best & ((1u << SP_KEY_BITS) - 1u));
        unsigned *q = s_sum + bl * SP_FIELDS;
        atomicAdd(q + 0, 1u); atomicAdd(q + 1, (unsigned)x); atomicAdd(q + 2, (unsigned)y);
        atomicAdd(q + 3, (unsigned)pb); atomicAdd(q + 4, (unsigned)pg); atomicAdd(q + 5, (unsigned)pr);
    }
    __syncthreads();
    for (int j = t; j < SP_NLC * SP_FIELDS; j += SP_THREADS) {
        const unsigned v = s_sum[j];
        if (v) atomicAdd(&sums[(size_t)s_k[j / SP_FIELDS] * SP_ROW + j % SP_FIELDS], v);          // v != 0: the centre exists
    }
}

// counts: NULL but in the last iteration
__global__ void __launch_bounds__(SP_THREADS) sp_update_kernel(SpGrid g, int32_t *__restrict__ centers, uint32_t *__restrict__ sums,
                                                               int32_t *counts)
{
    const int k = blockIdx.x * SP_THREADS + threadIdx.x;
    bool empty = false;
    if (k < g.K) {
        uint32_t *s = sums + (size_t)k * SP_ROW;
        int32_t *c = centers + (size_t)k * SP_ROW;
        const uint32_t n = s[0];
        if (n) {
#pragma unroll
            for (int f = 0; f < 5; f++) c[f] = (int32_t)((16ull * (unsigned long long)s[1 + f] + (unsigned long long)(n >> 1)) / n);
        }
        c[5] = (int32_t)n;
#pragma unroll
        for (int f = 0; f < SP_FIELDS; f++) s[f] = 0u;
        empty = n == 0u;
    }
    const bool is[1] = {empty};
    block_count<1>(is, counts, 1);
}

// ---- the 4-connected components of equal SLIC label (union_find.h's tile, border and root steps): every pixel of the frame is a
// member, and a SLIC label is >= 0, so no member's equals the -1 beyond the frame
__global__ void __launch_bounds__(SP_THREADS) sp_tile_kernel(int h, int w, const int32_t *__restrict__ slic, int *__restrict__ comp,
                                                             int *__restrict__ size)
{
    __shared__ int s_val[SP_THREADS];                 // the SLIC label, -1 (no label) beyond the frame
    const int t = threadIdx.x, x = blockIdx.x * SP_TW + t % SP_TW, y = blockIdx.y * SP_TH + t / SP_TW;
    const bool inside = x < w && y < h;
    const int v = inside ? slic[(size_t)y * w + x] : -1;
    s_val[t] = v;
    uf_tile_step<SP_TW, SP_TH>(h, w, inside, [&](int, int o) { return s_val[o] == v; }, comp, size);
}

__global__ void __launch_bounds__(SP_THREADS) sp_border_kernel(int h, int w, const int32_t *__restrict__ slic, int *comp)
{
    int p, q;
    if (!uf_border_pair<SP_TW, SP_TH>(h, w, blockIdx.x * SP_THREADS + threadIdx.x, p, q)) return;
    if (slic[p] == slic[q]) uf_union<__HIP_MEMORY_SCOPE_AGENT, UF_HANG>(comp, p, q);
}

__global__ void __launch_bounds__(SP_THREADS) sp_root_kernel(int n, int *comp, int *size) { uf_root_step<SP_THREADS>(n, comp, size); }

// The end of a root's chain of targets (fin[root]); comp and size are read only.  A step goes to the root of the pixel to the
// left of the root pixel, or above it in column 0: a smaller index, so the walk ends, at pixel 0 at the latest.
__global__ void __launch_bounds__(SP_THREADS) sp_merge_kernel(int n, int w, int min_size, const int *__restrict__ comp,
                                                              const int *__restrict__ size, int *__restrict__ fin,
                                                              int32_t *__restrict__ block_sums, int32_t *counts)
{
    __shared__ int s_fin[SP_WAVES];
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    bool root = false, small = false, final_root = false;
    if (i < n && comp[i] == i) {
        root = true;
        small = size[i] < min_size;
        int r = i;
        while (r != 0 && size[r] < min_size) r = comp[r % w ? r - 1 : r - w];
        fin[i] = r;
        final_root = r == i;
    }
    block_rank(final_root, s_fin);
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < SP_WAVES; k++) sum += s_fin[k];
        block_sums[blockIdx.x] = sum;
    }
    const bool is[2] = {root, small};
    block_count<2>(is, counts, 2);
}

// One block: the block sums become their exclusive prefix sums (block_scan_sums, plane_ops.h); block_sums[nb] and counts[5] = the
// total, n_seg.
__global__ void __launch_bounds__(SP_THREADS) sp_scan_kernel(int nb, int32_t *__restrict__ block_sums, int32_t *counts)
{
    const int total = block_scan_sums<SP_WAVES>(nb, block_sums);
    if (threadIdx.x == 0) {
        block_sums[nb] = total;
        if (counts) counts[5] = total;
    }
}

// A final root takes its number, stored as -1 - number in its own fin (no other lane reads it here); another root adds its size
// to its final root's (nobody reads a final root's size here).
__global__ void __launch_bounds__(SP_THREADS) sp_number_kernel(int n, const int *__restrict__ comp, int *size, int *fin,
                                                               const int32_t *__restrict__ block_sums)
{
    __shared__ int s_fin[SP_WAVES];
    const int i = blockIdx.x * SP_THREADS + threadIdx.x, wave = threadIdx.x >> 6;
    bool final_root = false;
    if (i < n && comp[i] == i) {
        const int f = fin[i];
        final_root = f == i;
        if (!final_root) atomicAdd(&size[f], size[i]);
    }
    const int rank = block_rank(final_root, s_fin);
    __syncthreads();
    if (final_root) {
        int number = block_sums[blockIdx.x] + rank;
        for (int k = 0; k < wave; k++) number += s_fin[k];
        fin[i] = -1 - number;
    }
}

__global__ void __launch_bounds__(SP_THREADS) sp_write_kernel(int n, const int *__restrict__ comp, const int *__restrict__ size,
                                                              const int *__restrict__ fin, int32_t *label, int32_t *__restrict__ slic,
                                                              int32_t *counts)
{
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    bool changed = false;
    int largest = 0;
    if (i < n) {
        const int r = comp[i];
        int v = fin[r];
        changed = v >= 0;                             // the root is not final: its final root holds the number
        if (changed) v = fin[v];
        if (slic) slic[i] = label[i];                 // the raw label, which d_label has held so far: a lane's own pixel
        label[i] = -1 - v;
        if (r == i && !changed) largest = size[i];
    }
    if (counts) {                                     // uniform
        largest = block_reduce<SP_WAVES>(largest, [](int &x, const int &y) { x = max(x, y); });
        if (threadIdx.x == 0 && largest) atomicMax(&counts[6], largest);
    }
    const bool is[1] = {changed};
    block_count<1>(is, counts, 4);
}

int launch_superpixels(int H, int W, const uint8_t *bgr, int step, int compactness, int iters, int min_size, int32_t *label,
                       int32_t *centers, int32_t *slic, int32_t *counts, int32_t *sums, int32_t *comp, int32_t *size, int32_t *fin,
                       int32_t *scan, hipStream_t s)
{
    SpGrid g;
    g.h = H; g.w = W; g.S = step; g.gw = (W + step - 1) / step; g.gh = (H + step - 1) / step; g.K = g.gw * g.gh;
    static_assert(8192 / SP_MIN_STEP * (8192 / SP_MIN_STEP) <= 1 << SP_KEY_BITS, "K fits the key's low bits");
    // D' < 64^2 * 3 * 4080^2 + 255^2 * 2 * (4 * 64 * 16)^2 < 2^38 + 2^41 < 2^(64 - SP_KEY_BITS)
    static_assert(4096ull * 3 * 4080 * 4080 + 65025ull * 2 * 4096 * 4096 < 1ull << (64 - SP_KEY_BITS), "the key fits 64 bits");
    const int n = H * W, ntx = (W + SP_TW - 1) / SP_TW, nty = (H + SP_TH - 1) / SP_TH;
    const int nb = (n + SP_THREADS - 1) / SP_THREADS, kb = (g.K + SP_THREADS - 1) / SP_THREADS;
    uint32_t *usums = reinterpret_cast<uint32_t *>(sums);
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, SP_COUNTS * sizeof(int32_t), s));
    hipLaunchKernelGGL(sp_init_kernel, dim3(kb), dim3(SP_THREADS), 0, s, g, bgr, centers, usums, counts);
    for (int it = 0; it < iters; it++) {
        const bool last = it == iters - 1;
        hipLaunchKernelGGL(sp_assign_kernel, dim3(ntx, nty), dim3(SP_THREADS), 0, s, g, (uint32_t)(step * step),
                           (uint32_t)(compactness * compactness), bgr, (const int32_t *)centers, usums, last ? label : nullptr);
        hipLaunchKernelGGL(sp_update_kernel, dim3(kb), dim3(SP_THREADS), 0, s, g, centers, usums, last ? counts : nullptr);
    }
    hipLaunchKernelGGL(sp_tile_kernel, dim3(ntx, nty), dim3(SP_THREADS), 0, s, H, W, (const int32_t *)label, comp, size);
    hipLaunchKernelGGL(sp_border_kernel, dim3(uf_border_blocks<SP_TW, SP_TH>(H, W)), dim3(SP_THREADS), 0, s, H, W, (const int32_t *)label,
                       comp);
    hipLaunchKernelGGL(sp_root_kernel, dim3(nb), dim3(SP_THREADS), 0, s, n, comp, size);
    hipLaunchKernelGGL(sp_merge_kernel, dim3(nb), dim3(SP_THREADS), 0, s, n, W, min_size, (const int *)comp, (const int *)size, fin, scan,
                       counts);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(SP_THREADS), 0, s, nb, scan, counts);
    hipLaunchKernelGGL(sp_number_kernel, dim3(nb), dim3(SP_THREADS), 0, s, n, (const int *)comp, size, fin, (const int32_t *)scan);
    hipLaunchKernelGGL(sp_write_kernel, dim3(nb), dim3(SP_THREADS), 0, s, n, (const int *)comp, (const int *)size, (const int *)fin, label,
                       slic, counts);
    return dflow_check_launch("superpixel kernels");
}

// ---------------------------------------------------------------------------------------------- the per-segment fit
#define SF_COUNTS 8

struct SfArgs {
    int h, w, layout, n_seg, n;
    float thresh;
    const float *flow;
    const int32_t *label;
    float *models;                                    // (n_seg, 6)
    int32_t *seg_counts;                              // (n_seg, 4): pixels, participants, agreeing, kind
    unsigned long long *acc;                          // (n_seg, 12)
};

__device__ __forceinline__ static void sf_model_flow(const float *__restrict__ m, float xf, float yf, float &Um, float &Vm)
{
    Um = (m[0] * xf + m[1] * yf) + m[2];
    Vm = (m[3] * xf + m[4] * yf) + m[5];
}

// AGREES at T (include/dflow.h); a NaN anywhere makes it false
__device__ __forceinline__ static bool sf_agrees(float Um, float Vm, float U, float V, float T)
{
    const float eu = U - Um, ev = V - Vm;
    return eu * eu + ev * ev <= T * T;
}

__device__ __forceinline__ static bool sf_in_range(float U, float V) { return fabsf(U) <= FIT_RANGE && fabsf(V) <= FIT_RANGE; }

// round 0: every participant, and the pixels per label; round r > 0: the participants that agree with the model so far at T
__global__ void __launch_bounds__(SP_THREADS) sf_acc_kernel(SfArgs a, int round, float T)
{
    // a wave is an 8 x 8 square of the block's SP_TW x SP_TH tile: segments are compact, so a square meets fewer of them than a row
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * SP_TW + (int)(threadIdx.x >> 6) * 8 + (lane & 7), y = blockIdx.y * SP_TH + (lane >> 3);
    int l = -1;
    bool part = false;
    long long v[FIT_NSUMS - 1];
#pragma unroll
    for (int k = 0; k < FIT_NSUMS - 1; k++) v[k] = 0;
    if (x < a.w && y < a.h) {
        const int i = y * a.w + x;
        const int lab = a.label[i];
        if (lab >= 0 && lab < a.n_seg) {
            l = lab;
            float U = 0.0f, V = 0.0f;
            part = flow_good(a.flow, a.layout, (size_t)i, U, V) && sf_in_range(U, V);
            if (part && round > 0) {
                part = a.seg_counts[(size_t)l * 4 + 3] != 0;
                if (part) {
                    float Um, Vm;
                    sf_model_flow(a.models + (size_t)l * 6, (float)x, (float)y, Um, Vm);
                    part = sf_agrees(Um, Vm, U, V, T);
                }
            }
            if (part) {
                const long long ca = 2 * x - (a.w - 1), cb = 2 * y - (a.h - 1), p = llrintf(U * 64.0f), q = llrintf(V * 64.0f);
                v[0] = ca; v[1] = cb; v[2] = ca * ca; v[3] = ca * cb; v[4] = cb * cb;
                v[5] = p; v[6] = ca * p; v[7] = cb * p; v[8] = q; v[9] = ca * q; v[10] = cb * q;
            }
        }
    }
    // one add per wave, distinct label and sum
    wave_each_key(round == 0 ? l >= 0 : part, l, [&](int r, bool mine, bool is_leader) {
        const int c_all = wave_count(mine), c_part = wave_count(mine && part);
        if (c_part) {                                 // uniform
            unsigned long long *acc = a.acc + (size_t)r * FIT_NSUMS;
            if (is_leader) atomicAdd(&acc[0], (unsigned long long)c_part);
#pragma unroll
            for (int k = 0; k < FIT_NSUMS - 1; k++) {
                const long long sum = wave_reduce_all(mine && part ? v[k] : 0ll, [](long long &a, long long b) { a += b; });
                if (is_leader && sum) atomicAdd(&acc[1 + k], (unsigned long long)sum);
            }
        }
        if (round == 0 && is_leader) atomicAdd(&a.seg_counts[(size_t)r * 4], c_all);
    });
}

// counts: NULL but in the last round
__global__ void __launch_bounds__(SP_THREADS) sf_solve_kernel(SfArgs a, int round, int32_t *counts)
{
    const int s = blockIdx.x * SP_THREADS + threadIdx.x;
    int kind = -1;
    if (s < a.n_seg) {
        unsigned long long *acc = a.acc + (size_t)s * FIT_NSUMS;
        const long long N = (long long)acc[0];
        double S[FIT_NSUMS];
#pragma unroll
        for (int k = 0; k < FIT_NSUMS; k++) { S[k] = (double)(long long)acc[k]; acc[k] = 0ull; }
        float *mo = a.models + (size_t)s * 6;
        int32_t *sc = a.seg_counts + (size_t)s * 4;
        if (round == 0) sc[1] = (int32_t)N;
        kind = round == 0 ? 0 : sc[3];
        float m[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        bool write = round == 0;
        if (N >= 1) {
            write = true;
            if (N >= 3 && fit_affine_from_sums(S, a.w, a.h, m)) kind = 2;
            else {
                m[0] = 0.0f; m[1] = 0.0f; m[2] = (float)((S[6] / S[0]) * 0.015625);
                m[3] = 0.0f; m[4] = 0.0f; m[5] = (float)((S[9] / S[0]) * 0.015625);
                kind = 1;
            }
        }
        if (write) {
#pragma unroll
            for (int k = 0; k < 6; k++) mo[k] = m[k];
            sc[3] = kind;
        }
    }
    const bool is[3] = {kind > 0, kind == 2, kind == 1};
    block_count<3>(is, counts, 2);
}

__global__ void __launch_bounds__(SP_THREADS) sf_apply_kernel(SfArgs a, float *__restrict__ out, uint8_t *__restrict__ cls,
                                                              int32_t *counts)
{
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    int l = -1;
    bool part = false, agree = false, bad_label = false, bad_range = false;
    if (i < a.n) {
        const int lab = a.label[i];
        const bool in = lab >= 0 && lab < a.n_seg;
        bad_label = !in;
        const int y = i / a.w, x = i - y * a.w;
        float U = 0.0f, V = 0.0f;
        const bool good = flow_good(a.flow, a.layout, (size_t)i, U, V), ranged = good && sf_in_range(U, V);
        bad_range = good && !ranged;
        part = in && ranged;
        const int kind = in ? a.seg_counts[(size_t)lab * 4 + 3] : 0;
        FlowOut o = {0.0f, 0.0f, 0.0f};
        if (kind) {
            l = lab;
            sf_model_flow(a.models + (size_t)lab * 6, (float)x, (float)y, o.u, o.v);
            o.valid = 1.0f;
            agree = part && sf_agrees(o.u, o.v, U, V, a.thresh);
        }
        if (out) reinterpret_cast<FlowOut *>(out)[i] = o;
        if (cls) cls[i] = (uint8_t)(!part ? 0 : !kind ? 3 : agree ? 1 : 2);
    }
    wave_add_by_key(agree, l * 4 + 2, a.seg_counts, 1);              // l < 2^26
    const bool is0[2] = {part, agree}, is5[2] = {bad_label, bad_range};
    block_count<2>(is0, counts, 0);
    block_count<2>(is5, counts, 5);
}

int launch_segment_fit(int H, int W, const float *flow, int layout, const int32_t *label, int n_seg, float thresh, int rounds,
                       float *models, int32_t *seg_counts, float *out, uint8_t *cls, int32_t *counts, int64_t *acc, hipStream_t s)
{
    SfArgs a;
    a.h = H; a.w = W; a.layout = layout; a.n_seg = n_seg; a.n = H * W; a.thresh = thresh;
    a.flow = flow; a.label = label; a.models = models; a.seg_counts = seg_counts; a.acc = reinterpret_cast<unsigned long long *>(acc);
    DFLOW_HIP(hipMemsetAsync(acc, 0, (size_t)n_seg * FIT_NSUMS * sizeof(int64_t), s));
    DFLOW_HIP(hipMemsetAsync(seg_counts, 0, (size_t)n_seg * 4 * sizeof(int32_t), s));
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, SF_COUNTS * sizeof(int32_t), s));
    const int nb = (a.n + SP_THREADS - 1) / SP_THREADS, sb = (n_seg + SP_THREADS - 1) / SP_THREADS;
    for (int r = 0; r < rounds; r++) {
        const float T = thresh * (float)(1 << (rounds - 1 - r));      // one multiplication by an exact power of two
        hipLaunchKernelGGL(sf_acc_kernel, dim3((W + SP_TW - 1) / SP_TW, (H + SP_TH - 1) / SP_TH), dim3(SP_THREADS), 0, s, a, r, T);
        hipLaunchKernelGGL(sf_solve_kernel, dim3(sb), dim3(SP_THREADS), 0, s, a, r, r == rounds - 1 ? counts : nullptr);
    }
    hipLaunchKernelGGL(sf_apply_kernel, dim3(nb), dim3(SP_THREADS), 0, s, a, out, cls, counts);
    return dflow_check_launch("segment fit kernels");
}
