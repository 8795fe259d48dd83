// Point trajectories through a frame sequence (include/dflow.h: dflow_track_advance, dflow_track_seed, dflow_track_flow; DESIGN.md
// "Point trajectories"): a set of tracks carried one frame forward along a forward flow and ended where the backward flow does not
// undo it (Sundaram, Brox, Keutzer), new tracks started in the cells no live track covers, and the displacement of the tracks that
// live in two snapshots as a sparse flow.  This build's definitions; the reference has no counterpart.
//
// One track (track_advance_kernel, track_mark_kernel, track_claim_kernel) or one cell / pixel per lane, 256 threads per block; a
// position is one 8-byte load, the corners of a bilinear sample through flow_good (dflow_common.h), the counts through block_count /
// block_count_class (plane_ops.h).  One IEEE float32 operation per written operation (-ffp-contract=off).  A lane touches only its
// own slot, so dflow_track_advance runs in place.  The seed's compaction is per-block counts (block_rank, plane_ops.h), one block
// that scans the block sums (block_scan_sums, plane_ops.h; superpixels.hip numbers its segments the same way) and an emit that
// repeats the block's own ranks: no workgroup waits for another.
#include <math.h>
#include "plane_ops.h"

#define TRK_THREADS 256
#define TRK_WAVES (TRK_THREADS / 64)
#define TRK_FREE 0
#define TRK_LIVE 1
#define TRK_LEFT 2
#define TRK_NOFLOW 3
#define TRK_NOBACK 4
#define TRK_INCONSISTENT 5
#define TRK_ADV_CLASSES 6                             // live after, left, noflow, noback, inconsistent, not live before

// The bilinear sample (U, V) of field f at the INSIDE position (x, y); false when a corner that is looked at is not good.
// 0 <= y0 <= h-1, and ay > 0 only below h-1 (x likewise): every corner that is read lies inside the frame.  A corner of weight
// zero is the corner beside it, which is read once.
__device__ static inline bool track_sample(const float *__restrict__ f, int layout, int w, float x, float y, float &U, float &V)
{
    const int y0 = (int)floorf(y), x0 = (int)floorf(x);
    const float ay = y - (float)y0, ax = x - (float)x0;
    const bool more_x = ax > 0.0f, more_y = ay > 0.0f;
    const size_t p00 = (size_t)y0 * w + x0, p10 = more_y ? p00 + w : p00;
    float u00, v00, u01, v01, u10, v10, u11, v11;
    bool good = flow_good(f, layout, p00, u00, v00);
    u01 = u00; v01 = v00;
    if (more_x) good = flow_good(f, layout, p00 + 1, u01, v01) && good;
    u10 = u00; v10 = v00; u11 = u01; v11 = v01;
    if (more_y) {
        good = flow_good(f, layout, p10, u10, v10) && good;
        u11 = u10; v11 = v10;
        if (more_x) good = flow_good(f, layout, p10 + 1, u11, v11) && good;
    }
    if (!good) return false;
    const float tu = u00 + ax * (u01 - u00), bu = u10 + ax * (u11 - u10);
    const float tv = v00 + ax * (v01 - v00), bv = v10 + ax * (v11 - v10);
    U = tu + ay * (bu - tu);
    V = tv + ay * (bv - tv);
    return true;
}

// pos_out / state_out may be pos_in / state_in: no __restrict__ on the four
__global__ void __launch_bounds__(TRK_THREADS) track_advance_kernel(int h, int w, const float *__restrict__ fwd, int layout_fwd,
                                                                    const float *__restrict__ bwd, int layout_bwd, int cap,
                                                                    const float2 *pos_in, const int32_t *state_in, float rel, float abs_tol,
                                                                    float2 *pos_out, int32_t *state_out, float *__restrict__ err,
                                                                    int32_t *counts)
{
    const int i = blockIdx.x * TRK_THREADS + threadIdx.x;
    int kind = -1;
    if (i < cap) {
        const float2 p = pos_in[i];
        const int st = state_in[i];
        float2 np = p;
        int ns = st;
        float e2 = -1.0f;
        kind = 5;
        if (st == TRK_LIVE) {
            float U, V, bu, bv;
            if (!bgr_inside(p.x, p.y, w, h)) ns = TRK_LEFT;
            else if (!track_sample(fwd, layout_fwd, w, p.x, p.y, U, V)) ns = TRK_NOFLOW;
            else {
                const float nx = p.x + U, ny = p.y + V;
                if (!bgr_inside(nx, ny, w, h)) ns = TRK_LEFT;
                else if (!bwd) { np.x = nx; np.y = ny; }
                else if (!track_sample(bwd, layout_bwd, w, nx, ny, bu, bv)) ns = TRK_NOBACK;
                else {
                    const float du = U + bu, dv = V + bv;
                    e2 = du * du + dv * dv;
                    const float m2 = (U * U + V * V) + (bu * bu + bv * bv);
                    if (e2 <= rel * m2 + abs_tol) { np.x = nx; np.y = ny; }
                    else ns = TRK_INCONSISTENT;                                         // a NaN is inconsistent
                }
            }
            kind = ns == TRK_LIVE ? 0 : ns - 1;
        }
        pos_out[i] = np;
        state_out[i] = ns;
        if (err) err[i] = e2;
    }
    block_count_class<TRK_ADV_CLASSES>(kind, counts, 0);
}

int launch_track_advance(int H, int W, const float *fwd, int layout_fwd, const float *bwd, int layout_bwd, int cap, const float *pos_in,
                         const int32_t *state_in, float rel, float abs_tol, float *pos_out, int32_t *state_out, float *err,
                         int32_t *counts, hipStream_t s)
{
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, TRK_ADV_CLASSES * sizeof(int32_t), s));
    hipLaunchKernelGGL(track_advance_kernel, dim3((cap + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, s, H, W, fwd, layout_fwd,
                       bwd, layout_bwd, cap, reinterpret_cast<const float2 *>(pos_in), state_in, rel, abs_tol,
                       reinterpret_cast<float2 *>(pos_out), state_out, err, counts);
    return dflow_check_launch("track_advance_kernel");
}

// ---- the seed: d_scan = the cells (gh*gw), the block sums (one per TRK_SEED_CELLS cells), the n the call started from
#define TRK_SEED_ROUNDS 4
#define TRK_SEED_CELLS (TRK_THREADS * TRK_SEED_ROUNDS)
#define TRK_SEED_COUNTS 4                             // covered cells, seedable cells, seeded, dropped

struct SeedGrid { int h, w, step, gw, ncells; };

__device__ static inline int seed_clamp_n(const int32_t *d_n, int cap) { return clampi(*d_n, 0, cap); }

// a LIVE track among the slots below n marks its cell; all writers of a cell store the same value
__global__ void __launch_bounds__(TRK_THREADS) track_mark_kernel(SeedGrid g, int cap, const float2 *__restrict__ pos,
                                                                 const int32_t *__restrict__ state, const int32_t *__restrict__ d_n,
                                                                 int32_t *__restrict__ cells)
{
    const int i = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (i >= seed_clamp_n(d_n, cap) || state[i] != TRK_LIVE) return;
    const float2 p = pos[i];
    if (!bgr_inside(p.x, p.y, g.w, g.h)) return;
    cells[((int)rintf(p.y) / g.step) * g.gw + (int)rintf(p.x) / g.step] = 1;
}

// the seed pixel of cell c
__device__ static inline void seed_pixel(const SeedGrid &g, int c, int &sx, int &sy)
{
    const int cy = c / g.gw, cx = c - cy * g.gw;
    sx = min(cx * g.step + g.step / 2, g.w - 1);
    sy = min(cy * g.step + g.step / 2, g.h - 1);
}

// cell c is SEEDABLE: not covered, and its seed pixel is in the mask
__device__ static inline bool seed_seedable(const SeedGrid &g, const int32_t *__restrict__ cells, const uint8_t *__restrict__ mask, int c,
                                            bool &covered)
{
    covered = c < g.ncells && cells[c] != 0;
    if (c >= g.ncells || covered) return false;
    if (!mask) return true;
    int sx, sy;
    seed_pixel(g, c, sx, sy);
    return mask[(size_t)sy * g.w + sx] != 0;
}

// The seedable cells of the block's TRK_SEED_CELLS cells in raster order, round k = cells base + k*256 .. +255: is[k] the lane's
// own, s_wave[k * TRK_WAVES + wave] the count of each wave of each round (valid after the __syncthreads at the end).
__device__ static inline void seed_block_flags(const SeedGrid &g, const int32_t *__restrict__ cells, const uint8_t *__restrict__ mask,
                                               int32_t *counts, bool (&is)[TRK_SEED_ROUNDS], int (&rank)[TRK_SEED_ROUNDS], int *s_wave)
{
    const int base = blockIdx.x * TRK_SEED_CELLS;
#pragma unroll
    for (int k = 0; k < TRK_SEED_ROUNDS; k++) {
        bool covered;
        is[k] = seed_seedable(g, cells, mask, base + k * TRK_THREADS + (int)threadIdx.x, covered);
        rank[k] = block_rank(is[k], s_wave + k * TRK_WAVES);
        block_count_class<1>(covered ? 0 : -1, counts, 0);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(TRK_THREADS) track_seed_count_kernel(SeedGrid g, const int32_t *__restrict__ cells,
                                                                       const uint8_t *__restrict__ mask, int32_t *__restrict__ block_sums,
                                                                       int32_t *counts)
{
    __shared__ int s_wave[TRK_SEED_ROUNDS * TRK_WAVES];
    bool is[TRK_SEED_ROUNDS];
    int rank[TRK_SEED_ROUNDS];
    seed_block_flags(g, cells, mask, counts, is, rank, s_wave);
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int j = 0; j < TRK_SEED_ROUNDS * TRK_WAVES; j++) sum += s_wave[j];
        block_sums[blockIdx.x] = sum;
    }
}

// One block: the block sums become their exclusive prefix sums (block_scan_sums, plane_ops.h), the n the call started from is kept
// for the emit, *d_n and the counts are set.
__global__ void __launch_bounds__(TRK_THREADS) track_seed_scan_kernel(int nb, int cap, int32_t *__restrict__ block_sums, int32_t *d_n,
                                                                      int32_t *counts)
{
    const int total = block_scan_sums<TRK_WAVES>(nb, block_sums);
    if (threadIdx.x == 0) {
        const int n = seed_clamp_n(d_n, cap), seeded = min(total, cap - n);
        block_sums[nb] = n;
        *d_n = n + seeded;
        if (counts) { counts[1] = total; counts[2] = seeded; counts[3] = total - seeded; }
    }
}

// the r-th seedable cell in raster order gets slot n + r, if that is below cap
__global__ void __launch_bounds__(TRK_THREADS) track_seed_emit_kernel(SeedGrid g, int nb, int cap, int frame, const int32_t *__restrict__ cells,
                                                                      const uint8_t *__restrict__ mask, const int32_t *__restrict__ block_sums,
                                                                      float2 *__restrict__ pos, int32_t *__restrict__ state,
                                                                      int32_t *__restrict__ birth)
{
    __shared__ int s_wave[TRK_SEED_ROUNDS * TRK_WAVES];
    bool is[TRK_SEED_ROUNDS];
    int rank[TRK_SEED_ROUNDS];
    seed_block_flags(g, cells, mask, nullptr, is, rank, s_wave);
    const int wave = threadIdx.x >> 6, n = block_sums[nb];
    int before = block_sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < TRK_SEED_ROUNDS; k++) {
        for (int j = 0; j < TRK_WAVES; j++) {
            if (is[k] && j == wave) {
                const int slot = n + before + rank[k];                                  // n <= 2^26 and r < 2^26
                if (slot < cap) {
                    int sx, sy;
                    seed_pixel(g, blockIdx.x * TRK_SEED_CELLS + k * TRK_THREADS + (int)threadIdx.x, sx, sy);
                    pos[slot] = make_float2((float)sx, (float)sy);
                    state[slot] = TRK_LIVE;
                    birth[slot] = frame;
                }
            }
            before += s_wave[k * TRK_WAVES + j];
        }
    }
}

int launch_track_seed(int H, int W, int cap, int step, int frame, const uint8_t *mask, float *pos, int32_t *state, int32_t *birth,
                      int32_t *d_n, int32_t *scan, int32_t *counts, hipStream_t s)
{
    SeedGrid g;
    g.h = H; g.w = W; g.step = step; g.gw = (W + step - 1) / step;
    g.ncells = ((H + step - 1) / step) * g.gw;
    const int nb = (g.ncells + TRK_SEED_CELLS - 1) / TRK_SEED_CELLS;
    int32_t *cells = scan, *block_sums = scan + g.ncells;
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, TRK_SEED_COUNTS * sizeof(int32_t), s));
    DFLOW_HIP(hipMemsetAsync(cells, 0, (size_t)g.ncells * sizeof(int32_t), s));
    hipLaunchKernelGGL(track_mark_kernel, dim3((cap + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, s, g, cap,
                       reinterpret_cast<const float2 *>(pos), state, d_n, cells);
    hipLaunchKernelGGL(track_seed_count_kernel, dim3(nb), dim3(TRK_THREADS), 0, s, g, cells, mask, block_sums, counts);
    hipLaunchKernelGGL(track_seed_scan_kernel, dim3(1), dim3(TRK_THREADS), 0, s, nb, cap, block_sums, d_n, counts);
    hipLaunchKernelGGL(track_seed_emit_kernel, dim3(nb), dim3(TRK_THREADS), 0, s, g, nb, cap, frame, cells, mask, block_sums,
                       reinterpret_cast<float2 *>(pos), state, birth);
    return dflow_check_launch("track_seed kernels");
}

// ---- the sparse flow a -> b of the tracks that live in both snapshots
#define TRK_FLOW_COUNTS 3                             // pixels set, tracks that lost their pixel, tracks that took no part
#define TRK_NO_OWNER 0x7fffffff

// the pixel track i claims, -1 if it takes no part
__device__ static inline int track_pixel(int h, int w, const float2 *__restrict__ pos_a, const int32_t *__restrict__ state_a,
                                         const int32_t *__restrict__ state_b, int i, float2 &pa)
{
    if (state_a[i] != TRK_LIVE || state_b[i] != TRK_LIVE) return -1;
    pa = pos_a[i];
    if (!bgr_inside(pa.x, pa.y, w, h)) return -1;
    return (int)rintf(pa.y) * w + (int)rintf(pa.x);
}

__global__ void __launch_bounds__(TRK_THREADS) track_claim_kernel(int h, int w, int cap, const float2 *__restrict__ pos_a,
                                                                  const int32_t *__restrict__ state_a, const int32_t *__restrict__ state_b,
                                                                  int32_t *__restrict__ owner)
{
    const int i = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (i >= cap) return;
    float2 pa;
    const int pix = track_pixel(h, w, pos_a, state_a, state_b, i, pa);
    if (pix >= 0) atomicMin(&owner[pix], i);
}

// lane j is pixel j (j < h*w) and track j (j < cap): the pixel's vector is its winner's, the track is counted
__global__ void __launch_bounds__(TRK_THREADS) track_flow_kernel(int h, int w, int cap, const float2 *__restrict__ pos_a,
                                                                 const int32_t *__restrict__ state_a, const float2 *__restrict__ pos_b,
                                                                 const int32_t *__restrict__ state_b, const int32_t *__restrict__ owner,
                                                                 float *__restrict__ out, int32_t *counts)
{
    const int j = blockIdx.x * TRK_THREADS + threadIdx.x;
    bool is[TRK_FLOW_COUNTS] = {false, false, false};
    if (j < h * w) {
        const int o = owner[j];
        FlowOut v = {0.0f, 0.0f, 0.0f};
        if (o != TRK_NO_OWNER) {
            const float2 pa = pos_a[o], pb = pos_b[o];
            v.u = pb.x - pa.x; v.v = pb.y - pa.y; v.valid = 1.0f;
            is[0] = true;
        }
        reinterpret_cast<FlowOut *>(out)[j] = v;
    }
    if (counts && j < cap) {                                                            // counts is uniform
        float2 pa;
        const int pix = track_pixel(h, w, pos_a, state_a, state_b, j, pa);
        is[2] = pix < 0;
        is[1] = pix >= 0 && owner[pix] != j;
    }
    block_count<TRK_FLOW_COUNTS>(is, counts, 0);
}

int launch_track_flow(int H, int W, int cap, const float *pos_a, const int32_t *state_a, const float *pos_b, const int32_t *state_b,
                      int32_t *owner, float *out, int32_t *counts, hipStream_t s)
{
    const int npix = H * W, nlanes = npix > cap ? npix : cap;
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, TRK_FLOW_COUNTS * sizeof(int32_t), s));
    DFLOW_HIP(hipMemsetD32Async((hipDeviceptr_t)owner, TRK_NO_OWNER, (size_t)npix, s));
    hipLaunchKernelGGL(track_claim_kernel, dim3((cap + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, s, H, W, cap,
                       reinterpret_cast<const float2 *>(pos_a), state_a, state_b, owner);
    hipLaunchKernelGGL(track_flow_kernel, dim3((nlanes + TRK_THREADS - 1) / TRK_THREADS), dim3(TRK_THREADS), 0, s, H, W, cap,
                       reinterpret_cast<const float2 *>(pos_a), state_a, reinterpret_cast<const float2 *>(pos_b), state_b, owner, out,
                       counts);
    return dflow_check_launch("track_flow kernels");
}
