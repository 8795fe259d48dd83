// Energy and label-change statistics of a labelling (include/dflow.h, DESIGN.md "BCD statistics and the stop rule"): per
// pass the sum of the chosen labels' data costs, the truncated-L1 smoothness over the 4-adjacent pairs, the labels that
// differ from an earlier labelling, and a copy of the labels for the next comparison.  It reads proposals, lcosts, nprop
// and the labels only: the records dflow_bcd_prepare left in a pass's workspace are never touched.
//
// Two launches on the caller's stream, nothing read back, no atomics:
//   bcd_stats_main_kernel   a workgroup takes tiles of BS_TW x BS_TH pixels (grid-stride over at most BS_MAX_BLOCKS blocks,
//                           the pass of a batch on gridDim.y).  Per tile every pixel's chosen label is gathered ONCE: its
//                           flow (and whether it has one) goes into an LDS image of (BS_TH + 1) x (BS_TW + 1) entries, the
//                           extra column and row being the right and lower neighbours of the tile's last pixels, so the
//                           two pairs of a pixel, (p, right of p) and (p, below p), are formed from LDS.  A lane keeps its
//                           own counts and its double sum of data costs; block_reduce (plane_ops.h) adds them in a fixed
//                           order and thread 0 writes the block's partial.
//   bcd_stats_final_kernel  one block per pass: thread t adds the partials t, t + 256, ... in that order, then a fixed
//                           LDS tree; thread 0 writes the pass's dflow_bcd_stats.
// The grid is a function of the geometry alone, so the order of every double addition is fixed: the same inputs give the
// same bits of data_sum on every call, from the single and from the batch entry point.
#include "plane_ops.h"

#define BS_TW 32
#define BS_TH 8
#define BS_THREADS (BS_TW * BS_TH)
#define BS_WAVES (BS_THREADS / 64)
#define BS_PITCH (BS_TW + 1)             // LDS image row: the tile and its right neighbours; odd, so a column walks the banks
#define BS_MAX_BLOCKS 1024               // 4 blocks of 256 threads on each of the 256 CUs
#define BS_MAX_BATCH 8                   // passes whose pointers travel in one launch's arguments

// what a lane, a wave or a block has seen.  A block of an 8192 x 8192 field sees at most 2^16 pixels, 2^17 pairs of at
// most 8 each: 32-bit counts
struct BsPartial {
    double data;
    uint32_t smooth, pairs_trunc, data_trunc, changed, bad, pad;
};

struct BsPass {
    const uint32_t *proposals;
    const float *lcosts;
    const int32_t *nprop, *labels;
    const int32_t *prev;                 // may be NULL; may be prev_out
    int32_t *prev_out;                   // may be NULL
    BsPartial *partials;
    struct dflow_bcd_stats *stats;
};
struct BsArgs {
    int H, W, LP, tpsi;
    float tphi;
    BsPass pass[BS_MAX_BATCH];
};

__device__ __forceinline__ static void bs_merge(BsPartial &a, const BsPartial &b)
{
    a.data = a.data + b.data;
    a.smooth += b.smooth; a.pairs_trunc += b.pairs_trunc; a.data_trunc += b.data_trunc; a.changed += b.changed; a.bad += b.bad;
}

// prev and prev_out may be one buffer: a pixel's old label is read and its new one written by the same thread, and no other
// thread reads prev at that pixel (the neighbours' entries of the LDS image come from `labels`)
__global__ void __launch_bounds__(BS_THREADS) bcd_stats_main_kernel(BsArgs a)
{
    __shared__ uint32_t s_flow[(BS_TH + 1) * BS_PITCH];      // biased flow of the chosen label
    __shared__ uint8_t s_ok[(BS_TH + 1) * BS_PITCH];         // 1: inside the frame with a label in range
    const BsPass ps = a.pass[blockIdx.y];
    const int H = a.H, W = a.W, LP = a.LP;
    const int tiles_x = (W + BS_TW - 1) / BS_TW, tiles_y = (H + BS_TH - 1) / BS_TH;
    const int ntiles = tiles_x * tiles_y;                    // at most 256 * 1024
    const int tid = threadIdx.x, tx = tid % BS_TW, ty = tid / BS_TW;
    BsPartial acc = {};
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x0 = (t % tiles_x) * BS_TW, y0 = (t / tiles_x) * BS_TH;
        // entries of the LDS image: the thread's own pixel first, then the BS_TW + BS_TH entries of the halo (the corner
        // below the last column's neighbour is in no pair and stays unwritten)
        for (int e = tid; e < BS_THREADS + BS_TW + BS_TH; e += BS_THREADS) {
            int ly, lx;
            if (e < BS_THREADS) { ly = ty; lx = tx; }
            else if (e < BS_THREADS + BS_TH) { ly = e - BS_THREADS; lx = BS_TW; }           // right column
            else { ly = BS_TH; lx = e - BS_THREADS - BS_TH; }                               // lower row
            const int y = y0 + ly, x = x0 + lx;
            uint32_t f = 0u;
            bool ok = false;
            if (y < H && x < W) {
                const size_t pix = (size_t)y * W + x;
                const int l = ps.labels[pix];
                ok = l >= 0 && l < ps.nprop[pix] && l < LP;
                if (ok) f = flow_bias(ps.proposals[pix * LP + l]);
                if (e < BS_THREADS) {
                    if (ok) {
                        const float c = ps.lcosts[pix * LP + l];
                        acc.data = acc.data + (double)c;
                        acc.data_trunc += c >= a.tphi;
                    } else {
                        acc.bad++;
                    }
                    if (ps.prev) acc.changed += !ok || ps.prev[pix] != l;
                    if (ps.prev_out) ps.prev_out[pix] = l;
                }
            }
            s_flow[ly * BS_PITCH + lx] = f;
            s_ok[ly * BS_PITCH + lx] = ok;
        }
        __syncthreads();
        // outside the frame s_ok is 0, which also ends the pairs at the last column and row
        if (s_ok[ty * BS_PITCH + tx]) {
            const uint32_t f = s_flow[ty * BS_PITCH + tx];
            if (s_ok[ty * BS_PITCH + tx + 1]) {
                const uint32_t d = flow_l1_biased(f, s_flow[ty * BS_PITCH + tx + 1]);
                acc.smooth += min(d, (uint32_t)a.tpsi);
                acc.pairs_trunc += d >= (uint32_t)a.tpsi;
            }
            if (s_ok[(ty + 1) * BS_PITCH + tx]) {
                const uint32_t d = flow_l1_biased(f, s_flow[(ty + 1) * BS_PITCH + tx]);
                acc.smooth += min(d, (uint32_t)a.tpsi);
                acc.pairs_trunc += d >= (uint32_t)a.tpsi;
            }
        }
        __syncthreads();                                     // the image is rewritten by the next tile
    }
    acc = block_reduce<BS_WAVES>(acc, bs_merge);
    if (tid == 0) ps.partials[blockIdx.x] = acc;
}

struct BsTotal {
    double data;
    uint64_t smooth, pairs_trunc, data_trunc, changed, bad;
};

__global__ void __launch_bounds__(BS_THREADS) bcd_stats_final_kernel(BsArgs a, int nblocks)
{
    __shared__ BsTotal s_tot[BS_THREADS];
    const BsPass ps = a.pass[blockIdx.x];
    BsTotal t = {};
    for (int b = threadIdx.x; b < nblocks; b += BS_THREADS) {
        const BsPartial q = ps.partials[b];
        t.data = t.data + q.data;
        t.smooth += q.smooth; t.pairs_trunc += q.pairs_trunc; t.data_trunc += q.data_trunc; t.changed += q.changed; t.bad += q.bad;
    }
    s_tot[threadIdx.x] = t;
    __syncthreads();
    for (int off = BS_THREADS / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            BsTotal &u = s_tot[threadIdx.x];
            const BsTotal v = s_tot[threadIdx.x + off];
            u.data = u.data + v.data;
            u.smooth += v.smooth; u.pairs_trunc += v.pairs_trunc; u.data_trunc += v.data_trunc; u.changed += v.changed; u.bad += v.bad;
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const BsTotal r = s_tot[0];
    struct dflow_bcd_stats s;
    s.smooth_sum = r.smooth; s.n_pairs_trunc = r.pairs_trunc; s.n_data_trunc = r.data_trunc;
    s.n_changed = r.changed; s.n_bad_label = r.bad; s.data_sum = r.data;
    *ps.stats = s;
}

static int bs_blocks(int H, int W)
{
    const size_t t = (size_t)((W + BS_TW - 1) / BS_TW) * ((H + BS_TH - 1) / BS_TH);
    return (int)(t < BS_MAX_BLOCKS ? t : BS_MAX_BLOCKS);
}

// one pass's part of the workspace: one partial per block of the main kernel; a batch holds npass of them back to back
size_t bcd_stats_ws_bytes(int H, int W) { return align256((size_t)bs_blocks(H, W) * sizeof(BsPartial)); }

int launch_bcd_stats_batch(const dflow_params *p, int npass, const uint32_t *const *proposals, const float *const *lcosts,
                           const int32_t *const *nprop, const int32_t *const *labels, const int32_t *const *prev,
                           int32_t *const *prev_out, struct dflow_bcd_stats *stats, void *ws, hipStream_t s)
{
    const int nblocks = bs_blocks(p->pich, p->picw);
    const size_t per_pass = bcd_stats_ws_bytes(p->pich, p->picw);
    for (int b0 = 0; b0 < npass; b0 += BS_MAX_BATCH) {
        const int nb = npass - b0 < BS_MAX_BATCH ? npass - b0 : BS_MAX_BATCH;
        BsArgs a;
        a.H = p->pich; a.W = p->picw; a.LP = p->label_pitch; a.tpsi = p->tpsi; a.tphi = p->tphi;
        for (int b = 0; b < BS_MAX_BATCH; b++) {
            const int src = b0 + (b < nb ? b : 0);
            BsPass &q = a.pass[b];
            q.proposals = proposals[src]; q.lcosts = lcosts[src]; q.nprop = nprop[src]; q.labels = labels[src];
            q.prev = prev ? prev[src] : nullptr; q.prev_out = prev_out ? prev_out[src] : nullptr;
            q.partials = (BsPartial *)((char *)ws + (size_t)src * per_pass);
            q.stats = stats + src;
        }
        hipLaunchKernelGGL(bcd_stats_main_kernel, dim3(nblocks, nb), dim3(BS_THREADS), 0, s, a);
        hipLaunchKernelGGL(bcd_stats_final_kernel, dim3(nb), dim3(BS_THREADS), 0, s, a, nblocks);
        int rc = dflow_check_launch("BCD statistics kernels");
        if (rc) return rc;
    }
    return DFLOW_OK;
}
