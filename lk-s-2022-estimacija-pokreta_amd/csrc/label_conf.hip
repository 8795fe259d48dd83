// Per-pixel confidence of a labelling and the score gate of a flow field (include/dflow.h: dflow_label_confidence,
// dflow_flow_gate; DESIGN.md "Label confidence").  No counterpart in the reference, whose flow carries nothing of what the
// optimiser knew.
//
// label_conf_kernel: a workgroup takes one tile of LC_TW x LC_TH pixels in three steps.
//   gather   every pixel of the tile and of its one-pixel halo on all four sides has its chosen label gathered ONCE: the biased
//            flow, whether the pixel is labelled, and for the tile's own pixels l and n_p, into an LDS image of (LC_TH + 2) x
//            (LC_TW + 2) entries (bcd_stats.hip has the image with two sides).
//   rows     a pixel per 16-lane DPP row, four pixels per wave, LC_ROUNDS rounds per tile (prior.hip's lay-out).  The row's lanes
//            read the pixel's proposals and costs once, 64 slots per step (16 lanes x uint4 / float4), form e_k in double for every
//            slot below n_p and keep the smallest (e, k) among the alternatives: a lane meets its slots in ascending order, so a
//            strict compare keeps the smaller k.  e_k >= 0, so the bits of a double order like a uint64: the row's minimum is
//            three integer row minima (high word, low word with its sign bit flipped, k).  e_l is formed by all 16 lanes alike
//            from one cost and the LDS image.  Lane 0 leaves margin and alt in LDS.
//   write    a pixel per thread: margin, alt and the sparse vector go out coalesced, the six counts through block_count.
// Nothing depends on an order: integer minima, integer counts, one rounding per pixel.
//
// flow_gate_kernel: four pixels per lane and step through plane_ops.h; a lane reads its own four pixels before it writes them,
// so d_out may be d_flow under [U,V,valid].
#include <math.h>
#include "plane_ops.h"
#include "wave_ops.h"

#define LC_TW 32
#define LC_TH 8
#define LC_THREADS (LC_TW * LC_TH)
#define LC_ROW 16                                    // lanes per pixel: one DPP row
#define LC_PER_ROUND (LC_THREADS / LC_ROW)           // pixels a workgroup takes at a time
#define LC_ROUNDS (LC_THREADS / LC_PER_ROUND)
#define LC_PITCH (LC_TW + 2)
#define LC_IMG ((LC_TH + 2) * LC_PITCH)
#define LC_NONE 0x7FFFFFFF

struct LcArgs {
    int H, W, LP, tpsi, min_sep;
    float thresh;
    double lamda;
    const uint32_t *proposals;
    const float *lcosts;
    const int32_t *nprop, *labels;
    float *margin, *sparse;
    int32_t *alt, *counts;
};

// s_k of a slot's biased flow f against the four neighbours' biased flows; t[q] is tpsi, or 0 for a neighbour that adds nothing
__device__ __forceinline__ static uint32_t lc_smooth(uint32_t f, const uint32_t (&g)[4], const uint32_t (&t)[4])
{
    uint32_t s = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) s += min(t[q], flow_l1_biased(f, g[q]));
    return s;
}

template <int MODE> __device__ __forceinline__ static double lc_energy(double lamda, float c, uint32_t s)
{
    if constexpr (MODE == DFLOW_CONF_DATA) return (double)c;
    else return lamda * (double)c + (double)s;
}

template <int MODE> __global__ void __launch_bounds__(LC_THREADS) label_conf_kernel(LcArgs a)
{
    __shared__ uint32_t s_flow[LC_IMG];              // biased flow of the chosen label
    __shared__ int32_t s_label[LC_IMG], s_np[LC_IMG];
    __shared__ uint8_t s_ok[LC_IMG];                 // 1: inside the frame and labelled
    __shared__ float s_margin[LC_THREADS];
    __shared__ int32_t s_alt[LC_THREADS];
    const int H = a.H, W = a.W, LP = a.LP;
    const int tiles_x = (W + LC_TW - 1) / LC_TW;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * LC_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * LC_TH;
    const int tid = threadIdx.x;
    // ---- gather: image entry (ly, lx) is pixel (y0 + ly - 1, x0 + lx - 1)
    for (int e = tid; e < LC_IMG; e += LC_THREADS) {
        const int y = y0 + e / LC_PITCH - 1, x = x0 + e % LC_PITCH - 1;
        uint32_t f = 0u;
        int l = -1, n = 0;
        bool ok = false;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t pix = (size_t)y * W + x;
            l = a.labels[pix];
            n = min(a.nprop[pix], LP);
            ok = l >= 0 && l < n;
            if (ok) f = flow_bias(a.proposals[pix * LP + l]);
        }
        s_flow[e] = f; s_label[e] = l; s_np[e] = n; s_ok[e] = ok;
    }
    __syncthreads();
    // ---- rows: the same branch in all 16 lanes of a row
    const int lane = tid & (LC_ROW - 1);
    for (int r = 0; r < LC_ROUNDS; r++) {
        const int q = r * LC_PER_ROUND + tid / LC_ROW;
        const int ty = q / LC_TW, tx = q % LC_TW, c = (ty + 1) * LC_PITCH + tx + 1;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        float margin = -INFINITY;
        int alt = -1;
        if (s_ok[c]) {
            const size_t row = ((size_t)y * W + x) * LP;
            const int l = s_label[c], n = s_np[c];
            const uint32_t fl = s_flow[c];
            const int nb[4] = {c - LC_PITCH, c - 1, c + 1, c + LC_PITCH};
            uint32_t g[4], t[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { g[k] = s_flow[nb[k]]; t[k] = s_ok[nb[k]] ? (uint32_t)a.tpsi : 0u; }
            const double e_l = lc_energy<MODE>(a.lamda, a.lcosts[row + l], lc_smooth(fl, g, t));
            double best = INFINITY;
            int best_k = LC_NONE;
            for (int base = 0; base < n; base += 4 * LC_ROW) {
                const int j = base + 4 * lane;
                if (j < n) {                                  // j + 3 < LP: LP is a multiple of 16 and n <= LP
                    const uint4 pv = reinterpret_cast<const uint4 *>(a.proposals + row)[j >> 2];
                    const float4 cv = reinterpret_cast<const float4 *>(a.lcosts + row)[j >> 2];
                    const uint32_t lab[4] = {pv.x, pv.y, pv.z, pv.w};
                    const float cost[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t f = flow_bias(lab[i]);
                        const double e = lc_energy<MODE>(a.lamda, cost[i], lc_smooth(f, g, t));
                        if (j + i < n && flow_l1_biased(f, fl) > (uint32_t)a.min_sep && e < best) { best = e; best_k = j + i; }
                    }
                }
            }
            const int hi = __double2hiint(best), lo = __double2loint(best) ^ (int)0x80000000u;
            const int mh = row_min16(hi);
            const int ml = row_min16(hi == mh ? lo : LC_NONE);
            const int mk = row_min16(hi == mh && lo == ml ? best_k : LC_NONE);
            margin = INFINITY;
            if (mk != LC_NONE) {
                alt = mk;
                margin = (float)(__hiloint2double(mh, ml ^ (int)0x80000000u) - e_l);
            }
        }
        if (lane == 0) { s_margin[q] = margin; s_alt[q] = alt; }
    }
    __syncthreads();
    // ---- write: thread tid is pixel (tid / LC_TW, tid % LC_TW) of the tile
    bool is[DFLOW_CONF_COUNTS] = {};
    {
        const int ty = tid / LC_TW, tx = tid % LC_TW, c = (ty + 1) * LC_PITCH + tx + 1;
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            const size_t pix = (size_t)y * W + x;
            const float margin = s_margin[tid];
            const int alt = s_alt[tid];
            const bool ok = s_ok[c], kept = ok && margin >= a.thresh;
            if (a.margin) a.margin[pix] = margin;
            if (a.alt) a.alt[pix] = alt;
            if (a.sparse) {
                FlowOut o = {0.0f, 0.0f, 0.0f};
                if (kept) {
                    const uint32_t f = flow_bias(s_flow[c]);          // the bias is its own inverse
                    o.u = (float)flow_dx(f); o.v = (float)flow_dy(f); o.valid = 1.0f;
                }
                reinterpret_cast<FlowOut *>(a.sparse)[pix] = o;
            }
            is[0] = ok; is[1] = !ok; is[2] = ok && alt < 0; is[3] = ok && margin < 0.0f; is[4] = ok && margin == 0.0f; is[5] = kept;
        }
    }
    block_count<DFLOW_CONF_COUNTS>(is, a.counts, 0);
}

int launch_label_confidence(const dflow_params *p, const uint32_t *proposals, const float *lcosts, const int32_t *nprop,
                            const int32_t *labels, int mode, int min_sep, float thresh, float *margin, int32_t *alt, float *sparse,
                            int32_t *counts, hipStream_t s)
{
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, DFLOW_CONF_COUNTS * sizeof(int32_t), s));
    LcArgs a;
    a.H = p->pich; a.W = p->picw; a.LP = p->label_pitch; a.tpsi = p->tpsi; a.min_sep = min_sep; a.thresh = thresh;
    a.lamda = p->lamda; a.proposals = proposals; a.lcosts = lcosts; a.nprop = nprop; a.labels = labels;
    a.margin = margin; a.sparse = sparse; a.alt = alt; a.counts = counts;
    // at most 256 x 1024 tiles
    const unsigned tiles = (unsigned)((a.W + LC_TW - 1) / LC_TW) * (unsigned)((a.H + LC_TH - 1) / LC_TH);
    if (mode == DFLOW_CONF_DATA) hipLaunchKernelGGL(label_conf_kernel<DFLOW_CONF_DATA>, dim3(tiles), dim3(LC_THREADS), 0, s, a);
    else hipLaunchKernelGGL(label_conf_kernel<DFLOW_CONF_LOCAL>, dim3(tiles), dim3(LC_THREADS), 0, s, a);
    return dflow_check_launch("label_conf_kernel");
}

// ---- the score gate
#define FG_CLASSES 2                                  // good, kept

// a good vector whose score lies in [lo, hi] (a NaN score fails both compares)
__device__ __forceinline__ static bool fg_keep(bool good, float score, float lo, float hi) { return good && score >= lo && score <= hi; }

template <int LAYOUT>
__global__ void __launch_bounds__(PLANE_THREADS) flow_gate_kernel(const float *flow, const float *__restrict__ score, unsigned npix,
                                                                  float lo, float hi, float *out, int32_t *counts)
{
    const unsigned ngroups = (npix + 3u) / 4u, nfull = npix / 4u;
    int ngood = 0, nkept = 0;
    for (unsigned g = blockIdx.x * PLANE_THREADS + threadIdx.x; g < ngroups; g += gridDim.x * PLANE_THREADS) {
        if (g < nfull) {
            float U[4], V[4], valid[4], o[12];
            flow_load4<LAYOUT>(flow, g, U, V, valid);
            const float4 sv = reinterpret_cast<const float4 *>(score)[g];
            const float sc[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool good = valid[k] > 0.5f && isfinite(U[k]) && isfinite(V[k]), keep = fg_keep(good, sc[k], lo, hi);
                ngood += good; nkept += keep;
                o[3 * k] = keep ? U[k] : 0.0f; o[3 * k + 1] = keep ? V[k] : 0.0f; o[3 * k + 2] = keep ? 1.0f : 0.0f;
            }
            float4 *op = reinterpret_cast<float4 *>(out) + (size_t)g * 3;
            op[0] = make_float4(o[0], o[1], o[2], o[3]); op[1] = make_float4(o[4], o[5], o[6], o[7]);
            op[2] = make_float4(o[8], o[9], o[10], o[11]);
        } else {
            // the 1..3 pixels after the last whole group
            for (unsigned p = g * 4u; p < npix; p++) {
                float U, V, valid;
                flow_load1<LAYOUT>(flow, p, U, V, valid);
                const bool good = valid > 0.5f && isfinite(U) && isfinite(V), keep = fg_keep(good, score[p], lo, hi);
                ngood += good; nkept += keep;
                FlowOut o = {0.0f, 0.0f, 0.0f};
                if (keep) { o.u = U; o.v = V; o.valid = 1.0f; }
                reinterpret_cast<FlowOut *>(out)[p] = o;
            }
        }
    }
    // the lanes' counts -> the block's -> one integer atomic per block and counter
    __shared__ int s_cnt[FG_CLASSES];
    if (!counts) return;                              // uniform
    if (threadIdx.x < FG_CLASSES) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (ngood) atomicAdd(&s_cnt[0], ngood);
    if (nkept) atomicAdd(&s_cnt[1], nkept);
    __syncthreads();
    if (threadIdx.x < FG_CLASSES && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

int launch_flow_gate(int H, int W, const float *flow, int layout, const float *score, float lo, float hi, float *out, int32_t *counts,
                     hipStream_t s)
{
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, FG_CLASSES * sizeof(int32_t), s));
    const unsigned npix = (unsigned)H * (unsigned)W;
    const int nblocks = plane_blocks(H, W);
    if (layout == DFLOW_EVAL_UVV)
        hipLaunchKernelGGL(flow_gate_kernel<DFLOW_EVAL_UVV>, dim3(nblocks), dim3(PLANE_THREADS), 0, s, flow, score, npix, lo, hi, out, counts);
    else
        hipLaunchKernelGGL(flow_gate_kernel<DFLOW_EVAL_DYDX>, dim3(nblocks), dim3(PLANE_THREADS), 0, s, flow, score, npix, lo, hi, out, counts);
    return dflow_check_launch("flow_gate_kernel");
}
