// Prior-flow proposals and the flow advance (include/dflow.h: dflow_prior_proposals, dflow_flow_advance; DESIGN.md "Prior
// proposals").  No counterpart in the reference: its label sets are closed (kNN window + copies of neighbours' winners).
//
// prior_kernel: one pixel per 16-lane DPP row, four pixels per wave.  A pixel's work is a gather: its label row (up to 640
// bytes), up to five prior vectors and up to five descriptor rows of image 2.  The row's lanes read the label row in 256-byte
// pieces (16 lanes x uint4) and compare every piece against all five candidates at once; the smallest matching slot of each
// candidate is a row minimum by DPP.  What is found, appended, full or skipped depends on nothing but the labels, so it is
// decided (identically in all 16 lanes) before any descriptor is read, and only the appended labels pay for a cost.  The cost is
// l1_cost_np's sum in its order: lanes 0..7 of a half row hold the eight running sums of one appended label (two labels per
// row and round), the tree is three DPP exchanges inside the half row (IEEE addition commutes, so both partners of an exchange
// hold the same bits), then the four-element tail in sequence.
#include <math.h>
#include "plane_ops.h"
#include "wave_ops.h"

#define PRIOR_THREADS 256
#define PRIOR_ROW 16                                  // lanes per pixel: one DPP row
#define PRIOR_MAXCAND 5
#define PRIOR_NONE 0x7FFFFFFF

// The vector of pixel `src` of a flow plane as a label (rules 2 and 3 of the definition): false when it is invalid under
// [U,V,valid], when a component is not finite, or when a rounded component lies outside [-32767, 32767].
__device__ static inline bool prior_vector(const float *__restrict__ f, int layout, size_t src, int &dy, int &dx)
{
    float fy, fx;
    if (!flow_vector(f, layout, src, fy, fx)) return false;
    const float ry = rintf(fy), rx = rintf(fx);                             // ties to even
    if (!(fabsf(ry) <= 32767.0f) || !(fabsf(rx) <= 32767.0f)) return false; // NaN and infinities fail the compare
    dy = (int)ry; dx = (int)rx;
    return true;
}

struct PriorArgs {
    int H, W, LP, L, layout, stride;
    uint32_t flags;
    float tphi;
    const void *d1, *d2;
    const float *prior;
    uint32_t *proposals;
    float *lcosts;
    int32_t *nprop, *bestlabels, *counts;
};

// elements 8i + j (i = 0..7) and the tail 64..67 of descriptor row pix, widened to float32
template <typename T> __device__ static inline void desc_load_strided(float (&v)[8], float (&t)[4], const T *__restrict__ base, size_t pix, int j)
{
    const T *row = base + pix * DescPitch<T>::value;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = (float)row[8 * i + j];
    if constexpr (sizeof(T) == 4) {
        const float4 u = *reinterpret_cast<const float4 *>(row + 64);
        t[0] = u.x; t[1] = u.y; t[2] = u.z; t[3] = u.w;
    } else {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 u = *reinterpret_cast<const h4 *>(row + 64);
#pragma unroll
        for (int i = 0; i < 4; i++) t[i] = (float)u[i];
    }
}

template <typename T> __global__ void __launch_bounds__(PRIOR_THREADS) prior_kernel(PriorArgs a)
{
    __shared__ int s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (PRIOR_ROW - 1);
    const int pix = blockIdx.x * (PRIOR_THREADS / PRIOR_ROW) + (threadIdx.x / PRIOR_ROW);
    if (pix < a.H * a.W) {                       // the same for all 16 lanes of a row; so is every branch below but the stores
        const int y = pix / a.W, x = pix % a.W;
        const int ncand = a.stride ? PRIOR_MAXCAND : 1;
        // ---- the candidates: label, target pixel, usable or skipped
        uint32_t cl[PRIOR_MAXCAND];
        int tp[PRIOR_MAXCAND];
        bool ok[PRIOR_MAXCAND];
#pragma unroll
        for (int k = 0; k < PRIOR_MAXCAND; k++) {
            ok[k] = false; cl[k] = 0; tp[k] = 0;
            const int sy = y + (k == 1 ? -a.stride : k == 4 ? a.stride : 0), sx = x + (k == 2 ? -a.stride : k == 3 ? a.stride : 0);
            if (k < ncand && sy >= 0 && sy < a.H && sx >= 0 && sx < a.W) {
                int dy, dx;
                if (prior_vector(a.prior, a.layout, (size_t)sy * a.W + sx, dy, dx)) {
                    const int ty = y + dy, tx = x + dx;
                    if (ty >= 0 && ty < a.H && tx >= 0 && tx < a.W) { ok[k] = true; cl[k] = pack_flow(dy, dx); tp[k] = ty * a.W + tx; }
                }
            }
        }
        // ---- the label row against all candidates: 64 labels per round, the smallest matching slot per candidate
        uint32_t *prow = a.proposals + (size_t)pix * a.LP;
        const int nread = a.nprop[pix];
        const int n0 = nread < 0 ? 0 : nread;                 // a negative count (no stage writes one) must not become a slot
        const int nscan = n0 < a.L ? n0 : a.L;                // nor may a count above maxnprop read past the row
        int m[PRIOR_MAXCAND];
#pragma unroll
        for (int k = 0; k < PRIOR_MAXCAND; k++) m[k] = PRIOR_NONE;
        for (int base = 0; base < nscan; base += 4 * PRIOR_ROW) {
            const int j = base + 4 * lane;
            if (j < nscan) {                                  // j + 3 < LP: LP is a multiple of 16 and nscan <= LP
                const uint4 v = reinterpret_cast<const uint4 *>(prow)[j >> 2];
                const uint32_t lab[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int k = 0; k < PRIOR_MAXCAND; k++)
                        if (ok[k] && j + e < nscan && lab[e] == cl[k]) m[k] = min(m[k], j + e);
            }
        }
#pragma unroll
        for (int k = 0; k < PRIOR_MAXCAND; k++) m[k] = row_min16(m[k]);
        // ---- found / appended / full / skipped, in candidate order
        int n = n0, napp = 0, seed_slot = -1;
        int c_app = 0, c_found = 0, c_full = 0, c_skip = 0;
        uint32_t al[PRIOR_MAXCAND];
        int at[PRIOR_MAXCAND];
#pragma unroll
        for (int k = 0; k < PRIOR_MAXCAND; k++) { al[k] = 0; at[k] = 0; }
#pragma unroll
        for (int k = 0; k < PRIOR_MAXCAND; k++) {
            if (k >= ncand) continue;
            if (!ok[k]) { c_skip++; continue; }
            int slot = m[k] != PRIOR_NONE ? m[k] : -1;
#pragma unroll
            for (int i = 0; i < PRIOR_MAXCAND; i++)           // the labels this pixel appended so far, slots n0 + i
                if (slot < 0 && i < napp && al[i] == cl[k]) slot = n0 + i;
            if (slot >= 0) c_found++;
            else if (n < a.L) {
                slot = n;
#pragma unroll
                for (int i = 0; i < PRIOR_MAXCAND; i++) if (i == napp) { al[i] = cl[k]; at[i] = tp[k]; }
                napp++; n++; c_app++;
            } else c_full++;
            if (k == 0) seed_slot = slot;
        }
        // ---- the costs of the appended labels, two per round: half row h takes label t + h
        if (napp > 0) {
            const int j8 = lane & 7, half = lane >> 3;
            float q[8], qt[4];
            desc_load_strided(q, qt, reinterpret_cast<const T *>(a.d1), (size_t)pix, j8);
            for (int t = 0; t < napp; t += 2) {
                const int c = t + half < napp ? t + half : napp - 1;      // an idle half row repeats the last label and stores nothing
                uint32_t label = al[0];
                int tpix = at[0];
#pragma unroll
                for (int i = 1; i < PRIOR_MAXCAND; i++) if (i == c) { label = al[i]; tpix = at[i]; }
                float b[8], bt[4];
                desc_load_strided(b, bt, reinterpret_cast<const T *>(a.d2), (size_t)tpix, j8);
                float r = fabsf(q[0] - b[0]);
#pragma unroll
                for (int i = 1; i < 8; i++) r = r + fabsf(q[i] - b[i]);
                r = r + dpp_f<DPP_QUAD_PERM(1, 0, 3, 2)>(r);              // r0+r1, r2+r3, r4+r5, r6+r7
                r = r + dpp_f<DPP_QUAD_PERM(2, 3, 0, 1)>(r);              // (r0+r1)+(r2+r3), (r4+r5)+(r6+r7)
                r = r + dpp_f<DPP_ROW_HALF_MIRROR>(r);                    // their sum
#pragma unroll
                for (int i = 0; i < 4; i++) r = r + fabsf(qt[i] - bt[i]);
                if (j8 == 0 && t + half < napp) {
                    prow[n0 + c] = label;
                    a.lcosts[(size_t)pix * a.LP + n0 + c] = r < a.tphi ? r : a.tphi;      // a NaN gives tphi
                }
            }
        }
        if (lane == 0) {
            if (napp > 0) a.nprop[pix] = n;
            if ((a.flags & DFLOW_PRIOR_SEED_LABELS) && seed_slot >= 0) a.bestlabels[pix] = seed_slot;
            if (a.counts) {
                if (c_app) atomicAdd(&s_cnt[0], c_app);
                if (c_found) atomicAdd(&s_cnt[1], c_found);
                if (c_full) atomicAdd(&s_cnt[2], c_full);
                if (c_skip) atomicAdd(&s_cnt[3], c_skip);
            }
        }
    }
    __syncthreads();
    if (a.counts && threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], s_cnt[threadIdx.x]);
}

int launch_prior(const dflow_params *p, const void *d1, const void *d2, const float *prior, int layout, int stride, uint32_t flags,
                 uint32_t *proposals, float *lcosts, int32_t *nprop, int32_t *bestlabels, int32_t *counts, hipStream_t s)
{
    PriorArgs a;
    a.H = p->pich; a.W = p->picw; a.LP = p->label_pitch; a.L = p->maxnprop; a.layout = layout; a.stride = stride;
    a.flags = flags; a.tphi = p->tphi; a.d1 = d1; a.d2 = d2; a.prior = prior; a.proposals = proposals; a.lcosts = lcosts;
    a.nprop = nprop; a.bestlabels = bestlabels; a.counts = counts;
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
    const int n = p->pich * p->picw, per_block = PRIOR_THREADS / PRIOR_ROW;
    with_descr_type(p, [&](auto d) {
        hipLaunchKernelGGL(prior_kernel<typename decltype(d)::T>, dim3((n + per_block - 1) / per_block), dim3(PRIOR_THREADS), 0, s, a);
    });
    return dflow_check_launch("prior_kernel");
}

// ---- flow advance: every usable vector is carried to the pixel it points at; a target takes the claimant with the smallest
// raster index (atomicMin on a uint32 plane: the result does not depend on the order of arrival)
#define ADV_THREADS 256
#define ADV_FREE 0xFFFFFFFFu

__global__ void __launch_bounds__(ADV_THREADS) advance_claim_kernel(int H, int W, const float *__restrict__ flow, int layout,
                                                                    uint32_t *__restrict__ win, int32_t *counts)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W, i = blockIdx.x * ADV_THREADS + threadIdx.x;
    bool part = false;
    if (i < n) {
        const int y = (int)(i / (uint32_t)W), x = (int)(i % (uint32_t)W);
        int dy, dx;
        if (prior_vector(flow, layout, (size_t)i, dy, dx)) {
            const int ty = y + dy, tx = x + dx;
            if (ty >= 0 && ty < H && tx >= 0 && tx < W) { part = true; atomicMin(&win[(size_t)ty * W + tx], i); }
        }
    }
    // counts[1] holds the claimants until the resolve kernel takes the claimed targets off; counts[2] the others
    const bool is[2] = {part, i < n && !part};
    block_count<2>(is, counts, 1);
}

__global__ void __launch_bounds__(ADV_THREADS) advance_resolve_kernel(int H, int W, const float *__restrict__ flow, int layout, int negate,
                                                                      const uint32_t *__restrict__ win, float *__restrict__ out,
                                                                      int32_t *counts)
{
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const uint32_t n = (uint32_t)H * (uint32_t)W, t = blockIdx.x * ADV_THREADS + threadIdx.x;
    bool claimed = false;
    if (t < n) {
        const uint32_t w = win[t];
        float u = 0.0f, v = 0.0f, valid = 0.0f;
        int dy, dx;
        if (w != ADV_FREE && prior_vector(flow, layout, (size_t)w, dy, dx)) {
            claimed = true;
            u = (float)(negate ? -dx : dx); v = (float)(negate ? -dy : dy); valid = 1.0f;    // the integer is negated: 0 stays +0.0
        }
        float *o = out + (size_t)t * 3;
        o[0] = u; o[1] = v; o[2] = valid;
    }
    if (counts) {
        const int c = wave_count(claimed);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
        __syncthreads();
        if (threadIdx.x == 0 && s_cnt) { atomicAdd(&counts[0], s_cnt); atomicSub(&counts[1], s_cnt); }
    }
}

struct AdvWs { uint32_t *win; size_t bytes; };
static AdvWs adv_ws(int H, int W, void *ws)
{
    WsCarver c(ws);
    uint32_t *win = c.take<uint32_t>((size_t)H * W);
    return {win, c.bytes};
}

size_t flow_advance_ws_bytes(int H, int W) { return adv_ws(H, W, nullptr).bytes; }

int launch_flow_advance(int H, int W, const float *flow, int layout, uint32_t flags, float *out, int32_t *counts, void *ws,
                        hipStream_t s)
{
    uint32_t *win = adv_ws(H, W, ws).win;
    const size_t n = (size_t)H * W;
    DFLOW_HIP(hipMemsetAsync(win, 0xFF, n * sizeof(uint32_t), s));
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), s));
    const unsigned blocks = (unsigned)((n + ADV_THREADS - 1) / ADV_THREADS);
    hipLaunchKernelGGL(advance_claim_kernel, dim3(blocks), dim3(ADV_THREADS), 0, s, H, W, flow, layout, win, counts);
    hipLaunchKernelGGL(advance_resolve_kernel, dim3(blocks), dim3(ADV_THREADS), 0, s, H, W, flow, layout,
                       (int)((flags & DFLOW_ADVANCE_NEGATE) != 0), (const uint32_t *)win, out, counts);
    return dflow_check_launch("advance_resolve_kernel");
}
