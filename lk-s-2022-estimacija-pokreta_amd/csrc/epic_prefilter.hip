// EpicFlow's match pre-filter (dflow_epic_prefilter; DESIGN.md "EpicFlow interpolation", "Match pre-filter"): this build's
// own definition of the step that removes unreliable matches before the interpolation.
//
//   stage A, saliency     launch_var_smooth (variational.hip) smooths the three channels of the first image, sigma 0.8;
//                         pf_tensor_kernel takes central differences and sums the structure tensor over the channels;
//                         pf_saliency_kernel smooths the three tensor planes (sigma 1.0, a 32x32 tile + halo in LDS, along x
//                         then y), takes s = sqrt(max(0, lambda_min)) and drops the seeds with s < saliency_th.
//                         Without stage A pf_copy_kernel only marks the seeds.
//   stage B, consistency  the Voronoi diagram and the seed graph of the survivors (epic_build_graph, epic.hip), then
//                         pf_consistency_kernel, one wave per seed: the bounded Dijkstra of epic.h over pref_nn + 1 seeds,
//                         the Nadaraya-Watson estimate of the others in double, the decision against pref_th.  It only marks:
//                         every seed is judged against the whole stage-A survivor set.
//   pf_compact_kernel     zeroes the seeds stage B marked, writes the reason plane and the three counters.
//
// Stage A is float32, one IEEE operation per written operation in a fixed order (-ffp-contract=off).  Either stage writes
// sparse_out pixel by pixel from values read before, so sparse_out may be sparse_in.
#include <math.h>
#include "epic.h"

#define PF_ST 32
#define PF_THREADS 256
#define PF_MAX_RADIUS 3                     // ceil(3 * 1.0)
#define PF_SIGMA_IMAGE 0.8f
#define PF_SIGMA_TENSOR 1.0f
enum { PF_NONE = 0, PF_KEPT = 1, PF_SALIENCY = 2, PF_CONSISTENCY = 3 };
enum { CNT_PF = 8 };                        // three words of EpicWs::cnt: seeds in, dropped by stage A, dropped by stage B

// the six float planes of stage A live where the interpolation keeps its models: stage B has no models
struct PfWs {
    EpicWs epic;
    float *chan[3], *tensor[3];
    uint8_t *reason;      // (H,W) PF_*
    size_t bytes;
};

static PfWs pf_ws(void *ws, int H, int W)
{
    const size_t n = (size_t)H * W;
    PfWs w;
    size_t epic_bytes;
    w.epic = epic_ws(ws, H, W, &epic_bytes);
    for (int i = 0; i < 3; i++) { w.chan[i] = w.epic.model + i * n; w.tensor[i] = w.epic.model + (3 + i) * n; }
    w.reason = (uint8_t *)((uintptr_t)ws + epic_bytes);
    w.bytes = epic_bytes + align256(n);
    return w;
}

size_t epic_prefilter_ws_bytes(int H, int W) { return pf_ws(nullptr, H, W).bytes; }

// J = sum over the channels of (fx fx, fx fy, fy fy), fx = 0.5 (f[x + 1] - f[x - 1]), replicate border
__global__ void __launch_bounds__(PF_THREADS) pf_tensor_kernel(int H, int W, PfWs w)
{
    const int p = blockIdx.x * PF_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p % W;
    const size_t l = (size_t)y * W + clampi(x - 1, 0, W - 1), r = (size_t)y * W + clampi(x + 1, 0, W - 1);
    const size_t t = (size_t)clampi(y - 1, 0, H - 1) * W + x, b = (size_t)clampi(y + 1, 0, H - 1) * W + x;
    float jxx = 0.0f, jxy = 0.0f, jyy = 0.0f;
    for (int c = 0; c < 3; c++) {
        const float *f = w.chan[c];
        const float fx = 0.5f * (f[r] - f[l]), fy = 0.5f * (f[b] - f[t]);
        jxx = c ? jxx + fx * fx : fx * fx;
        jxy = c ? jxy + fx * fy : fx * fy;
        jyy = c ? jyy + fy * fy : fy * fy;
    }
    w.tensor[0][p] = jxx; w.tensor[1][p] = jxy; w.tensor[2][p] = jyy;
}

// The pixel's [U,V,valid] copied to out, or zeros when it is a seed with s < th; reason = PF_NONE / PF_KEPT / PF_SALIENCY.
// in and out may be the same buffer: no __restrict__.
__device__ static inline void pf_stage_a_pixel(int p, bool below, const float *in, float *out, uint8_t *reason)
{
    const float u = in[3 * (size_t)p], v = in[3 * (size_t)p + 1], valid = in[3 * (size_t)p + 2];
    const bool seed = is_seed(in, p), drop = seed && below;
    out[3 * (size_t)p] = drop ? 0.0f : u;
    out[3 * (size_t)p + 1] = drop ? 0.0f : v;
    out[3 * (size_t)p + 2] = drop ? 0.0f : valid;
    reason[p] = seed ? (drop ? PF_SALIENCY : PF_KEPT) : PF_NONE;
}

// Separable Gaussian of the three tensor planes after the pattern of var_smooth_kernel (a halo cell holds the value at the
// clamped coordinate), the smoothed values kept in registers, 4 pixels per thread; then the smaller eigenvalue.
__global__ void __launch_bounds__(PF_THREADS) pf_saliency_kernel(int H, int W, VarTaps taps, PfWs w, const float *sparse_in,
                                                                 double th, float *sparse_out, float *__restrict__ saliency)
{
    constexpr int S = PF_ST + 2 * PF_MAX_RADIUS, PER = PF_ST * PF_ST / PF_THREADS;
    __shared__ float in[S][S + 1];
    __shared__ float mid[S][PF_ST + 1];
    const int r = taps.r, n = PF_ST + 2 * r;
    const int x0 = blockIdx.x * PF_ST, y0 = blockIdx.y * PF_ST;
    float J[3][PER];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *__restrict__ plane = w.tensor[c];
        for (int i = threadIdx.x; i < n * n; i += PF_THREADS) {
            const int ly = i / n, lx = i - ly * n;
            in[ly][lx] = plane[(size_t)clampi(y0 + ly - r, 0, H - 1) * W + clampi(x0 + lx - r, 0, W - 1)];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n * PF_ST; i += PF_THREADS) {
            const int ly = i / PF_ST, lx = i - ly * PF_ST;
            float acc = 0.0f;
            for (int k = 0; k <= 2 * r; k++) acc = acc + taps.t[k] * in[ly][lx + k];
            mid[ly][lx] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int i = threadIdx.x + q * PF_THREADS, ly = i / PF_ST, lx = i - ly * PF_ST;
            float acc = 0.0f;
            for (int k = 0; k <= 2 * r; k++) acc = acc + taps.t[k] * mid[ly + k][lx];
            J[c][q] = acc;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int i = threadIdx.x + q * PF_THREADS, ly = i / PF_ST, lx = i - ly * PF_ST;
        if (y0 + ly >= H || x0 + lx >= W) continue;
        const int p = (y0 + ly) * W + x0 + lx;
        const float jxx = J[0][q], jxy = J[1][q], jyy = J[2][q];
        const float d = jxx - jyy;
        const float lmin = 0.5f * (jxx + jyy) - sqrtf(0.25f * (d * d) + jxy * jxy);
        const float s = sqrtf(fmaxf(0.0f, lmin));
        if (saliency) saliency[p] = s;
        pf_stage_a_pixel(p, (double)s < th, sparse_in, sparse_out, w.reason);
    }
}

// stage A skipped: every seed survives
__global__ void __launch_bounds__(256) pf_copy_kernel(int n, const float *sparse_in, float *sparse_out, uint8_t *reason)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) pf_stage_a_pixel(p, false, sparse_in, sparse_out, reason);
}

// One wave per stage-A survivor s: its nn = pref_nn + 1 nearest seeds, the estimate from all but the first (s itself), in
// double in list order.  A seed with no other seed in reach is kept and its estimate is its own flow.
template <int NSLOT>
__global__ void __launch_bounds__(256) pf_consistency_kernel(int nseeds, int nn, double k, double th2,
                                                             const float *__restrict__ sparse, EpicWs ws,
                                                             uint8_t *__restrict__ reason, float *__restrict__ estimate)
{
    const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wi >= nseeds) return;
    const int s = ws.seeds[wi];
    double sw = 0, su = 0, sv = 0;
    const int nl = epic_dijkstra<NSLOT>(ws, s, nn, lane, [&](int pos, int id, uint64_t g) {
        if (pos == 0) return;
        const double w = exp(-(k * (double)g) / 2000.0);
        const double u = (double)sparse[3 * (size_t)id], v = (double)sparse[3 * (size_t)id + 1];
        sw += w; su += w * u; sv += w * v;
    });
    if (lane != 0) return;
    const double u = (double)sparse[3 * (size_t)s], v = (double)sparse[3 * (size_t)s + 1];
    const double eu = nl > 1 ? su / sw : u, ev = nl > 1 ? sv / sw : v;
    const double du = eu - u, dv = ev - v;
    if (du * du + dv * dv > th2) reason[s] = PF_CONSISTENCY;
    if (estimate) { estimate[2 * (size_t)s] = (float)eu; estimate[2 * (size_t)s + 1] = (float)ev; }
}

__global__ void __launch_bounds__(256) pf_compact_kernel(int n, float *__restrict__ sparse_out, const uint8_t *__restrict__ reason,
                                                         uint8_t *__restrict__ reason_out, uint32_t *__restrict__ cnt)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int r = p < n ? reason[p] : PF_NONE;
    if (r == PF_CONSISTENCY) { sparse_out[3 * (size_t)p] = 0.0f; sparse_out[3 * (size_t)p + 1] = 0.0f; sparse_out[3 * (size_t)p + 2] = 0.0f; }
    if (p < n && reason_out) reason_out[p] = (uint8_t)r;
    const int seeds = __syncthreads_count(r != PF_NONE), a = __syncthreads_count(r == PF_SALIENCY),
              b = __syncthreads_count(r == PF_CONSISTENCY);
    if (threadIdx.x == 0) {
        if (seeds) atomicAdd(&cnt[CNT_PF], (uint32_t)seeds);
        if (a) atomicAdd(&cnt[CNT_PF + 1], (uint32_t)a);
        if (b) atomicAdd(&cnt[CNT_PF + 2], (uint32_t)b);
    }
}

// Counters and timings of the last call on this thread (dflow_epic_prefilter_last_stats).
static thread_local int32_t g_counts[3] = {0, 0, 0};
static thread_local hipEvent_t g_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};

int epic_prefilter_last_stats(int32_t *counts, float *stage_ms)
{
    if (!g_ev[0]) return dflow_set_error(DFLOW_EINVAL, "no pre-filter has run on this thread");
    if (counts)
        for (int i = 0; i < 3; i++) counts[i] = g_counts[i];
    if (stage_ms) {
        DFLOW_HIP(hipEventSynchronize(g_ev[4]));
        for (int i = 0; i < 4; i++) DFLOW_HIP(hipEventElapsedTime(&stage_ms[i], g_ev[i], g_ev[i + 1]));
    }
    return DFLOW_OK;
}

int launch_epic_prefilter(int H, int W, const uint8_t *bgr, const float *sparse_in, const float *edges, double saliency_th,
                          int pref_nn, double pref_th, double k, float *sparse_out, uint8_t *reason, float *saliency,
                          float *estimate, void *wsp, hipStream_t st)
{
    const PfWs w = pf_ws(wsp, H, W);
    const int n = H * W, blocks = (n + 255) / 256;
    if (!g_ev[0])
        for (int i = 0; i < 5; i++) DFLOW_HIP(hipEventCreate(&g_ev[i]));

    DFLOW_HIP(hipEventRecord(g_ev[0], st));
    if (saliency_th != 0.0) {
        const VarTaps taps = var_taps(PF_SIGMA_TENSOR);
        if (taps.r > PF_MAX_RADIUS) return dflow_set_error(DFLOW_EINVAL, "epic_prefilter: tensor radius %d above %d", taps.r, PF_MAX_RADIUS);
        int rc = launch_var_smooth(H, W, bgr, PF_SIGMA_IMAGE, w.chan[0], w.chan[1], w.chan[2], st); if (rc) return rc;
        pf_tensor_kernel<<<blocks, PF_THREADS, 0, st>>>(H, W, w);
        const dim3 tiles((W + PF_ST - 1) / PF_ST, (H + PF_ST - 1) / PF_ST);
        pf_saliency_kernel<<<tiles, PF_THREADS, 0, st>>>(H, W, taps, w, sparse_in, saliency_th, sparse_out, saliency);
    } else {
        if (saliency) DFLOW_HIP(hipMemsetAsync(saliency, 0, (size_t)n * sizeof(float), st));
        pf_copy_kernel<<<blocks, 256, 0, st>>>(n, sparse_in, sparse_out, w.reason);
    }
    DFLOW_HIP(hipEventRecord(g_ev[1], st));
    if (estimate) DFLOW_HIP(hipMemsetAsync(estimate, 0, (size_t)n * 2 * sizeof(float), st));
    int nseeds = 0, rounds = 0;
    if (pref_nn > 0) {
        const int rc = epic_build_graph(H, W, sparse_out, edges, w.epic, st, &nseeds, &rounds, nullptr); if (rc) return rc;
    }
    DFLOW_HIP(hipEventRecord(g_ev[2], st));
    if (nseeds) {
        const int nn = pref_nn + 1, grid = (nseeds + 3) / 4;
        const double th2 = pref_th * pref_th;
        if (nn <= 64) pf_consistency_kernel<1><<<grid, 256, 0, st>>>(nseeds, nn, k, th2, sparse_out, w.epic, w.reason, estimate);
        else pf_consistency_kernel<4><<<grid, 256, 0, st>>>(nseeds, nn, k, th2, sparse_out, w.epic, w.reason, estimate);
    }
    DFLOW_HIP(hipEventRecord(g_ev[3], st));
    DFLOW_HIP(hipMemsetAsync(w.epic.cnt + CNT_PF, 0, 3 * sizeof(uint32_t), st));
    pf_compact_kernel<<<blocks, 256, 0, st>>>(n, sparse_out, w.reason, reason, w.epic.cnt);
    int rc = dflow_check_launch("epic pre-filter kernels"); if (rc) return rc;
    uint32_t h_cnt[3];
    DFLOW_HIP(hipMemcpyAsync(h_cnt, w.epic.cnt + CNT_PF, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    DFLOW_HIP(hipEventRecord(g_ev[4], st));
    DFLOW_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 3; i++) g_counts[i] = (int32_t)h_cnt[i];
    return DFLOW_OK;
}
