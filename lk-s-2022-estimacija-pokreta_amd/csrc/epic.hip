// Edge-aware interpolation of a sparse flow field: EpicFlow's sparse-to-dense step (Revaud et al., CVPR 2015, "EPIC"),
// restated with integer geodesics so that the Voronoi diagram, the seed graph and the neighbour lists are exact and do not
// depend on any schedule (DESIGN.md "EpicFlow interpolation").
//
//   epic_init_kernel     cost c(p) = 1 + rint(1000 e(p)), e = clamp(edge, 0, 1) (NaN -> 1); key(seed) = (0, id), else
//                        INF; seeds appended to a compact list (its order is irrelevant: every seed is handled alone)
//   epic_voronoi_kernel  one round: each 64x16 tile relaxes its keys in LDS to local convergence (four directional
//                        sweeps running side by side on LDS atomicMin), the 1-pixel halo read from global memory with
//                        agent-scope atomic loads, improved keys written back with agent-scope atomic stores; a tile that
//                        lowered any key bumps the round's counter.  The host repeats rounds until one changes nothing.
//   epic_graph_*_kernel  seed-graph CSR, rows indexed by the seed's pixel id: count boundary pairs per seed, carve each
//                        seed's row out of one array with an atomic cursor, then scatter the directed edges
//   epic_lists_kernel    one wave per seed: bounded Dijkstra over (G, id) keys (frontier of at most nn - settled entries,
//                        held 4 per lane in registers), then the NW / LA model in double, 6 floats per seed
//   epic_fill_kernel     every pixel evaluates the model of its Voronoi seed
//
// A key is (D << 32) | id with D the integer geodesic distance, so u64 atomicMin realises the lexicographic minimum;
// keys only decrease, so stale reads of another tile's halo cost progress, never correctness.
#include <math.h>
#include "epic.h"

#define VT_W 64
#define VT_H 16
#define VT_THREADS 256

size_t epic_ws_bytes(int H, int W) { size_t b; epic_ws(nullptr, H, W, &b); return b; }

__global__ void __launch_bounds__(256) epic_init_kernel(int n, const float *__restrict__ sparse, const float *__restrict__ edges,
                                                        EpicWs ws)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    float e = edges[p];
    e = isnan(e) ? 1.0f : fminf(fmaxf(e, 0.0f), 1.0f);
    ws.cost[p] = (uint16_t)(1 + (int)rintf(1000.0f * e));
    uint64_t k = KEY_INF;
    if (is_seed(sparse, p)) {
        k = (uint64_t)p;
        ws.seeds[atomicAdd(&ws.cnt[CNT_NSEEDS], 1u)] = p;
    }
    ws.key[p] = k;
    ws.rowend[p] = 0;
}

// key(q) + c(p) + c(q) along a step q -> p, or INF when q has no seed yet.  D of a shortest path is at most
// (H + W) * 2002 < 2^32, so a candidate whose D would overflow is never the minimum and is dropped.
__device__ static inline uint64_t step_key(uint64_t kq, int cq, int cp)
{
    if (kq == KEY_INF) return KEY_INF;
    const uint64_t d = (kq >> 32) + (uint64_t)(cq + cp);
    return d > 0xFFFFFFFFull ? KEY_INF : (d << 32) | (kq & 0xFFFFFFFFull);
}

__global__ void __launch_bounds__(VT_THREADS) epic_voronoi_kernel(int H, int W, EpicWs ws, uint32_t *__restrict__ changed)
{
    __shared__ uint64_t key[VT_H + 2][VT_W + 2];        // tile + 1-pixel halo; INF outside the image
    __shared__ uint16_t cost[VT_H + 2][VT_W + 2];       // 0 outside the image: nothing enters those cells
    __shared__ uint8_t lowered[VT_H][VT_W];
    const int tid = threadIdx.x, x0 = blockIdx.x * VT_W, y0 = blockIdx.y * VT_H;

    bool finite = false;
    for (int i = tid; i < (VT_H + 2) * (VT_W + 2); i += VT_THREADS) {
        const int r = i / (VT_W + 2), c = i % (VT_W + 2), Y = y0 - 1 + r, X = x0 - 1 + c;
        uint64_t k = KEY_INF;
        int cs = 0;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
            const size_t p = (size_t)Y * W + X;
            k = __hip_atomic_load(&ws.key[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cs = ws.cost[p];
        }
        key[r][c] = k;
        cost[r][c] = (uint16_t)cs;
        finite |= k != KEY_INF;
    }
    for (int i = tid; i < VT_H * VT_W; i += VT_THREADS) lowered[i / VT_W][i % VT_W] = 0;
    if (!__syncthreads_or(finite)) return;                // no seed has reached the tile or its halo yet

    // threads 0-15 sweep rows left to right, 16-31 right to left, 32-95 columns downwards, 96-159 upwards.  Each step
    // is an LDS atomicMin, so the four sweeps may cross; an iteration in which no sweep lowered a key is a fixed point.
    int dir = -1, line = 0;
    if (tid < 32) { dir = tid >> 4; line = (tid & 15) + 1; }
    else if (tid < 160) { dir = 2 + ((tid - 32) >> 6); line = ((tid - 32) & 63) + 1; }
    for (bool mine = true; __syncthreads_or(mine);) {
        mine = false;
        if (dir >= 0) {
            const bool horiz = dir < 2, fwd = (dir & 1) == 0;
            const int len = horiz ? VT_W : VT_H;
            int r = horiz ? line : (fwd ? 0 : VT_H + 1), c = horiz ? (fwd ? 0 : VT_W + 1) : line;
            const int dr = horiz ? 0 : (fwd ? 1 : -1), dc = horiz ? (fwd ? 1 : -1) : 0;
            uint64_t kq = __hip_atomic_load(&key[r][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            int cq = cost[r][c];
            for (int s = 0; s < len; s++) {
                r += dr; c += dc;
                const int cp = cost[r][c];
                const uint64_t cand = cp ? step_key(kq, cq, cp) : KEY_INF;
                uint64_t cur;
                if (cand != KEY_INF) {
                    const uint64_t old = __hip_atomic_fetch_min(&key[r][c], cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (cand < old) { mine = true; lowered[r - 1][c - 1] = 1; }
                    cur = cand < old ? cand : old;
                } else {
                    cur = __hip_atomic_load(&key[r][c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                kq = cur; cq = cp;
            }
        }
    }
    bool wrote = false;
    for (int i = tid; i < VT_H * VT_W; i += VT_THREADS) {
        const int ly = i / VT_W, lx = i % VT_W, Y = y0 + ly, X = x0 + lx;
        if (!lowered[ly][lx] || Y >= H || X >= W) continue;
        __hip_atomic_store(&ws.key[(size_t)Y * W + X], key[ly + 1][lx + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        wrote = true;
    }
    if (__syncthreads_or(wrote) && tid == 0) atomicAdd(changed, 1u);
}

// the right and lower 4-neighbour of p whose seed differs from p's: (seed of p, seed of q, edge weight)
template <typename F> __device__ static inline void boundary_pairs(int H, int W, int p, const EpicWs &ws, F f)
{
    const int y = p / W, x = p % W;
    const uint64_t kp = ws.key[p];
    if (kp == KEY_INF) return;                            // no seed at all
    const uint32_t s = (uint32_t)kp, dp = (uint32_t)(kp >> 32), cp = ws.cost[p];
    const int nb[2] = {x + 1 < W ? p + 1 : -1, y + 1 < H ? p + W : -1};
    for (int j = 0; j < 2; j++) {
        if (nb[j] < 0) continue;
        const uint64_t kq = ws.key[nb[j]];
        const uint32_t t = (uint32_t)kq;
        if (kq == KEY_INF || t == s) continue;
        f(s, t, dp + cp + ws.cost[nb[j]] + (uint32_t)(kq >> 32));
    }
}

__global__ void __launch_bounds__(256) epic_graph_count_kernel(int H, int W, EpicWs ws)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    boundary_pairs(H, W, p, ws, [&](uint32_t s, uint32_t t, uint32_t) {
        atomicAdd(&ws.rowend[s], 1u);
        atomicAdd(&ws.rowend[t], 1u);
    });
}

__global__ void __launch_bounds__(256) epic_graph_alloc_kernel(int nseeds, EpicWs ws)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nseeds) return;
    const int s = ws.seeds[i];
    const uint32_t beg = atomicAdd(&ws.cnt[CNT_EDGES], ws.rowend[s]);
    ws.rowbeg[s] = beg;
    ws.rowend[s] = beg;                                   // the fill kernel's cursor; one past the row when it is done
}

__global__ void __launch_bounds__(256) epic_graph_fill_kernel(int H, int W, EpicWs ws)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    boundary_pairs(H, W, p, ws, [&](uint32_t s, uint32_t t, uint32_t w) {
        ws.edges[atomicAdd(&ws.rowend[s], 1u)] = ((uint64_t)w << 32) | t;
        ws.edges[atomicAdd(&ws.rowend[t], 1u)] = ((uint64_t)w << 32) | s;
    });
}

// One wave per seed s: the bounded Dijkstra of epic.h (frontier of at most nn - settled entries, held 4 per lane in
// registers, so nn <= 256), the model's sums accumulated as each seed settles.
__global__ void __launch_bounds__(256) epic_lists_kernel(int H, int W, int nseeds, int nn, double k, int method,
                                                         const float *__restrict__ sparse, EpicWs ws,
                                                         int32_t *__restrict__ lists, uint64_t *__restrict__ list_g)
{
    const int lane = threadIdx.x & 63, wi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wi >= nseeds) return;
    const int s = ws.seeds[wi], xs = s % W, ys = s / W;
    double sw = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0, su = 0, sv = 0, sxu = 0, syu = 0, sxv = 0, syv = 0;
    const int nl = epic_dijkstra<4>(ws, s, nn, lane, [&](int pos, int id, uint64_t g) {
        if (lists && lane == 0) lists[(size_t)s * nn + pos] = id;
        if (list_g && lane == 0) list_g[(size_t)s * nn + pos] = g;
        // the model's sums, in list order; every lane holds the same values
        const double w = id == s ? 1.0 : exp(-(k * (double)g) / 2000.0);
        const double dx = (double)(id % W - xs), dy = (double)(id / W - ys);
        const double u = (double)sparse[3 * (size_t)id], v = (double)sparse[3 * (size_t)id + 1];
        const double wx = w * dx, wy = w * dy;
        sw += w; sx += wx; sy += wy; sxx += wx * dx; sxy += wx * dy; syy += wy * dy;
        su += w * u; sv += w * v; sxu += wx * u; syu += wy * u; sxv += wx * v; syv += wy * v;
    });
    if (lane != 0) return;
    const double mu = su / sw, mv = sv / sw;
    float out[6] = {(float)mu, 0.0f, 0.0f, (float)mv, 0.0f, 0.0f};
    if (method == DFLOW_EPIC_LA && nl >= 3) {
        const double mx = sx / sw, my = sy / sw;
        const double cxx = sxx / sw - mx * mx, cxy = sxy / sw - mx * my, cyy = syy / sw - my * my;
        const double h = 0.5 * (cxx - cyy);
        const double lmin = 0.5 * (cxx + cyy) - sqrt(h * h + cxy * cxy);
        if (lmin >= DFLOW_EPIC_TAU) {
            const double det = cxx * cyy - cxy * cxy;
            const double cxu = sxu / sw - mx * mu, cyu = syu / sw - my * mu, cxv = sxv / sw - mx * mv, cyv = syv / sw - my * mv;
            const double bu = (cyy * cxu - cxy * cyu) / det, cu = (cxx * cyu - cxy * cxu) / det;
            const double bv = (cyy * cxv - cxy * cyv) / det, cv = (cxx * cyv - cxy * cxv) / det;
            out[0] = (float)(mu - bu * mx - cu * my); out[1] = (float)bu; out[2] = (float)cu;
            out[3] = (float)(mv - bv * mx - cv * my); out[4] = (float)bv; out[5] = (float)cv;
        }
    }
    for (int j = 0; j < 6; j++) ws.model[(size_t)s * 6 + j] = out[j];
}

__global__ void __launch_bounds__(256) epic_fill_kernel(int H, int W, EpicWs ws, float *__restrict__ flow,
                                                        int32_t *__restrict__ seed_of, uint32_t *__restrict__ dist)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const uint64_t kp = ws.key[p];
    float fy = 0.0f, fx = 0.0f;
    if (kp != KEY_INF) {
        const int s = (int)(uint32_t)kp;
        const float dx = (float)(p % W - s % W), dy = (float)(p / W - s / W);
        const float *m = ws.model + (size_t)s * 6;
        fx = (m[0] + m[1] * dx) + m[2] * dy;
        fy = (m[3] + m[4] * dx) + m[5] * dy;
    }
    flow[2 * (size_t)p] = fy;                             // [dy, dx]: v, then u
    flow[2 * (size_t)p + 1] = fx;
    if (seed_of) seed_of[p] = kp == KEY_INF ? -1 : (int32_t)(uint32_t)kp;
    if (dist) dist[p] = (uint32_t)(kp >> 32);
}

// Timings of the last call on this thread (dflow_epic_last_stats).
static thread_local int g_rounds = 0;
static thread_local hipEvent_t g_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};

int epic_last_stats(int32_t *rounds, float *stage_ms)
{
    if (rounds) *rounds = g_rounds;
    if (stage_ms) {
        if (!g_ev[0]) return dflow_set_error(DFLOW_EINVAL, "no interpolation has run on this thread");
        DFLOW_HIP(hipEventSynchronize(g_ev[4]));
        for (int i = 0; i < 4; i++) DFLOW_HIP(hipEventElapsedTime(&stage_ms[i], g_ev[i], g_ev[i + 1]));
    }
    return DFLOW_OK;
}

int epic_build_graph(int H, int W, const float *sparse, const float *edges, const EpicWs &ws, hipStream_t st, int *nseeds,
                     int *rounds, hipEvent_t after_voronoi)
{
    const int n = H * W, blocks = (n + 255) / 256;
    const dim3 tiles((W + VT_W - 1) / VT_W, (H + VT_H - 1) / VT_H);
    // A round settles at least the next tile crossing of every shortest path, and a shortest path crosses each pair of
    // neighbouring pixels in different tiles at most once.
    const long long max_rounds = (long long)H * (tiles.x - 1) + (long long)W * (tiles.y - 1) + 2;
    DFLOW_HIP(hipMemsetAsync(ws.cnt, 0, CNT_WORDS * 4, st));
    epic_init_kernel<<<blocks, 256, 0, st>>>(n, sparse, edges, ws);
    uint32_t h_cnt[EPIC_CHUNK + 1];
    for (long long round = 0;;) {
        DFLOW_HIP(hipMemsetAsync(ws.cnt + CNT_CHANGED, 0, EPIC_CHUNK * 4, st));
        for (int j = 0; j < EPIC_CHUNK; j++) epic_voronoi_kernel<<<tiles, VT_THREADS, 0, st>>>(H, W, ws, ws.cnt + CNT_CHANGED + j);
        int rc = dflow_check_launch("epic_voronoi_kernel"); if (rc) return rc;
        DFLOW_HIP(hipMemcpyAsync(h_cnt, ws.cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
        DFLOW_HIP(hipStreamSynchronize(st));
        int j = 0;
        while (j < EPIC_CHUNK && h_cnt[CNT_CHANGED + j]) j++;
        if (j < EPIC_CHUNK) { *rounds = (int)(round + j + 1); break; }
        round += EPIC_CHUNK;
        if (round >= max_rounds)
            return dflow_set_error(DFLOW_EHIP, "epic: the Voronoi relaxation still changed after %lld rounds", round);
    }
    *nseeds = (int)h_cnt[CNT_NSEEDS];
    if (after_voronoi) DFLOW_HIP(hipEventRecord(after_voronoi, st));
    if (*nseeds) {
        epic_graph_count_kernel<<<blocks, 256, 0, st>>>(H, W, ws);
        epic_graph_alloc_kernel<<<(*nseeds + 255) / 256, 256, 0, st>>>(*nseeds, ws);
        epic_graph_fill_kernel<<<blocks, 256, 0, st>>>(H, W, ws);
    }
    return dflow_check_launch("epic graph kernels");
}

int launch_epic(int H, int W, const float *sparse, const float *edges, int nn, double k, int method, float *flow,
                int32_t *seed_of, uint32_t *dist, int32_t *lists, uint64_t *list_g, void *wsp, hipStream_t st)
{
    const EpicWs ws = epic_ws(wsp, H, W);
    const int n = H * W, blocks = (n + 255) / 256;
    if (!g_ev[0])
        for (int i = 0; i < 5; i++) DFLOW_HIP(hipEventCreate(&g_ev[i]));
    g_rounds = 0;

    DFLOW_HIP(hipEventRecord(g_ev[0], st));
    int nseeds = 0;
    const int rc = epic_build_graph(H, W, sparse, edges, ws, st, &nseeds, &g_rounds, g_ev[1]);
    if (rc) return rc;
    DFLOW_HIP(hipEventRecord(g_ev[2], st));
    if (lists) DFLOW_HIP(hipMemsetAsync(lists, 0xFF, (size_t)n * nn * sizeof(int32_t), st));
    if (list_g) DFLOW_HIP(hipMemsetAsync(list_g, 0xFF, (size_t)n * nn * sizeof(uint64_t), st));
    if (nseeds) epic_lists_kernel<<<(nseeds + 3) / 4, 256, 0, st>>>(H, W, nseeds, nn, k, method, sparse, ws, lists, list_g);
    DFLOW_HIP(hipEventRecord(g_ev[3], st));
    epic_fill_kernel<<<blocks, 256, 0, st>>>(H, W, ws, flow, seed_of, dist);
    DFLOW_HIP(hipEventRecord(g_ev[4], st));
    return dflow_check_launch("epic kernels");
}
