// What epic.hip (the interpolation) and epic_prefilter.hip (the match pre-filter) share: the workspace of the geodesic
// Voronoi diagram and the seed graph, the host function that builds both, and the one definition of the bounded per-seed
// Dijkstra over the seed graph.
#pragma once
#include "dflow_common.h"
#include "wave_ops.h"

#define EPIC_CHUNK 4                        // Voronoi rounds launched between two reads of their change counters
#define EPIC_ID_BITS 26                     // seed ids < 8192 * 8192
#define EPIC_ID_MASK ((1ull << EPIC_ID_BITS) - 1)
#define KEY_INF 0xFFFFFFFFFFFFFFFFull

enum { CNT_CHANGED = 0, CNT_NSEEDS = EPIC_CHUNK, CNT_EDGES, CNT_WORDS = 16 };

struct EpicWs {
    uint32_t *cnt;        // CNT_WORDS counters
    uint64_t *key;        // (H,W) (D << 32) | S
    uint16_t *cost;       // (H,W) c(p) in [1, 1001]
    uint32_t *rowbeg;     // (H,W) first edge of a seed's row
    uint32_t *rowend;     // (H,W) degree, then the cursor, then one past the row's last edge
    int32_t *seeds;       // compact list of seed ids
    uint64_t *edges;      // directed seed-graph edges (w << 32) | t
    float *model;         // (H,W,6) per seed: u = m0 + m1 dx + m2 dy, v = m3 + m4 dx + m5 dy
};

// every 4-neighbour pair with different seeds gives two directed edges
static inline size_t epic_max_edges(int H, int W) { return 2 * ((size_t)H * (W - 1) + (size_t)(H - 1) * W); }

static inline EpicWs epic_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    const size_t n = (size_t)H * W;
    WsCarver c(ws);
    EpicWs w;
    w.cnt = c.take<uint32_t>(CNT_WORDS);
    w.key = c.take<uint64_t>(n);
    w.cost = c.take<uint16_t>(n);
    w.rowbeg = c.take<uint32_t>(n);
    w.rowend = c.take<uint32_t>(n);
    w.seeds = c.take<int32_t>(n);
    w.edges = c.take<uint64_t>(epic_max_edges(H, W));
    w.model = c.take<float>(6 * n);
    if (bytes) *bytes = c.bytes;
    return w;
}

// Seed init, the Voronoi rounds and the seed-graph CSR of `sparse` over `edges` into ws (epic.hip).  Synchronises the stream
// (the Voronoi loop reads its change counters back).  *nseeds: the seeds found; *rounds: the Voronoi rounds run; after_voronoi,
// when not null, is recorded between the last round and the graph kernels.
int epic_build_graph(int H, int W, const float *sparse, const float *edges, const EpicWs &ws, hipStream_t st, int *nseeds,
                     int *rounds, hipEvent_t after_voronoi);

__device__ static inline bool is_seed(const float *__restrict__ sparse, int p)
{
    const float u = sparse[3 * (size_t)p], v = sparse[3 * (size_t)p + 1], valid = sparse[3 * (size_t)p + 2];
    return valid > 0.5f && isfinite(u) && isfinite(v);
}

// One wave walks the seed graph from seed s: the nn seeds nearest to s by (G, id), s itself first, in that order; every
// lane calls settled(position, id, G) for each, with the same values, and gets the number of seeds settled back.  The
// frontier holds (G << 26) | id keys in slots j * 64 + lane (j < NSLOT, so nn <= 64 * NSLOT), INF when free; settled ids sit
// in the same layout.  G < 2^34: a settled seed's shortest path has at most nn - 1 edges of weight below 2^26.  A frontier
// entry ranked below nn - settled others can never be settled among the first nn, so the frontier is capped at that size:
// a new entry replaces the largest one or is dropped.  Dropping loses nothing: if the entry's true key is smaller, its
// predecessor on the true path is settled before it and offers it again.
template <int NSLOT, typename F>
__device__ __forceinline__ static int epic_dijkstra(const EpicWs &ws, int s, int nn, int lane, F &&settled)
{
    const int nslot = (nn + 63) >> 6;
    uint64_t fk[NSLOT];
    int lid[NSLOT];
#pragma unroll
    for (int j = 0; j < NSLOT; j++) { fk[j] = KEY_INF; lid[j] = -1; }
    if (lane == 0) fk[0] = (uint64_t)s;
    int nf = 1, nl = 0;
    while (nf > 0) {
        uint64_t m = fk[0];
#pragma unroll
        for (int j = 1; j < NSLOT; j++) m = fk[j] < m ? fk[j] : m;
        m = wave_min_u64(m);
#pragma unroll
        for (int j = 0; j < NSLOT; j++) if (fk[j] == m) fk[j] = KEY_INF;
        nf--;
        const int id = (int)(m & EPIC_ID_MASK);
        const uint64_t g = m >> EPIC_ID_BITS;
#pragma unroll
        for (int j = 0; j < NSLOT; j++) if (j == (nl >> 6) && lane == (nl & 63)) lid[j] = id;
        settled(nl, id, g);
        if (++nl == nn) break;
        const int limit = nn - nl;
        const uint32_t beg = ws.rowbeg[id], end = ws.rowend[id];
        for (uint32_t base = beg; base < end; base += 64) {
            const uint64_t mine = base + lane < end ? ws.edges[base + lane] : 0;
            const int cnt = (int)min(64u, end - base);
            for (int i = 0; i < cnt; i++) {
                const uint64_t e = __shfl(mine, i);
                const uint32_t t = (uint32_t)e;
                const uint64_t nk = ((g + (e >> 32)) << EPIC_ID_BITS) | t;
                bool hit = false;
#pragma unroll
                for (int j = 0; j < NSLOT; j++) hit |= j < nslot && lid[j] == (int)t;
                if (__any(hit)) continue;                              // settled already
#pragma unroll
                for (int j = 0; j < NSLOT; j++)
                    if (fk[j] != KEY_INF && (fk[j] & EPIC_ID_MASK) == t) { hit = true; if (nk < fk[j]) fk[j] = nk; }
                if (__any(hit)) continue;                              // on the frontier: decreased if shorter
                if (nf < limit) {
#pragma unroll
                    for (int j = 0; j < NSLOT; j++) {
                        const uint64_t free_lanes = __ballot(fk[j] == KEY_INF);
                        if (j < nslot && free_lanes) {
                            if (lane == __ffsll((unsigned long long)free_lanes) - 1) fk[j] = nk;
                            break;
                        }
                    }
                    nf++;
                } else {
                    uint64_t mx = 0;
#pragma unroll
                    for (int j = 0; j < NSLOT; j++) if (fk[j] != KEY_INF && fk[j] > mx) mx = fk[j];
                    mx = wave_max_u64(mx);
                    if (nk < mx) {
#pragma unroll
                        for (int j = 0; j < NSLOT; j++) if (fk[j] == mx) fk[j] = nk;
                    }
                }
            }
        }
    }
    return nl;
}
