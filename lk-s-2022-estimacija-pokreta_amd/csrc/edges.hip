// Canny edge map: canny_ivice, edge.py:19-35 of the reference (cv2.cvtColor BGR2GRAY -> cv2.GaussianBlur((3,3), 0) ->
// cv2.Canny(threshold1, threshold2), L1 gradient, aperture 3 -> (255 - edges) / 255 as float32).  Integer arithmetic
// throughout, restated from the algorithm (DESIGN.md "Canny edge maps"); the u8 edge map is exact.
//
// Four launches on the caller's stream, no host round trip:
//   canny_front_kernel  per 64x16 tile, all in LDS: gray on the tile + 3 -> 3x3 [1,2,1] blur at BORDER_REFLECT_101 on the
//                       tile + 2 (centres clamped: the blurred image is read with BORDER_REPLICATE) -> Sobel on the tile + 1,
//                       L1 magnitude, 0 outside the image -> non-maximum suppression -> one class byte per pixel (none /
//                       weak / strong); then union-find of the candidates inside the tile (uf_union of union_find.h on LDS):
//                       every candidate's label = the global index of its tile-local root
//   canny_merge_kernel  union-find across tile borders: each candidate on a tile's perimeter links with its 8-neighbours
//                       in other tiles (agent-scope uf_union, union_find.h: parents always point to smaller indices)
//   canny_roots_kernel  every candidate finds its root (and stores it: path compression); strong candidates flag theirs
//   canny_output_kernel edge = candidate whose root is flagged: 255 / 0, and optionally (255 - e) / 255 as float32.
// The edge set (the candidates 8-connected through candidates to a strong one) does not depend on the order in which the
// unions happen, so the atomics cannot change the result.
#include <math.h>
#include "dflow_common.h"
#include "union_find.h"

#define CT_W 64
#define CT_H 16
#define CT_N (CT_W * CT_H)
#define CT_THREADS 256
#define CT_PERIM (2 * CT_W + 2 * CT_H)

enum { CLS_NONE = 0, CLS_WEAK = 1, CLS_STRONG = 2 };

struct CannyWs {
    int32_t *label;     // (H,W) parent pointers of the union-find, -1 for non-candidates
    uint8_t *cls;       // (H,W) CLS_*
    uint8_t *rootflag;  // (H,W) 1 at the root of a component that holds a strong pixel
};

static CannyWs canny_ws(void *ws, int H, int W, size_t *bytes = nullptr)
{
    const size_t n = (size_t)H * W;
    WsCarver c(ws);
    CannyWs w;
    w.label = c.take<int32_t>(n);
    w.cls = c.take<uint8_t>(n);
    w.rootflag = c.take<uint8_t>(n);
    if (bytes) *bytes = c.bytes;
    return w;
}

size_t canny_ws_bytes(int H, int W) { size_t b; canny_ws(nullptr, H, W, &b); return b; }

// BORDER_REFLECT_101 for the blur's taps (v in [-1, n]): -1 -> 1, n -> n - 2; a length-1 axis maps everything to 0
__device__ static inline int reflect101(int v, int n)
{
    if (n == 1) return 0;
    v = v < 0 ? -v : v;
    return v >= n ? 2 * n - 2 - v : v;
}

__global__ void __launch_bounds__(CT_THREADS) canny_front_kernel(const uint8_t *__restrict__ bgr, int H, int W, int lo, int hi,
                                                                 CannyWs ws)
{
    __shared__ int g[CT_H + 6][CT_W + 6];   // gray at real coordinates [gy0, ..] x [gx0, ..]
    __shared__ int b[CT_H + 4][CT_W + 4];   // blurred at real coordinates [by0, ..] x [bx0, ..]
    __shared__ int m[CT_H + 2][CT_W + 2];   // magnitude on the tile + 1 (0 outside the image)
    __shared__ int par[CT_N];
    __shared__ uint8_t cls[CT_N];
    const int tid = threadIdx.x, x0 = blockIdx.x * CT_W, y0 = blockIdx.y * CT_H;

    // gray: every row / column the blur centres below can reach after reflection
    const int gy0 = max(0, y0 - 3), gx0 = max(0, x0 - 3);
    const int gh = min(H - 1, y0 + CT_H + 2) - gy0 + 1, gw = min(W - 1, x0 + CT_W + 2) - gx0 + 1;
    for (int i = tid; i < gh * gw; i += CT_THREADS) {
        const int r = i / gw, c = i % gw;
        g[r][c] = gray_u8(bgr, W, gy0 + r, gx0 + c);
    }
    __syncthreads();
    // blur at the real rows / columns the Sobel taps reach after BORDER_REPLICATE clamping; taps at BORDER_REFLECT_101
    const int by0 = max(0, y0 - 2), bx0 = max(0, x0 - 2);
    const int bh = min(H - 1, y0 + CT_H + 1) - by0 + 1, bw = min(W - 1, x0 + CT_W + 1) - bx0 + 1;
    for (int i = tid; i < bh * bw; i += CT_THREADS) {
        const int r = i / bw, c = i % bw, Y = by0 + r, X = bx0 + c;
        const int ym = reflect101(Y - 1, H) - gy0, yc = Y - gy0, yp = reflect101(Y + 1, H) - gy0;
        const int xm = reflect101(X - 1, W) - gx0, xc = X - gx0, xp = reflect101(X + 1, W) - gx0;
        const int s = (g[ym][xm] + 2 * g[ym][xc] + g[ym][xp]) + 2 * (g[yc][xm] + 2 * g[yc][xc] + g[yc][xp])
                    + (g[yp][xm] + 2 * g[yp][xc] + g[yp][xp]);
        b[r][c] = (s + 8) >> 4;
    }
    __syncthreads();
    // Sobel of the blurred image at (Y, X) (inside the image), taps clamped (BORDER_REPLICATE)
    auto sobel = [&](int Y, int X, int &dx, int &dy) {
        const int ym = clampi(Y - 1, 0, H - 1) - by0, yc = Y - by0, yp = clampi(Y + 1, 0, H - 1) - by0;
        const int xm = clampi(X - 1, 0, W - 1) - bx0, xc = X - bx0, xp = clampi(X + 1, 0, W - 1) - bx0;
        dx = (b[ym][xp] - b[ym][xm]) + 2 * (b[yc][xp] - b[yc][xm]) + (b[yp][xp] - b[yp][xm]);
        dy = (b[yp][xm] - b[ym][xm]) + 2 * (b[yp][xc] - b[ym][xc]) + (b[yp][xp] - b[ym][xp]);
    };
    for (int i = tid; i < (CT_H + 2) * (CT_W + 2); i += CT_THREADS) {
        const int r = i / (CT_W + 2), c = i % (CT_W + 2), Y = y0 - 1 + r, X = x0 - 1 + c;
        int v = 0;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
            int dx, dy;
            sobel(Y, X, dx, dy);
            v = abs(dx) + abs(dy);
        }
        m[r][c] = v;
    }
    __syncthreads();
    // non-maximum suppression (tan 22.5 deg in Q15: 13573), then the class byte
    for (int i = tid; i < CT_N; i += CT_THREADS) {
        const int ly = i / CT_W, lx = i % CT_W, Y = y0 + ly, X = x0 + lx;
        int c = CLS_NONE;
        const int mc = m[ly + 1][lx + 1];
        if (Y < H && X < W && mc > lo) {
            int dx, dy;
            sobel(Y, X, dx, dy);
            const int ax = abs(dx), ay = abs(dy) << 15, t22 = ax * 13573, t67 = t22 + (ax << 16);
            bool keep;
            if (ay < t22) keep = mc > m[ly + 1][lx] && mc >= m[ly + 1][lx + 2];
            else if (ay > t67) keep = mc > m[ly][lx + 1] && mc >= m[ly + 2][lx + 1];
            else {
                const int s = (dx ^ dy) < 0 ? -1 : 1;
                keep = mc > m[ly][lx + 1 - s] && mc > m[ly + 2][lx + 1 + s];
            }
            if (keep) c = mc > hi ? CLS_STRONG : CLS_WEAK;
        }
        cls[i] = (uint8_t)c;
        par[i] = c ? i : -1;
        if (Y < H && X < W) {
            const size_t p = (size_t)Y * W + X;
            ws.cls[p] = (uint8_t)c;
            ws.rootflag[p] = 0;
        }
    }
    __syncthreads();
    // tile-local union-find over the 4 already-visited 8-neighbours (W, NW, N, NE) inside the tile
    for (int i = tid; i < CT_N; i += CT_THREADS) {
        if (!cls[i]) continue;
        const int ly = i / CT_W, lx = i % CT_W;
        if (lx > 0 && cls[i - 1]) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - 1);
        if (ly > 0) {
            if (lx > 0 && cls[i - CT_W - 1]) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CT_W - 1);
            if (cls[i - CT_W]) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CT_W);
            if (lx + 1 < CT_W && cls[i - CT_W + 1]) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CT_W + 1);
        }
    }
    __syncthreads();
    // local index -> global index is monotonic, so the global labels keep "parents point to smaller indices"
    for (int i = tid; i < CT_N; i += CT_THREADS) {
        const int ly = i / CT_W, lx = i % CT_W, Y = y0 + ly, X = x0 + lx;
        if (Y >= H || X >= W) continue;
        int l = -1;
        if (cls[i]) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i);
            l = (y0 + r / CT_W) * W + x0 + r % CT_W;
        }
        ws.label[(size_t)Y * W + X] = l;
    }
}

// Each candidate on a tile's perimeter links with its 8-neighbours in other tiles that have a smaller index; a pair whose
// neighbour in the other tile has the larger index is linked from that neighbour, on its own tile's perimeter (every
// cross-tile pair once).  Tiles run concurrently on different XCDs: parents are read with agent-scope atomic loads (L2, not a
// stale L1 line) and linked with agent-scope atomicMin.
__global__ void __launch_bounds__(CT_THREADS) canny_merge_kernel(int H, int W, CannyWs ws)
{
    const int t = threadIdx.x;
    if (t >= CT_PERIM) return;
    int ly, lx;
    if (t < CT_W) { ly = 0; lx = t; }
    else if (t < 2 * CT_W) { ly = CT_H - 1; lx = t - CT_W; }
    else if (t < 2 * CT_W + CT_H) { ly = t - 2 * CT_W; lx = 0; }
    else { ly = t - 2 * CT_W - CT_H; lx = CT_W - 1; }
    const int Y = blockIdx.y * CT_H + ly, X = blockIdx.x * CT_W + lx;
    if (Y >= H || X >= W) return;
    const int p = Y * W + X;
    if (!ws.cls[p]) return;
    for (int dy = -1; dy <= 0; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            if (dy == 0 && dx >= 0) continue;                  // the neighbours with a smaller index: W, NW, N, NE
            const int ny = Y + dy, nx = X + dx;
            if (ny < 0 || nx < 0 || nx >= W) continue;
            if (ny / CT_H == (int)blockIdx.y && nx / CT_W == (int)blockIdx.x) continue;   // same tile: done in the front kernel
            const int q = ny * W + nx;
            if (ws.cls[q]) uf_union<__HIP_MEMORY_SCOPE_AGENT>(ws.label, p, q);
        }
}

__global__ void __launch_bounds__(CT_THREADS) canny_roots_kernel(int n, CannyWs ws)
{
    const int p = blockIdx.x * CT_THREADS + threadIdx.x;
    if (p >= n) return;
    const int c = ws.cls[p];
    if (!c) return;
    const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(ws.label, p);
    // any ancestor is a valid parent, so concurrent finds that read either value stay correct
    __hip_atomic_store(&ws.label[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c == CLS_STRONG) ws.rootflag[r] = 1;
}

__global__ void __launch_bounds__(CT_THREADS) canny_output_kernel(int n, CannyWs ws, uint8_t *__restrict__ edges,
                                                                  float *__restrict__ ivice)
{
    const int p = blockIdx.x * CT_THREADS + threadIdx.x;
    if (p >= n) return;
    bool e = false;
    if (ws.cls[p]) {
        int r = ws.label[p];
        for (int q; (q = ws.label[r]) != r;) r = q;
        e = ws.rootflag[r] != 0;
    }
    edges[p] = e ? 255 : 0;
    if (ivice) ivice[p] = e ? 0.0f : 1.0f;                     // (255 - e) / 255
}

int launch_canny(int H, int W, const uint8_t *bgr, int lo, int hi, uint8_t *edges, float *ivice, void *ws, hipStream_t s)
{
    const CannyWs w = canny_ws(ws, H, W);
    const dim3 tiles((W + CT_W - 1) / CT_W, (H + CT_H - 1) / CT_H);
    const int n = H * W, blocks = (n + CT_THREADS - 1) / CT_THREADS;
    canny_front_kernel<<<tiles, CT_THREADS, 0, s>>>(bgr, H, W, lo, hi, w);
    canny_merge_kernel<<<tiles, CT_THREADS, 0, s>>>(H, W, w);
    canny_roots_kernel<<<blocks, CT_THREADS, 0, s>>>(n, w);
    canny_output_kernel<<<blocks, CT_THREADS, 0, s>>>(n, w, edges, ivice);
    return dflow_check_launch("canny kernels");
}
