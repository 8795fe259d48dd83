// Lock-free union-find with atomicMin (Playne and Hawick; Komura), in LDS (workgroup scope) or global memory (agent scope), and
// the three grid steps of a 4-connected labelling built on it: tile, border, root.  Users: the Canny edge map (edges.hip:
// uf_find and uf_union only; its labeller is 8-connected, fused with the suppression and has no sizes), the small-segment filter
// (segments.hip) and the components of equal SLIC label (superpixels.hip), which both take all three steps.  These, and
// plane_ops.h's wave_each_key, are the only loops of the image-plane code whose trip count depends on other lanes.
//
// Invariant: L[i] <= i for every element (a root has L[i] == i), and labels only ever decrease: the one kind of write is an
// atomicMin to L[i] with a value below i that belongs to i's set.  So every link points from a larger index to a smaller one
// of the same set, and the root of a set is its smallest index, whatever the order of the unions.
// Loads are atomic at SCOPE: a parent is never taken from a stale cache line or a register while other lanes lower it.
#pragma once
#include <hip/hip_runtime.h>
#include "plane_ops.h"

enum { UF_PLAIN = 0, UF_HANG = 1 };

// The root of x.  Terminates: L[x] <= x always and a step is taken only while L[x] < x, so x strictly decreases and is >= 0.
// UF_HANG: the start is then hung directly under what was found (an element of its own set below it: an atomicMin again), so
// that the chains a long winding set builds across many tiles are walked once and not once per lane.
template <int SCOPE, int HANG = UF_PLAIN> __device__ static inline int uf_find(int *L, int x)
{
    const int start = x;
    int parent = -1;                                  // the start's own parent
    for (;;) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, SCOPE);
        if (HANG && parent < 0) parent = p;
        if (p == x) break;
        x = p;
    }
    if (HANG && parent != x) __hip_atomic_fetch_min(&L[start], x, __ATOMIC_RELAXED, SCOPE);
    return x;
}

// Joins the sets of a and b.  Terminates: find never raises a or b; a round either returns or replaces the larger root a by
// the value `old` < a that atomicMin returned (some other lane linked a first), so a + b strictly decreases and is >= 0.
template <int SCOPE, int HANG = UF_PLAIN> __device__ static inline void uf_union(int *L, int a, int b)
{
    for (;;) {
        a = uf_find<SCOPE, HANG>(L, a);
        b = uf_find<SCOPE, HANG>(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;                         // a was still a root and now hangs under b
        a = old;                                      // a hangs under old (or b, the smaller): old's set and b's remain to be joined
    }
}

// ---- a frame's 4-connected components in three launches, tiles of TW x TH pixels, one pixel per thread of a TW * TH block.
// A label is the raster index of a pixel of the same component that is not larger than the pixel's own; -1: no member.

// The tile step, grid (ceil(w / TW), ceil(h / TH)): the tile's right and down joins merged in LDS, and every pixel inside the frame
// gets the raster index of its tile-local root as its label (-1: no member) and size 0.  Every thread of the block calls it, after
// it has stored what `joined` reads in LDS of its own (the first barrier here orders those stores too).  joined(t, o): the
// calling thread's pixel t, a member, and its right or lower neighbour o (tile-local indices) are joined; false where o is no
// member.  t is always the caller's own index, so a predicate may take t's values from registers.  A pixel beyond the frame is
// no member.
template <int TW, int TH, typename Joined>
__device__ static inline void uf_tile_step(int h, int w, bool member, Joined joined, int *__restrict__ label, int *__restrict__ size)
{
    __shared__ int s_lab[TW * TH];                    // tile-local index of a pixel of the same component, -1: no member
    const int t = threadIdx.x, lx = t % TW, ly = t / TW;
    const int x = blockIdx.x * TW + lx, y = blockIdx.y * TH + ly;
    s_lab[t] = member ? t : -1;
    __syncthreads();
    if (member) {
        if (lx + 1 < TW && joined(t, t + 1)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, t, t + 1);
        if (ly + 1 < TH && joined(t, t + TW)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, t, t + TW);
    }
    __syncthreads();
    if (x < w && y < h) {
        int root = -1;
        if (member) {
            // the smallest tile-local index is the smallest raster index of the tile's part of the component
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, t);
            root = (blockIdx.y * TH + r / TW) * w + blockIdx.x * TW + r % TW;
        }
        label[(size_t)y * w + x] = root;
        size[(size_t)y * w + x] = 0;
    }
}

// The joins that cross a tile border: first the (ntx - 1) * h across vertical borders (nvert), then the (nty - 1) * w across
// horizontal ones; the sum is returned.
template <int TW, int TH> __host__ __device__ static inline int uf_border_joins(int h, int w, int &nvert)
{
    nvert = ((w + TW - 1) / TW - 1) * h;
    return nvert + ((h + TH - 1) / TH - 1) * w;
}

// The border step's grid, a lane per join.  A frame of one tile has no joins: the grid keeps one block, whose lanes all return,
// so that the launches are the same whatever the frame.
template <int TW, int TH> static int uf_border_blocks(int h, int w)
{
    int nvert;
    const int b = (uf_border_joins<TW, TH>(h, w, nvert) + TW * TH - 1) / (TW * TH);
    return b > 0 ? b : 1;
}

// The pixel pair (p, q) of join k; false beyond the last join.  The caller tests the pair and, if it is joined, calls
// uf_union<__HIP_MEMORY_SCOPE_AGENT, UF_HANG>(label, p, q).
template <int TW, int TH> __device__ static inline bool uf_border_pair(int h, int w, int k, int &p, int &q)
{
    int nvert;
    if (k >= uf_border_joins<TW, TH>(h, w, nvert)) return false;
    if (k < nvert) {
        p = (k % h) * w + (k / h + 1) * TW - 1;       // the last column of a tile and the first of the next: below w
        q = p + 1;
    } else {
        k -= nvert;
        p = ((k / w + 1) * TH - 1) * w + k % w;       // the last row of a tile and the first of the next: below h
        q = p + w;
    }
    return true;
}

// The root step, a lane per pixel in blocks of THREADS: a member's root becomes its label, and the pixel is added to size[root],
// a wave's adds aggregated per distinct root first (a 446 464-pixel component is 6 976 adds on its root).
template <int THREADS> __device__ static inline void uf_root_step(int n, int *label, int *size)
{
    const int i = blockIdx.x * THREADS + threadIdx.x;
    int root = -1;
    if (i < n && __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) {
        // no root changes any more; other lanes only replace a parent by the root above it, so either value leads there
        root = uf_find<__HIP_MEMORY_SCOPE_AGENT, UF_HANG>(label, i);      // and label[i] = root (UF_HANG)
    }
    wave_add_by_key(root >= 0, root, size, 1);
}
