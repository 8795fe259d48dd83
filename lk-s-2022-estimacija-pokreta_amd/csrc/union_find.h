// Lock-free union-find with atomicMin (Playne and Hawick; Komura), in LDS (workgroup scope) or global memory (agent scope):
// the Canny edge map (edges.hip) and the small-segment filter (segments.hip).  These are the only loops of the image-plane code
// whose trip count depends on other lanes.
//
// Invariant: L[i] <= i for every element (a root has L[i] == i), and labels only ever decrease: the one kind of write is an
// atomicMin to L[i] with a value below i that belongs to i's set.  So every link points from a larger index to a smaller one
// of the same set, and the root of a set is its smallest index, whatever the order of the unions.
// Loads are atomic at SCOPE: a parent is never taken from a stale cache line or a register while other lanes lower it.
#pragma once
#include <hip/hip_runtime.h>

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
