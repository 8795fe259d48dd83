// Operations across the 64 lanes of a wave, each defined once: the DPP step and its control words, the results a row of 16
// lanes or the whole wave gets from DPP steps (minimum, inclusive scan), the butterfly reduction, what a ballot gives (count,
// rank), and the wave's LDS fence.  A leaf: it names no stage, and a file that uses it includes it itself.  DESIGN.md, "Wave
// primitives", lists every primitive with its form, where its result lives and its users.
// Precondition of everything here: the whole wave is active and converged at the call (a block of a multiple of 64 threads in one
// dimension, uniform control flow), so that a lane is threadIdx.x & 63.  DPP and ballots read hardware lanes; an inactive lane
// gives a DPP step no source, and is missing from a count or a rank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- DPP: one VALU operand taken from another lane of the wave
// the control words (GFX9 encoding).  The row shifts and the rotation move inside a row of 16 lanes; ROW_BCAST15 gives lane 15
// of a row to the next row, ROW_BCAST31 lane 31 to rows 2 and 3; WAVE_SHR1 is the lane below across the rows.
#define DPP_QUAD_PERM(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
#define DPP_ROW_SHL(n) (0x100 + (n))
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_ROW_ROR(n) (0x120 + (n))
#define DPP_WAVE_SHR1 0x138
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143
// the value of the lane CTRL points at; a lane without such a lane, or in a row that is not in ROWS, keeps its own
template <int CTRL, int ROWS = 0xF> __device__ static inline int dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xF, false); }
template <int CTRL> __device__ static inline float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }
// the value of the lane CTRL points at; 0 where there is no such lane or the row is not in ROWS
template <int CTRL, int ROWS = 0xF> __device__ static inline uint32_t dpp_or0(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false);
}

// ---- a row's result from DPP steps
// the minimum over the 16 lanes of a row, in every lane of it
__device__ static inline int row_min16(int v)
{
    v = min(v, dpp_i<DPP_ROW_ROR(8)>(v));
    v = min(v, dpp_i<DPP_ROW_ROR(4)>(v));
    v = min(v, dpp_i<DPP_ROW_ROR(2)>(v));
    v = min(v, dpp_i<DPP_ROW_ROR(1)>(v));
    return v;
}

// ---- wave results from the six steps of a DPP scan: row_shr 1, 2, 4, 8, then lane 15 of a row into the next row, lane 31 into
// rows 2 and 3
// the minimum over the wave, wave-uniform (lane 63 holds it, read back as a scalar)
__device__ static inline int wave_min(int x)
{
    x = min(x, dpp_i<DPP_ROW_SHR(1)>(x)); x = min(x, dpp_i<DPP_ROW_SHR(2)>(x)); x = min(x, dpp_i<DPP_ROW_SHR(4)>(x)); x = min(x, dpp_i<DPP_ROW_SHR(8)>(x));
    x = min(x, dpp_i<DPP_ROW_BCAST15, 0xA>(x)); x = min(x, dpp_i<DPP_ROW_BCAST31, 0xC>(x));
    return __builtin_amdgcn_readlane(x, 63);
}
// the inclusive scan: every lane gets the sum of x over itself and the lanes below it (lane 63: the wave's total)
__device__ static inline uint32_t wave_scan_add(uint32_t x)
{
    x += dpp_or0<DPP_ROW_SHR(1)>(x); x += dpp_or0<DPP_ROW_SHR(2)>(x); x += dpp_or0<DPP_ROW_SHR(4)>(x); x += dpp_or0<DPP_ROW_SHR(8)>(x);
    x += dpp_or0<DPP_ROW_BCAST15, 0xA>(x); x += dpp_or0<DPP_ROW_BCAST31, 0xC>(x);
    return x;
}

// ---- the butterfly reduction (xor 32 .. 1): the result in every lane; merge(a, b) folds b into a.  For a merge that commutes and
// associates exactly (integer sums, minima, maxima): lanes fold their operands in different orders.  A float or double sum
// wants the fixed order of the __shfl_down tree instead, which block_reduce (plane_ops.h) keeps.
template <typename T, typename Merge> __device__ static inline T wave_reduce_all(T v, Merge merge)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) merge(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ static inline uint64_t wave_min_u64(uint64_t v) { return wave_reduce_all(v, [](uint64_t &a, uint64_t b) { a = b < a ? b : a; }); }
__device__ static inline uint64_t wave_max_u64(uint64_t v) { return wave_reduce_all(v, [](uint64_t &a, uint64_t b) { a = b > a ? b : a; }); }

// ---- ballots
// how many lanes of the wave have `is` (uniform).  The flag is an int, as __ballot takes it: a bool parameter changes the callers'
// device code ("Wave primitives")
__device__ static inline int wave_count(int is) { return (int)__popcll(__ballot(is)); }
// how many lanes below the caller's are set in `mask`
__device__ static inline uint32_t lane_rank(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- What one lane wrote to LDS, every lane of the same wave may read after this (LDS serves a wave's requests in order:
// nothing to wait for, the compiler just must not move the accesses across)
__device__ static inline void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
