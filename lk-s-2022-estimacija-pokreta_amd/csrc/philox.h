// Philox4x32-10, the counter-based stream of neighbour.hip's draws and motion_fit.hip's samples: counter (c0, c1, 0, 0), key
// (k0, k1), words 0 and 1 of the output.  One definition: the CPU restatements (oracle, tests/motion_ref.py) agree with it draw
// for draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ static inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t &o0, uint32_t &o1)
{
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}
