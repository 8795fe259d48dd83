// The edge-aware weighted median of a flow field (include/dflow.h: dflow_flow_wmedian; DESIGN.md "Weighted median filter").
// This build's definition; the reference has no counterpart.  Everything is an integer or a copy of input bits.
//
// wmedian_kernel<LAYOUT, GUIDED>: a 32 x 8 tile per 256-thread block, one output pixel per lane; a wave is two tile rows, so the
// 32 lanes an LDS read serves together read 32 consecutive dwords whatever the pitch.  The tile with its halo of `radius` is
// staged once as three dwords per pixel: key U, key V and the ENTRY.  GUIDED: the entry is b | g << 8 | r << 16, its top byte
// 0xFF on a pixel that is not good or lies outside the frame, which makes the weight 0; one v_sad_u8 against the centre's entry
// with a clear top byte is the colour distance of an unmarked pixel (a marked one's is 255 more: the table is staged with zeros
// up to 1023 so that its look-up stays inside).  Not GUIDED: the entry is 1 on a good pixel and 0 elsewhere, the colour weight.
// The median is selected by bits, not by sorting.  Sweep 0 over the window gives W and the least and greatest key of each
// component; the bits above their highest differing bit are common.  Every further sweep decides one bit of both components,
// each at the lane's own position: it sums the weights of the samples that agree with the prefix and have the bit clear; with
// 2 (acc + sum0) >= W the bit is 0, else it is 1 and acc grows by sum0.  2 acc < W <= 2 (acc + weight of the samples under the
// prefix) holds throughout, so the final prefix is the key of a sample that takes part.  A wave sweeps until its last lane is done.
#include <math.h>
#include "plane_ops.h"

#define WMED_THREADS 256
#define WMED_TW 32
#define WMED_TH 8
#define WMED_RMAX 8
#define WMED_HALO ((WMED_TW + 2 * WMED_RMAX) * (WMED_TH + 2 * WMED_RMAX))
#define WMED_NCOLOR 766                               // |db| + |dg| + |dr| = 0 .. 765
#define WMED_COLOR_LDS 1024                           // ... and 255 more on a marked pixel: zeros
#define WMED_MARK 0xFF000000u

__device__ __forceinline__ static uint32_t wmed_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ static float wmed_unkey(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <int LAYOUT, bool GUIDED>
__global__ void __launch_bounds__(WMED_THREADS) wmedian_kernel(int h, int w, const float *__restrict__ flow,
                                                               const uint8_t *__restrict__ bgr, int radius,
                                                               const uint8_t *__restrict__ wspace, const uint8_t *__restrict__ wcolor,
                                                               float reject_thresh, uint32_t flags, float *__restrict__ out,
                                                               int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_ku[WMED_HALO], s_kv[WMED_HALO], s_entry[WMED_HALO];
    __shared__ uint8_t s_space[(WMED_RMAX + 1) * (WMED_RMAX + 1)];
    __shared__ uint8_t s_color[GUIDED ? WMED_COLOR_LDS : 4];

    const int pitch = WMED_TW + 2 * radius, rows = WMED_TH + 2 * radius;
    const int x0 = (int)blockIdx.x * WMED_TW - radius, y0 = (int)blockIdx.y * WMED_TH - radius;
    for (int i = threadIdx.x; i < pitch * rows; i += WMED_THREADS) {
        const int iy = i / pitch, ix = i - iy * pitch;
        const int y = y0 + iy, x = x0 + ix;
        uint32_t ku = 0u, kv = 0u, entry = GUIDED ? WMED_MARK : 0u;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const size_t p = (size_t)y * w + x;
            float U, V;
            const bool good = flow_good(flow, LAYOUT, p, U, V);
            if (good) { ku = wmed_key(U); kv = wmed_key(V); }
            if constexpr (GUIDED) {
                const uint8_t *c = bgr + p * 3;
                entry = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | (good ? 0u : WMED_MARK);
            } else {
                entry = good ? 1u : 0u;
            }
        }
        s_ku[i] = ku; s_kv[i] = kv; s_entry[i] = entry;
    }
    const int nspace = (radius + 1) * (radius + 1);
    if ((int)threadIdx.x < nspace) s_space[threadIdx.x] = wspace ? wspace[threadIdx.x] : (uint8_t)1;
    if constexpr (GUIDED) {
        for (int i = threadIdx.x; i < WMED_COLOR_LDS; i += WMED_THREADS) s_color[i] = i < WMED_NCOLOR ? wcolor[i] : (uint8_t)0;
    }
    __syncthreads();

    const int tx = threadIdx.x & (WMED_TW - 1), ty = threadIdx.x / WMED_TW;
    const int x = (int)blockIdx.x * WMED_TW + tx, y = (int)blockIdx.y * WMED_TH + ty;
    const bool inside = x < w && y < h;
    const int centre = (ty + radius) * pitch + tx + radius;
    const uint32_t own_entry = s_entry[centre];
    const uint32_t own_colour = own_entry & ~WMED_MARK;
    const bool good = inside && (GUIDED ? (own_entry & WMED_MARK) == 0u : own_entry != 0u);

    // the weight of the sample at LDS index i under the space weight S (uniform across the wave)
    auto weight = [&](int i, uint32_t S) -> uint32_t {
        const uint32_t e = s_entry[i];
        if constexpr (GUIDED) {                       // no branch: the look-up of a marked pixel stays inside the table
            const uint32_t c = s_color[__builtin_amdgcn_sad_u8(own_colour, e, 0u)];
            return S * (c & ~(uint32_t)((int32_t)e >> 31));
        } else {
            return S * e;
        }
    };

    // sweep 0: W, and the least and greatest key of each component among the samples that take part
    uint32_t W = 0u, min_u = 0xFFFFFFFFu, max_u = 0u, min_v = 0xFFFFFFFFu, max_v = 0u;
    for (int dy = -radius; dy <= radius; dy++) {
        const int row = centre + dy * pitch, srow = abs(dy) * (radius + 1);
#pragma unroll 1
        for (int dx = -radius; dx <= radius; dx++) {
            const uint32_t wq = weight(row + dx, s_space[srow + abs(dx)]);
            const uint32_t ku = s_ku[row + dx], kv = s_kv[row + dx];
            W += wq;
            min_u = min(min_u, wq ? ku : 0xFFFFFFFFu); max_u = max(max_u, wq ? ku : 0u);
            min_v = min(min_v, wq ? kv : 0xFFFFFFFFu); max_v = max(max_v, wq ? kv : 0u);
        }
    }
    const bool some = inside && W != 0u;

    // the prefix (the bits decided so far, the others 0), the mask of the decided bits plus the one in turn, and that bit;
    // bit == 0: the component is done
    uint32_t pre_u = min_u, pre_v = min_v, bit_u = 0u, bit_v = 0u, mask_u = 0xFFFFFFFFu, mask_v = 0xFFFFFFFFu;
    if (some && min_u != max_u) { bit_u = 0x80000000u >> __clz(min_u ^ max_u); mask_u = ~(bit_u - 1u); pre_u = min_u & (mask_u << 1); }
    if (some && min_v != max_v) { bit_v = 0x80000000u >> __clz(min_v ^ max_v); mask_v = ~(bit_v - 1u); pre_v = min_v & (mask_v << 1); }
    uint32_t acc_u = 0u, acc_v = 0u;
    while (bit_u | bit_v) {
        uint32_t sum_u = 0u, sum_v = 0u;
        for (int dy = -radius; dy <= radius; dy++) {
            const int row = centre + dy * pitch, srow = abs(dy) * (radius + 1);
            // not unrolled, here and in sweep 0: hipcc's own choice, unrolling the unguided loop by four, costs 156 VGPRs
            // (3 waves per SIMD) and was measured 1.5 x slower
#pragma unroll 1
            for (int dx = -radius; dx <= radius; dx++) {
                const uint32_t wq = weight(row + dx, s_space[srow + abs(dx)]);
                const uint32_t ku = s_ku[row + dx], kv = s_kv[row + dx];
                sum_u += ((ku ^ pre_u) & mask_u) == 0u ? wq : 0u;
                sum_v += ((kv ^ pre_v) & mask_v) == 0u ? wq : 0u;
            }
        }
        if (bit_u) {
            if (2u * (acc_u + sum_u) < W) { acc_u += sum_u; pre_u |= bit_u; }
            bit_u >>= 1; mask_u |= bit_u;
        }
        if (bit_v) {
            if (2u * (acc_v + sum_v) < W) { acc_v += sum_v; pre_v |= bit_v; }
            bit_v >>= 1; mask_v |= bit_v;
        }
    }

    FlowOut o = {0.0f, 0.0f, 0.0f};
    bool altered = good;
    if (some) {
        const float mu = wmed_unkey(pre_u), mv = wmed_unkey(pre_v);
        const uint32_t own_ku = s_ku[centre], own_kv = s_kv[centre];
        if (flags & DFLOW_WMED_REJECT) {
            if (good) {
                const float U = wmed_unkey(own_ku), V = wmed_unkey(own_kv);
                if (fabsf(U - mu) + fabsf(V - mv) <= reject_thresh) { o.u = U; o.v = V; o.valid = 1.0f; altered = false; }
            }
        } else if (good || !(flags & DFLOW_WMED_KEEP_HOLES)) {
            o.u = mu; o.v = mv; o.valid = 1.0f;
            altered = good && (pre_u != own_ku || pre_v != own_kv);
        }
    }
    if (inside) reinterpret_cast<FlowOut *>(out)[(size_t)y * w + x] = o;
    const bool valid_out = inside && o.valid != 0.0f;
    const bool is[4] = {good, valid_out, valid_out && !good, altered};
    block_count<4>(is, counts, 0);
}

int launch_flow_wmedian(int H, int W, const float *flow, int layout, const uint8_t *bgr, int radius, const uint8_t *wspace,
                        const uint8_t *wcolor, float reject_thresh, uint32_t flags, float *out, int32_t *counts, hipStream_t s)
{
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
    const dim3 grid((W + WMED_TW - 1) / WMED_TW, (H + WMED_TH - 1) / WMED_TH), block(WMED_THREADS);
    const bool uvv = layout == DFLOW_EVAL_UVV;
#define WMED_LAUNCH(L, G) hipLaunchKernelGGL((wmedian_kernel<L, G>), grid, block, 0, s, H, W, flow, bgr, radius, wspace, wcolor, \
                                             reject_thresh, flags, out, counts)
    if (bgr) { if (uvv) WMED_LAUNCH(DFLOW_EVAL_UVV, true); else WMED_LAUNCH(DFLOW_EVAL_DYDX, true); }
    else { if (uvv) WMED_LAUNCH(DFLOW_EVAL_UVV, false); else WMED_LAUNCH(DFLOW_EVAL_DYDX, false); }
#undef WMED_LAUNCH
    return dflow_check_launch("wmedian_kernel");
}
