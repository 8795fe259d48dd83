// The two image-plane kernels that connect two levels of a coarse-to-fine run (include/dflow.h: dflow_pyr_down,
// dflow_flow_upsample; DESIGN.md "Coarse to fine").  No counterpart in the reference, which runs one level.
//
// pyr_down_kernel: a workgroup owns a PYR_TW x PYR_TH tile of the half-size image; blockIdx.z is the image of a pair.
//   1. the (2 th + 3) input rows of the tile (rows clamped to the frame, so the vertical pass needs no clamp), each the bytes of
//      columns [cx_lo, cx_hi], as the aligned dwords of the image that cover them: rows are 3w bytes long, so every row has its
//      own byte shift (0..3) inside its first dword; a dword that would end behind the image is put together from bytes;
//   2. the horizontal [1,4,6,4,1] pass from those bytes (columns clamped here) into a uint16 LDS plane, at most 16 * 255 = 4080;
//   3. the vertical pass from that plane with the one rounding, (sum + 128) >> 8; a lane makes the four bytes of one aligned dword
//      of the output and stores them at once where all four belong to the tile, byte by byte at the tile's edges (the
//      neighbouring tile writes the other bytes of such a dword).
// upsample_kernel: one fine pixel per lane, the four coarse corners through flow_good (dflow_common.h), 12 bytes out; the
// three counts through block_count_class (plane_ops.h).
#include <math.h>
#include "plane_ops.h"

#define PYR_THREADS 256
#define PYR_TW 64                                     // output tile: 64 x 16 pixels
#define PYR_TH 16
#define PYR_ROWS (2 * PYR_TH + 3)                     // input rows of a tile
#define PYR_COLS (2 * PYR_TW + 3)                     // input columns of a tile
#define PYR_RAW_DW ((PYR_COLS * 3 + 3 + 3) / 4 + 1)   // dwords of a staged row: its bytes, the shift, rounded up: 100
#define PYR_E (PYR_TW * 3)                            // entries of a row of the uint16 plane

struct PyrArgs {
    int h, w, hc, wc;
    const uint8_t *in[2];
    uint8_t *out[2];
};

__global__ void __launch_bounds__(PYR_THREADS) pyr_down_kernel(PyrArgs a)
{
    __shared__ uint32_t s_raw[PYR_ROWS][PYR_RAW_DW];
    __shared__ uint16_t s_h[PYR_ROWS][PYR_E];
    const uint8_t *__restrict__ in = a.in[blockIdx.z];
    uint8_t *__restrict__ out = a.out[blockIdx.z];
    const int tx0 = blockIdx.x * PYR_TW, ty0 = blockIdx.y * PYR_TH;
    const int tw = min(PYR_TW, a.wc - tx0), th = min(PYR_TH, a.hc - ty0);          // >= 1: the grid covers (hc, wc)
    const int nrows = 2 * th + 3;
    const int cx_lo = max(0, 2 * tx0 - 2), cx_hi = min(a.w - 1, 2 * (tx0 + tw - 1) + 2);
    const int nbytes = (cx_hi - cx_lo + 1) * 3;                                      // <= PYR_COLS * 3
    const size_t total = (size_t)a.h * a.w * 3;

    // ---- 1. the rows, as aligned dwords
    for (int lr = threadIdx.x >> 7; lr < nrows; lr += PYR_THREADS >> 7) {            // 128 lanes per row: up to 100 dwords
        const int gy = min(max(2 * ty0 - 2 + lr, 0), a.h - 1);
        const size_t b0 = ((size_t)gy * a.w + cx_lo) * 3;                            // first byte of the row's part
        const size_t d0 = b0 >> 2;
        const int ndw = (int)(((b0 + nbytes + 3) >> 2) - d0);                        // <= PYR_RAW_DW
        for (int k = threadIdx.x & 127; k < ndw; k += 128) {
            const size_t off = (d0 + k) << 2;
            uint32_t v;
            if (off + 4 <= total) v = reinterpret_cast<const uint32_t *>(in)[d0 + k];
            else {
                v = 0;
                for (int b = 0; b < 4; b++) if (off + b < total) v |= (uint32_t)in[off + b] << (8 * b);
            }
            s_raw[lr][k] = v;
        }
    }
    __syncthreads();

    // ---- 2. horizontal pass: entry e = 3 * ox + c of row lr
    for (int idx = threadIdx.x; idx < nrows * PYR_E; idx += PYR_THREADS) {
        const int lr = idx / PYR_E, e = idx - lr * PYR_E;
        const int ox = e / 3, c = e - 3 * ox;
        if (ox >= tw) continue;
        const int gy = min(max(2 * ty0 - 2 + lr, 0), a.h - 1);
        const int sh = (int)((((size_t)gy * a.w + cx_lo) * 3) & 3);
        const uint8_t *row = reinterpret_cast<const uint8_t *>(s_raw[lr]) + sh + c;
        const int x = 2 * (tx0 + ox);
        const int xm2 = max(x - 2, 0) - cx_lo, xm1 = max(x - 1, 0) - cx_lo, x0 = x - cx_lo;
        const int xp1 = min(x + 1, a.w - 1) - cx_lo, xp2 = min(x + 2, a.w - 1) - cx_lo;
        const int s = (int)row[3 * xm2] + 4 * (int)row[3 * xm1] + 6 * (int)row[3 * x0] + 4 * (int)row[3 * xp1] + (int)row[3 * xp2];
        s_h[lr][e] = (uint16_t)s;
    }
    __syncthreads();

    // ---- 3. vertical pass: the aligned dwords of the output that hold the tile's bytes of row ty0 + oyl
    const int rb = tw * 3;                                                           // the tile's bytes of an output row
    for (int idx = threadIdx.x; idx < th * (PYR_E / 4 + 1); idx += PYR_THREADS) {
        const int oyl = idx / (PYR_E / 4 + 1), k = idx - oyl * (PYR_E / 4 + 1);
        const size_t g0 = ((size_t)(ty0 + oyl) * a.wc + tx0) * 3;                    // first byte of the tile in this row
        const size_t dw = (g0 >> 2) + k;
        const int rel0 = 4 * k - (int)(g0 & 3);                                      // tile-relative entry of the dword's byte 0
        if (rel0 >= rb) continue;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int e = rel0 + b;
            if (e < 0 || e >= rb) continue;
            const int s = (int)s_h[2 * oyl][e] + 4 * (int)s_h[2 * oyl + 1][e] + 6 * (int)s_h[2 * oyl + 2][e]
                          + 4 * (int)s_h[2 * oyl + 3][e] + (int)s_h[2 * oyl + 4][e];
            v |= (uint32_t)((s + 128) >> 8) << (8 * b);
        }
        if (rel0 >= 0 && rel0 + 4 <= rb) reinterpret_cast<uint32_t *>(out)[dw] = v;
        else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (rel0 + b >= 0 && rel0 + b < rb) out[(dw << 2) + b] = (uint8_t)(v >> (8 * b));
        }
    }
}

int launch_pyr_down(int H, int W, const uint8_t *in1, const uint8_t *in2, uint8_t *out1, uint8_t *out2, hipStream_t s)
{
    PyrArgs a;
    a.h = H; a.w = W; a.hc = (H + 1) / 2; a.wc = (W + 1) / 2;
    a.in[0] = in1; a.in[1] = in2; a.out[0] = out1; a.out[1] = out2;
    const dim3 grid((a.wc + PYR_TW - 1) / PYR_TW, (a.hc + PYR_TH - 1) / PYR_TH, in2 ? 2 : 1);
    hipLaunchKernelGGL(pyr_down_kernel, grid, dim3(PYR_THREADS), 0, s, a);
    return dflow_check_launch("pyr_down_kernel");
}

// ---- flow upsampling
#define UPS_THREADS 256

__global__ void __launch_bounds__(UPS_THREADS) upsample_kernel(int H, int W, int hc, int wc, const float *__restrict__ coarse, int layout,
                                                               FlowOut *__restrict__ out, int32_t *counts)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W, i = blockIdx.x * UPS_THREADS + threadIdx.x;
    int kind = -1;                                      // 0 BILINEAR, 1 NEAREST, 2 INVALID
    if (i < n) {
        const int y = (int)(i / (uint32_t)W), x = (int)(i % (uint32_t)W);
        const int y0 = y >> 1, y1 = min((y + 1) >> 1, hc - 1), x0 = x >> 1, x1 = min((x + 1) >> 1, wc - 1);
        float u00, v00, u01, v01, u10, v10, u11, v11;
        const bool g00 = flow_good(coarse, layout, (size_t)y0 * wc + x0, u00, v00);
        const bool g01 = flow_good(coarse, layout, (size_t)y0 * wc + x1, u01, v01);
        const bool g10 = flow_good(coarse, layout, (size_t)y1 * wc + x0, u10, v10);
        const bool g11 = flow_good(coarse, layout, (size_t)y1 * wc + x1, u11, v11);
        FlowOut o = {0.0f, 0.0f, 0.0f};
        kind = 2;
        if (g00 && g01 && g10 && g11) {
            const float u = ((u00 + u01) + (u10 + u11)) * 0.5f, v = ((v00 + v01) + (v10 + v11)) * 0.5f;
            if (isfinite(u) && isfinite(v)) { o.u = u; o.v = v; o.valid = 1.0f; kind = 0; }
        }
        if (kind == 2 && g00) {
            const float u = 2.0f * u00, v = 2.0f * v00;
            if (isfinite(u) && isfinite(v)) { o.u = u; o.v = v; o.valid = 1.0f; kind = 1; }
        }
        out[i] = o;
    }
    block_count_class<3>(kind, counts, 0);
}

int launch_flow_upsample(int H, int W, const float *coarse, int layout, float *out, int32_t *counts, hipStream_t s)
{
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int32_t), s));
    const unsigned n = (unsigned)H * (unsigned)W;
    hipLaunchKernelGGL(upsample_kernel, dim3((n + UPS_THREADS - 1) / UPS_THREADS), dim3(UPS_THREADS), 0, s, H, W, (H + 1) / 2, (W + 1) / 2,
                       coarse, layout, reinterpret_cast<FlowOut *>(out), counts);
    return dflow_check_launch("upsample_kernel");
}
