// The small-segment filter of a sparse flow field (include/dflow.h: dflow_segment_filter; DESIGN.md "Small-segment filter"):
// connected components of the good vectors under "4-adjacent and |dU| + |dV| <= thresh", and every component below min_size
// pixels removed.  This build's definition; the reference's removeSmallSegments (post.hip, dflow_remove_small_segments_host)
// is a sequential flood fill whose result depends on its scan order and stays what it is.
//
// Union-find with atomicMin (union_find.h, where the invariant and the termination arguments are): a label is the raster index
// of a pixel of the same segment that is not larger than the pixel's own.  In global memory a find hangs its start under the
// root it found (UF_HANG).  Four launches, whatever the field holds, and no workgroup waits for another; the first three are
// union_find.h's tile, border and root steps (the header lists their users) around this file's join test:
//   seg_tile_kernel    one workgroup per SEG_TW x SEG_TH tile: the tile's vectors staged in LDS, then uf_tile_step: the right and
//                      down joins merged in LDS, flattened, and every pixel's label written as the raster index of its
//                      tile-local root (-1: no member); sizes zeroed;
//   seg_border_kernel  one lane per join that crosses a tile border (uf_border_pair): the join re-tested from the flow and the
//                      union of the two labels in global memory;
//   seg_root_kernel    uf_root_step: every pixel finds its root, which becomes its label, and adds itself to size[root], a
//                      wave's adds aggregated per distinct root first (wave_add_by_key, plane_ops.h);
//   seg_write_kernel   d_out, the optional planes and the four counts (block_count, plane_ops.h).
// The root of a segment is its smallest raster index.  Everything is integer or a copy of input bits; -ffp-contract=off and
// the join test is one subtraction, fabsf and addition as written.
#include <math.h>
#include "plane_ops.h"
#include "union_find.h"

#define SEG_TW 32
#define SEG_TH 8
#define SEG_THREADS (SEG_TW * SEG_TH)

// a member is a good vector (flow_good, dflow_common.h: GOOD in dflow_flow_consistency).  Two members are joined: symmetric
// (a - b and b - a differ in sign only), and a difference that overflows gives inf, which is not <= a finite thresh
__device__ static inline bool seg_joined(float ua, float va, float ub, float vb, float thresh)
{
    return fabsf(ua - ub) + fabsf(va - vb) <= thresh;
}

__global__ void __launch_bounds__(SEG_THREADS) seg_tile_kernel(int h, int w, const float *__restrict__ flow, int layout, float thresh,
                                                               int *__restrict__ label, int *__restrict__ size)
{
    __shared__ float s_u[SEG_THREADS], s_v[SEG_THREADS];
    __shared__ unsigned char s_mem[SEG_THREADS];
    const int t = threadIdx.x, x = blockIdx.x * SEG_TW + t % SEG_TW, y = blockIdx.y * SEG_TH + t / SEG_TW;
    float u = 0.0f, v = 0.0f;
    // ragged edge tiles: the pixels beyond the frame are no members
    const bool member = x < w && y < h && flow_good(flow, layout, (size_t)y * w + x, u, v);
    s_u[t] = u; s_v[t] = v; s_mem[t] = member;
    uf_tile_step<SEG_TW, SEG_TH>(h, w, member, [&](int, int o) { return s_mem[o] && seg_joined(u, v, s_u[o], s_v[o], thresh); },
                                 label, size);
}

__global__ void __launch_bounds__(SEG_THREADS) seg_border_kernel(int h, int w, const float *__restrict__ flow, int layout, float thresh,
                                                                 int *label)
{
    int p, q;
    if (!uf_border_pair<SEG_TW, SEG_TH>(h, w, blockIdx.x * SEG_THREADS + threadIdx.x, p, q)) return;
    float up, vp, uq, vq;
    if (flow_good(flow, layout, (size_t)p, up, vp) && flow_good(flow, layout, (size_t)q, uq, vq) && seg_joined(up, vp, uq, vq, thresh))
        uf_union<__HIP_MEMORY_SCOPE_AGENT, UF_HANG>(label, p, q);
}

__global__ void __launch_bounds__(SEG_THREADS) seg_root_kernel(int n, int *label, int *size) { uf_root_step<SEG_THREADS>(n, label, size); }

#define SEG_COUNTS 4                                  // segments, segments removed, members, pixels removed

__global__ void __launch_bounds__(SEG_THREADS) seg_write_kernel(int n, const float *flow, int layout, int min_size, int keep_singletons,
                                                                const int *__restrict__ label, const int *__restrict__ size,
                                                                float *out, int *__restrict__ segment, int *__restrict__ size_out,
                                                                int *counts)
{
    const int i = blockIdx.x * SEG_THREADS + threadIdx.x;
    bool member = false, removed = false, is_root = false;
    if (i < n) {
        const int root = label[i];
        member = root >= 0;
        is_root = root == i;
        const int sz = member ? size[root] : 0;
        removed = member && sz < min_size && !(keep_singletons && sz == 1);
        FlowOut o = {0.0f, 0.0f, 0.0f};
        if (member && !removed) {                     // the pixel's own bits; flow may be out (UVV): a lane touches its own pixel only
            float u, v;
            flow_vector(flow, layout, (size_t)i, v, u);
            o.u = u; o.v = v; o.valid = 1.0f;
        }
        reinterpret_cast<FlowOut *>(out)[i] = o;
        if (segment) segment[i] = root;
        if (size_out) size_out[i] = sz;
    }
    const bool is[SEG_COUNTS] = {is_root, is_root && removed, member, removed};
    block_count<SEG_COUNTS>(is, counts, 0);
}

// a label and a size per pixel
struct SegWs { int *label, *size; };
static size_t seg_carve(void *ws, int H, int W, SegWs &r)
{
    WsCarver c(ws);
    r.label = c.take<int>((size_t)H * W);
    r.size = c.take<int>((size_t)H * W);
    return c.bytes;
}

size_t segment_filter_ws_bytes(int H, int W)
{
    SegWs r;
    return seg_carve(nullptr, H, W, r);
}

int launch_segment_filter(int H, int W, const float *flow, int layout, float thresh, int min_size, uint32_t flags, float *out,
                          int32_t *segment, int32_t *size, int32_t *counts, void *ws, hipStream_t s)
{
    SegWs r;
    seg_carve(ws, H, W, r);
    if (counts) DFLOW_HIP(hipMemsetAsync(counts, 0, SEG_COUNTS * sizeof(int32_t), s));
    const int n = H * W, ntx = (W + SEG_TW - 1) / SEG_TW, nty = (H + SEG_TH - 1) / SEG_TH;
    const int nblocks = (n + SEG_THREADS - 1) / SEG_THREADS;
    hipLaunchKernelGGL(seg_tile_kernel, dim3(ntx, nty), dim3(SEG_THREADS), 0, s, H, W, flow, layout, thresh, r.label, r.size);
    hipLaunchKernelGGL(seg_border_kernel, dim3(uf_border_blocks<SEG_TW, SEG_TH>(H, W)), dim3(SEG_THREADS), 0, s, H, W, flow, layout,
                       thresh, r.label);
    hipLaunchKernelGGL(seg_root_kernel, dim3(nblocks), dim3(SEG_THREADS), 0, s, n, r.label, r.size);
    hipLaunchKernelGGL(seg_write_kernel, dim3(nblocks), dim3(SEG_THREADS), 0, s, n, (const float *)flow, layout, min_size,
                       (int)((flags & DFLOW_SEG_KEEP_SINGLETONS) != 0), (const int *)r.label, (const int *)r.size, out, segment, size,
                       counts);
    return dflow_check_launch("segment filter kernels");
}
