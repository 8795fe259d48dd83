// Shared host/device helpers of libdflow.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dflow.h"

#define DFLOW_FILL_PROPOSAL 0xFFFFFFFFu /* [-1,-1], daisy i flann.py:89 */
#define DFLOW_FILL_COST 1000.0f         /* daisy i flann.py:90 */

// Geometry of the cell grid (daisy i flann.py:42-43,85-86; ragged last cells: DESIGN.md "Geometry").
struct Geom {
    int H, W, ch, cw, ncx, ncy, win;
    __host__ __device__ int cellx(int x) const { int c = x / cw; return c < ncx ? c : ncx - 1; }
    __host__ __device__ int celly(int y) const { int c = y / ch; return c < ncy ? c : ncy - 1; }
    __host__ __device__ int x0(int ci) const { return ci * cw; }
    __host__ __device__ int y0(int cj) const { return cj * ch; }
    __host__ __device__ int x1(int ci) const { return ci == ncx - 1 ? W : (ci + 1) * cw; }
    __host__ __device__ int y1(int cj) const { return cj == ncy - 1 ? H : (cj + 1) * ch; }
    // the candidate cells of query cell (qci, qcj): [imin, imax] x [jmin, jmax]; slot = its place in the reference order
    // (ci outer, cj inner: Q2)
    struct Window {
        int imin, imax, jmin, jmax;
        __host__ __device__ int slot(int ci, int cj) const { return (ci - imin) * (jmax - jmin + 1) + (cj - jmin); }
    };
    __host__ __device__ Window window(int qci, int qcj) const
    {
        return {max(0, qci - win), min(ncx - 1, qci + win), max(0, qcj - win), min(ncy - 1, qcj + win)};
    }
};

// pixels of the largest cell (the last one: the ragged cells are the larger ones)
__host__ __device__ static inline int max_cell_points(const Geom &g)
{
    return (g.x1(g.ncx - 1) - g.x0(g.ncx - 1)) * (g.y1(g.ncy - 1) - g.y0(g.ncy - 1));
}

// a compile-time int as a type (selects an instantiation of a generic lambda)
template <int V> struct IntC { static constexpr int value = V; };

static inline Geom make_geom(const dflow_params *p)
{
    Geom g;
    g.H = p->pich; g.W = p->picw; g.ch = p->cellh; g.cw = p->cellw;
    g.ncx = p->picw / p->cellw; g.ncy = p->pich / p->cellh; g.win = p->window;
    return g;
}

// luma of pixel (y, x) of a (H,W,3) BGR u8 image: cv::cvtColor BGR2GRAY on u8 (fixed point, 14 fractional bits, round half
// up).  DAISY (daisy.hip) and the Canny edge map (edges.hip) both start from it.
__device__ static inline int gray_u8(const uint8_t *__restrict__ bgr, int W, int y, int x)
{
    const uint8_t *px = bgr + ((size_t)y * W + x) * 3;
    return (1868 * px[0] + 9617 * px[1] + 4899 * px[2] + 8192) >> 14;
}

// label packing: int16 dy | int16 dx << 16
__host__ __device__ static inline uint32_t pack_flow(int dy, int dx)
{
    return (uint32_t)(uint16_t)(int16_t)dy | ((uint32_t)(uint16_t)(int16_t)dx << 16);
}
__host__ __device__ static inline int flow_dy(uint32_t f) { return (int)(int16_t)(f & 0xFFFFu); }
__host__ __device__ static inline int flow_dx(uint32_t f) { return (int)(int16_t)(f >> 16); }

// The vector (fy, fx) of pixel `src` of a flow plane in either layout: DFLOW_EVAL_UVV (H,W,3) [U,V,valid], false when the pixel
// is not valid (a NaN compares false); DFLOW_EVAL_DYDX (H,W,2) [dy,dx], every pixel valid.  prior.hip and pyramid.hip read
// their flows through it.
__device__ static inline bool flow_vector(const float *__restrict__ f, int layout, size_t src, float &fy, float &fx)
{
    if (layout == DFLOW_EVAL_UVV) {
        const float *q = f + src * 3;
        if (!(q[2] > 0.5f)) return false;
        fx = q[0]; fy = q[1];
    } else {
        const float *q = f + src * 2;
        fy = q[0]; fx = q[1];
    }
    return true;
}

// A good vector (u, v) = (fx, fy): valid under its layout and both components finite.  What pyramid.hip doubles, consistency.hip
// checks and segments.hip takes as a member; FlowOut is the [U,V,valid] pixel the three write.
__device__ static inline bool flow_good(const float *__restrict__ f, int layout, size_t src, float &u, float &v)
{
    return flow_vector(f, layout, src, v, u) && isfinite(u) && isfinite(v);
}
struct FlowOut { float u, v, valid; };

__device__ static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// |dy-dy'| + |dx-dx'| of two packed labels (purepsi, daisy i flann.py:114-115): flip the sign bits so that the
// int16 halves order like uint16, then one v_sad_u16.
__device__ static inline uint32_t flow_bias(uint32_t f) { return f ^ 0x80008000u; }
__device__ static inline uint32_t flow_l1_biased(uint32_t a, uint32_t b) { return __builtin_amdgcn_sad_u16(a, b, 0u); }

// ---- descriptor storage: float32 rows of 68 values (272 bytes), or -- DFLOW_FLAG_DESCR_F16 -- binary16 rows of 68 values
// + 4 zero pads (144 bytes, 16-byte aligned).  Arithmetic is always on the values widened to float32.
#define DFLOW_DESC_PITCH_H 72
typedef _Float16 dflow_h8 __attribute__((ext_vector_type(8)));
template <typename T> struct DescPitch { static constexpr int value = DFLOW_DESC; };
template <> struct DescPitch<_Float16> { static constexpr int value = DFLOW_DESC_PITCH_H; };
static inline bool descr_f16(const dflow_params *p) { return (p->flags & DFLOW_FLAG_DESCR_F16) != 0; }

// the descriptor of pixel pix into registers
template <typename T> __device__ static inline void desc_load_row(float (&q)[DFLOW_DESC], const T *__restrict__ base, size_t pix)
{
    if constexpr (sizeof(T) == 4) {
        const float4 *s = reinterpret_cast<const float4 *>(base + pix * DFLOW_DESC);
#pragma unroll
        for (int k = 0; k < DFLOW_DESC / 4; k++) { float4 v = s[k]; q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w; }
    } else {
        const dflow_h8 *s = reinterpret_cast<const dflow_h8 *>(base + pix * DFLOW_DESC_PITCH_H);
#pragma unroll
        for (int k = 0; k < DFLOW_DESC_PITCH_H / 8; k++) {
            const dflow_h8 v = s[k];
#pragma unroll
            for (int j = 0; j < 8; j++) if (8 * k + j < DFLOW_DESC) q[8 * k + j] = (float)v[j];
        }
    }
}

// numpy float32 pairwise-sum order for 68 contiguous values (np.sum at daisy i flann.py:179,229)
__device__ static inline float np_pairwise_sum68(const float *a)
{
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = a[j];
#pragma unroll
    for (int i = 8; i < 64; i += 8)
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = __fadd_rn(r[j], a[i + j]);
    float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                          __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
#pragma unroll
    for (int i = 64; i < DFLOW_DESC; i++) res = __fadd_rn(res, a[i]);
    return res;
}

// The canonical pair arithmetic of the kNN stage, for query q and candidate c (as 17 float4): l2 = squared L2 of q - c as a
// sequential fmaf chain over k = 0..67; l1() = sum_k |q[k]-c[k]| in numpy's float32 pairwise order (8 running sums, a tree,
// then the 4-element tail; l1_cost_np), summed where it is used so that a kernel that needs it only for some pairs pays
// the tree only for those.  Every kernel that must agree bit for bit with the brute-force search uses it.
struct PairDist {
    float l2, rs[8], tl[4];
    __device__ float l1() const
    {
        float l1 = ((rs[0] + rs[1]) + (rs[2] + rs[3])) + ((rs[4] + rs[5]) + (rs[6] + rs[7]));
        l1 = l1 + tl[0]; l1 = l1 + tl[1]; l1 = l1 + tl[2]; l1 = l1 + tl[3];
        return l1;
    }
};
typedef float dflow_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ static PairDist pair_dist(const float (&q)[DFLOW_DESC], const float4 (&c)[DFLOW_DESC / 4])
{
    PairDist d;
    d.l2 = 0.0f;
#pragma unroll
    for (int k = 0; k < DFLOW_DESC / 4; k++) {
        const float4 v = c[k];
        // two differences per instruction (v_pk_add_f32 with negated operand: the same IEEE subtraction per half)
        const dflow_f2 ea = (dflow_f2){q[4 * k], q[4 * k + 1]} - (dflow_f2){v.x, v.y};
        const dflow_f2 eb = (dflow_f2){q[4 * k + 2], q[4 * k + 3]} - (dflow_f2){v.z, v.w};
        const float e[4] = {ea.x, ea.y, eb.x, eb.y};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            d.l2 = __fmaf_rn(e[i], e[i], d.l2);
            const int j = (4 * k + i) & 7;
            if (k < 2) d.rs[j] = fabsf(e[i]);
            else if (k < 16) d.rs[j] = d.rs[j] + fabsf(e[i]);
            else d.tl[i] = fabsf(e[i]);
        }
    }
    return d;
}

// sum_k |a[k]-b[k]| in numpy's float32 pairwise order (np.sum(np.absolute(..)), daisy i flann.py:179-180).
// Cold path (5 winners per cell): both rows are re-read from memory in a rolled loop so that the hot search
// loop keeps its register budget.
__device__ __noinline__ static float l1_cost_np(const float *__restrict__ a, const float *__restrict__ b)
{
    const float4 *a4 = reinterpret_cast<const float4 *>(a), *b4 = reinterpret_cast<const float4 *>(b);
    float r[8];
    {
        float4 u0 = a4[0], u1 = a4[1], v0 = b4[0], v1 = b4[1];
        r[0] = fabsf(u0.x - v0.x); r[1] = fabsf(u0.y - v0.y); r[2] = fabsf(u0.z - v0.z); r[3] = fabsf(u0.w - v0.w);
        r[4] = fabsf(u1.x - v1.x); r[5] = fabsf(u1.y - v1.y); r[6] = fabsf(u1.z - v1.z); r[7] = fabsf(u1.w - v1.w);
    }
#pragma unroll 1
    for (int i = 2; i < 16; i += 2) {
        float4 u0 = a4[i], u1 = a4[i + 1], v0 = b4[i], v1 = b4[i + 1];
        r[0] = r[0] + fabsf(u0.x - v0.x); r[1] = r[1] + fabsf(u0.y - v0.y); r[2] = r[2] + fabsf(u0.z - v0.z); r[3] = r[3] + fabsf(u0.w - v0.w);
        r[4] = r[4] + fabsf(u1.x - v1.x); r[5] = r[5] + fabsf(u1.y - v1.y); r[6] = r[6] + fabsf(u1.z - v1.z); r[7] = r[7] + fabsf(u1.w - v1.w);
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    float4 u = a4[16], v = b4[16];
    res = res + fabsf(u.x - v.x); res = res + fabsf(u.y - v.y); res = res + fabsf(u.z - v.z); res = res + fabsf(u.w - v.w);
    return res;
}

// the same for binary16 rows (both rows widened to float32 first; same summation order)
__device__ __noinline__ static float l1_cost_np(const _Float16 *__restrict__ a, const _Float16 *__restrict__ b)
{
    float u[DFLOW_DESC], v[DFLOW_DESC], r[8];
    desc_load_row(u, a, 0); desc_load_row(v, b, 0);
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = fabsf(u[j] - v[j]);
#pragma unroll
    for (int i = 8; i < 64; i += 8)
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = r[j] + fabsf(u[i + j] - v[i + j]);
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int i = 64; i < DFLOW_DESC; i++) res = res + fabsf(u[i] - v[i]);
    return res;
}

// calls f(tag) once, with the descriptor storage of p: tag::T is float or _Float16, tag::F16 the matching bool
template <typename T_> struct DescrType { using T = T_; static constexpr bool F16 = sizeof(T_) == 2; };
template <typename F> static inline void with_descr_type(const dflow_params *p, F &&f)
{
    if (descr_f16(p)) f(DescrType<_Float16>()); else f(DescrType<float>());
}

// error plumbing (abi.hip)
int dflow_set_error(int code, const char *fmt, ...);
int dflow_check_launch(const char *what);
int dflow_check_params(const dflow_params *p);
// a HIP runtime call: on failure, return DFLOW_EHIP from the enclosing function with the call and HIP's message
#define DFLOW_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return dflow_set_error(DFLOW_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

// A stage's workspace layout: regions handed out in order, each on a 256-byte boundary of the caller's (256-byte aligned)
// buffer; bytes = their total, every region rounded up to 256 bytes.  Given nullptr as the base it only counts, so that
// one function both sizes and carves a stage's part of the workspace.
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct WsCarver {
    uintptr_t base;
    size_t bytes = 0;
    explicit WsCarver(void *ws) : base((uintptr_t)ws) {}
    template <typename T> T *take(size_t count) { T *r = (T *)(base + bytes); bytes = align256(bytes + count * sizeof(T)); return r; }
};
// spare bytes at the end of the whole workspace (dflow_workspace_bytes), beyond the largest stage
#define DFLOW_WS_SLACK 256

// stage launchers (one per .hip file)
int launch_daisy(const dflow_params *p, const uint8_t *bgr, void *descr, void *ws, hipStream_t s);
size_t daisy_ws_bytes(const dflow_params *p);
// both images of a pair through one set of launches (a second set of scratch planes: daisy_pair_ws_bytes)
int launch_daisy_pair(const dflow_params *p, const uint8_t *bgr1, const uint8_t *bgr2, void *descr1, void *descr2, void *ws,
                      hipStream_t s);
size_t daisy_pair_ws_bytes(const dflow_params *p);
// d1, d2: float32 (H,W,68) or, with DFLOW_FLAG_DESCR_F16, binary16 (H,W,72)
int launch_knn(const dflow_params *p, const void *d1, const void *d2, uint32_t *proposals, float *lcosts,
               int32_t *nprop, int32_t *bestlabels, hipStream_t s);
#define KNN_MFMA_EVENTS 7
// the brute-force search for the lists the MFMA screen could not finish (ovf_list[0 .. *ovf_count)), knn.hip
int launch_knn_fix(const dflow_params *p, const void *d1, const void *d2, uint32_t *proposals, float *lcosts,
                   const int *ovf_count, const int4 *ovf_list, int ovf_cap, const int *flags, hipStream_t s);
int launch_knn_mfma(const dflow_params *p, const void *d1, const void *d2, uint32_t *proposals, float *lcosts,
                    int32_t *nprop, int32_t *bestlabels, void *ws, hipStream_t s, hipEvent_t *ev = nullptr);
double knn_mfma_issued(const dflow_params *p);
int knn_mfma_stats(const dflow_params *p, void *ws, hipStream_t s, int64_t *h_out);
size_t knn_mfma_ws_bytes(const dflow_params *p);
bool knn_mfma_supported(const dflow_params *p);
int launch_neighbour(const dflow_params *p, const void *d1, const void *d2, uint32_t *proposals, float *lcosts,
                     int32_t *nprop, const int32_t *bestlabels, void *ws, hipStream_t s);
size_t neighbour_ws_bytes(const dflow_params *p);
int launch_bcd_phase(const dflow_params *p, const int32_t *nprop, int32_t *bestlabels, int phase, void *ws, hipStream_t s);
int launch_bcd_phase_batch(const dflow_params *p, int npass, const int32_t *const *nprop, int32_t *const *bestlabels, int phase,
                           void *const *ws, hipStream_t s);
size_t bcd_ws_bytes(const dflow_params *p);
int launch_bcd_prepare(const dflow_params *p, const uint32_t *proposals, const float *lcosts, const int32_t *nprop, void *ws,
                       hipStream_t s);
// bcd_stats.hip: energy and label-change statistics of npass labellings (arguments validated by the caller); prev, prev_out
// and their entries may be NULL; ws holds npass regions of bcd_stats_ws_bytes
size_t bcd_stats_ws_bytes(int H, int W);
int launch_bcd_stats_batch(const dflow_params *p, int npass, const uint32_t *const *proposals, const float *const *lcosts,
                           const int32_t *const *nprop, const int32_t *const *labels, const int32_t *const *prev,
                           int32_t *const *prev_out, struct dflow_bcd_stats *stats, void *ws, hipStream_t s);
int launch_labels_to_flow(const dflow_params *p, const uint32_t *proposals, const int32_t *bestlabels, float *flow,
                          hipStream_t s);
int launch_pack_compat(const dflow_params *p, const uint32_t *proposals, const int32_t *nprop, uint8_t *packed, hipStream_t s);
int host_remove_small_segments(float *flow, int A, int B, float tresh, int min_segment_size);
int launch_fb_consistency(const dflow_params *p, const float *fwd, const float *bwd, float tresh, float *sparse,
                          hipStream_t s);
// edges.hip: Canny edge map of a (H,W,3) BGR image; thresholds already swapped and floored
size_t canny_ws_bytes(int H, int W);
int launch_canny(int H, int W, const uint8_t *bgr, int lo, int hi, uint8_t *edges, float *ivice, void *ws, hipStream_t s);
// pb_edges.hip: Pb-style soft edge strength of a (H,W,3) BGR image (arguments validated by the caller); orient may be NULL
size_t pb_ws_bytes(int H, int W);
int launch_pb(int H, int W, const uint8_t *bgr, int radius, float *strength, float *orient, void *ws, hipStream_t s);
// epic.hip: edge-aware interpolation of a sparse flow field (arguments validated by the caller)
size_t epic_ws_bytes(int H, int W);
int launch_epic(int H, int W, const float *sparse, const float *edges, int nn, double k, int method, float *flow,
                int32_t *seed_of, uint32_t *dist, int32_t *lists, uint64_t *list_g, void *ws, hipStream_t s);
int epic_last_stats(int32_t *rounds, float *stage_ms);
// variational.hip: variational refinement of a dense flow (arguments validated by the caller)
#define VAR_MAX_RADIUS 15            // ceil(3 * 5): sigma <= 5
// the taps of a Gaussian of radius r = ceil(3 sigma), t[0 .. 2r], normalised in double and rounded to float32
struct VarTaps { float t[2 * VAR_MAX_RADIUS + 1]; int r; };
VarTaps var_taps(float sigma);
// its separable Gaussian of one (H,W,3) uint8 image into three float planes (var_smooth_kernel)
int launch_var_smooth(int H, int W, const uint8_t *bgr, float sigma, float *o0, float *o1, float *o2, hipStream_t s);
size_t var_ws_bytes(int H, int W);
int launch_var(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *flow_in, const dflow_var_params *p,
               float *flow_out, void *ws, hipStream_t s);
// epic_prefilter.hip: EpicFlow's match pre-filter (arguments validated by the caller)
size_t epic_prefilter_ws_bytes(int H, int W);
int launch_epic_prefilter(int H, int W, const uint8_t *bgr, const float *sparse_in, const float *edges, double saliency_th,
                          int pref_nn, double pref_th, double k, float *sparse_out, uint8_t *reason, float *saliency,
                          float *estimate, void *ws, hipStream_t s);
int epic_prefilter_last_stats(int32_t *counts, float *stage_ms);
// flow_eval.hip: error statistics, error plane and error picture of a flow against the ground truth (arguments validated by
// the caller); err and bgr may be NULL
size_t eval_ws_bytes(int H, int W);
int launch_flow_eval(int H, int W, const float *test, int layout, const float *gt, float abs_thresh, uint32_t flags,
                     dflow_eval_stats *stats, float *err, uint8_t *bgr, void *ws, hipStream_t s);
// flow_picture.hip: the colour-wheel picture of a flow, and the warp of the second image onto the first with its photometric
// error (arguments validated by the caller); maxrad, warped, err and err_bgr may be NULL
size_t flow_color_ws_bytes(int H, int W);
int launch_flow_color(int H, int W, const float *flow, int layout, float max_flow, uint8_t *bgr, float *maxrad, void *ws,
                      hipStream_t s);
size_t warp_eval_ws_bytes(int H, int W);
int launch_warp_eval(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *flow, int layout, float err_thresh,
                     float err_max, uint32_t flags, dflow_photo_stats *stats, uint8_t *warped, float *err, uint8_t *err_bgr,
                     void *ws, hipStream_t s);
// prior.hip: labels from a prior flow appended to the state, and a flow carried to the pixels it points at (arguments
// validated by the caller); counts may be NULL
int launch_prior(const dflow_params *p, const void *d1, const void *d2, const float *prior, int layout, int stride, uint32_t flags,
                 uint32_t *proposals, float *lcosts, int32_t *nprop, int32_t *bestlabels, int32_t *counts, hipStream_t s);
size_t flow_advance_ws_bytes(int H, int W);
int launch_flow_advance(int H, int W, const float *flow, int layout, uint32_t flags, float *out, int32_t *counts, void *ws,
                        hipStream_t s);
// pyramid.hip: one level of an image pyramid (in2 / out2 both NULL: one image) and a coarse flow doubled onto the next finer
// grid (arguments validated by the caller); counts may be NULL
int launch_pyr_down(int H, int W, const uint8_t *in1, const uint8_t *in2, uint8_t *out1, uint8_t *out2, hipStream_t s);
int launch_flow_upsample(int H, int W, const float *coarse, int layout, float *out, int32_t *counts, hipStream_t s);
// consistency.hip: the forward/backward check in image coordinates, one direction or (out_bwd given) both in one launch
// (arguments validated by the caller); err_* and counts may be NULL
int launch_flow_consistency(int H, int W, const float *fwd, int layout_fwd, const float *bwd, int layout_bwd, float thresh,
                            uint32_t flags, float *out_fwd, float *out_bwd, float *err_fwd, float *err_bwd, int32_t *counts,
                            hipStream_t s);
// segments.hip: the small-segment filter of a sparse flow field, four launches whatever the field holds (arguments validated by
// the caller); segment, size and counts may be NULL
size_t segment_filter_ws_bytes(int H, int W);
int launch_segment_filter(int H, int W, const float *flow, int layout, float thresh, int min_size, uint32_t flags, float *out,
                          int32_t *segment, int32_t *size, int32_t *counts, void *ws, hipStream_t s);
// frame_interp.hip: the frame at time t between two frames, 3 + fill_rounds launches whatever the fields hold (arguments
// validated by the caller); bwd, source and counts may be NULL, motion_tmp too when fill_rounds is 0
int launch_frame_interp(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *fwd, int layout_fwd, const float *bwd,
                        int layout_bwd, float t, int fill_rounds, float occl_thresh, uint8_t *out, uint64_t *keys, float *motion,
                        float *motion_tmp, uint8_t *source, int32_t *counts, hipStream_t s);
// flow_wmedian.hip: the weighted median filter of a flow field, one launch (arguments validated by the caller); bgr and wcolor
// are both NULL (unguided) or both given, wspace and counts may be NULL
int launch_flow_wmedian(int H, int W, const float *flow, int layout, const uint8_t *bgr, int radius, const uint8_t *wspace,
                        const uint8_t *wcolor, float reject_thresh, uint32_t flags, float *out, int32_t *counts, hipStream_t s);
// motion_fit.hip: the robust fit of an affine map or a homography to a flow field, 3 + 4 (lo_rounds + 1) + 4 polish launches
// whatever the field holds (arguments validated by the caller); exclude, cls, model_flow, residual and counts may be NULL
int launch_motion_fit(int H, int W, const float *flow, int layout, const uint8_t *exclude, int model, float thresh, int n_hyp,
                      int lo_rounds, int polish, int step, uint64_t seed, float *d_model, float *models, int32_t *hyp_counts,
                      int64_t *state, uint8_t *cls, float *model_flow, float *residual, int32_t *counts, hipStream_t s);
// epipolar.hip: the robust fit of a fundamental matrix to a flow field, 3 + 4 (lo_rounds + 1) launches whatever the field holds
// (arguments validated by the caller); exclude, cls, residual and counts may be NULL
int launch_epipolar_fit(int H, int W, const float *flow, int layout, const uint8_t *exclude, float thresh, int n_hyp, int lo_rounds,
                        int step, uint64_t seed, float *d_model, float *models, int32_t *hyp_counts, int64_t *state, uint8_t *cls,
                        float *residual, int32_t *counts, hipStream_t s);
// label_conf.hip: the per-pixel margin of a labelling and the score gate of a flow field, one launch each (arguments validated by
// the caller); margin, alt, sparse and counts may be NULL (not all four), the gate's counts too
int launch_label_confidence(const dflow_params *p, const uint32_t *proposals, const float *lcosts, const int32_t *nprop,
                            const int32_t *labels, int mode, int min_sep, float thresh, float *margin, int32_t *alt, float *sparse,
                            int32_t *counts, hipStream_t s);
int launch_flow_gate(int H, int W, const float *flow, int layout, const float *score, float lo, float hi, float *out, int32_t *counts,
                     hipStream_t s);
