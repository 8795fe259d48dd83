// C-ABI entry points of libdflow.so (declared in include/dflow.h): parameter validation, workspace
// accounting and dispatch to the per-stage launchers.  No torch types, no allocation, no synchronisation.
//
// A gate is a sequence of the checks defined below dflow_check_launch, each called with __func__ and returning DFLOW_OK or what
// dflow_set_error returned: check_frame_size, check_layout, check_flags, check_finite_ge0 / check_finite_gt0, check_int_range,
// check_not_nan, check_ordered, check_any_given, CHECK_PTR, check_aligned (CHECK_ALIGNED; check_aligned_entry for one entry of a batch form's arrays), check_distinct (outputs against inputs and each other) and, last but where d_ws has always been among
// the aligned pointers, CHECK_WS; FRAME_WS_BYTES defines an image-plane stage's size function.  A new entry point's gate is
// assembled from these, and its refusals are added to tests/test_abi_refusals.py, which pins every status, text and the order.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "dflow_common.h"
#include "../../include/dflow_klt.h"

// tracks.hip: a track set carried one frame on, new tracks in the uncovered cells, the sparse flow between two snapshots (arguments
// validated by the caller); bwd, err, mask and counts may be NULL.  Declared here: dflow_common.h is part of every device build.
int launch_track_advance(int H, int W, const float *fwd, int layout_fwd, const float *bwd, int layout_bwd, int cap, const float *pos_in,
                         const int32_t *state_in, float rel, float abs_tol, float *pos_out, int32_t *state_out, float *err,
                         int32_t *counts, hipStream_t s);
int launch_track_seed(int H, int W, int cap, int step, int frame, const uint8_t *mask, float *pos, int32_t *state, int32_t *birth,
                      int32_t *d_n, int32_t *scan, int32_t *counts, hipStream_t s);
int launch_track_flow(int H, int W, int cap, const float *pos_a, const int32_t *state_a, const float *pos_b, const int32_t *state_b,
                      int32_t *owner, float *out, int32_t *counts, hipStream_t s);

// superpixels.hip: the integer SLIC with connected, compactly numbered segments, 8 + 2 iters launches, and the per-segment affine
// fit, 2 rounds + 1 launches, whatever the planes hold (arguments validated by the caller); slic, out, cls and counts may be NULL
int launch_superpixels(int H, int W, const uint8_t *bgr, int step, int compactness, int iters, int min_size, int32_t *label,
                       int32_t *centers, int32_t *slic, int32_t *counts, int32_t *sums, int32_t *comp, int32_t *size, int32_t *fin,
                       int32_t *scan, hipStream_t s);
int launch_segment_fit(int H, int W, const float *flow, int layout, const int32_t *label, int n_seg, float thresh, int rounds,
                       float *models, int32_t *seg_counts, float *out, uint8_t *cls, int32_t *counts, int64_t *acc, hipStream_t s);

// two_view.hip: the pose, depth, class and reprojection error of a flow field under its fundamental matrix, 4 launches whatever the
// planes hold (arguments validated by the caller); part, depth, cls, err and counts may be NULL
int launch_two_view(int H, int W, const float *flow, int layout, const float *model, const uint8_t *part, double fx, double fy, double cx,
                    double cy, int step, double *pose, int64_t *state, float *depth, uint8_t *cls, float *err, int32_t *counts,
                    hipStream_t s);

// klt.hip: the grey pyramid, the corners of its level 0 and pyramidal Lucas-Kanade over a track set (include/dflow_klt.h; arguments
// validated by the caller); the set of launch_corners, and err, back and counts may be NULL
size_t klt_pyramid_bytes(int H, int W, int levels);
int launch_klt_pyramid(int H, int W, int levels, const uint8_t *bgr, uint8_t *pyr, hipStream_t s);
int launch_corners(int H, int W, const uint8_t *grey, int rc, int min_dist, int border, float quality, float min_response, int cap,
                   const float *pos, const int32_t *state, const int32_t *d_n, float *resp, uint8_t *mask, uint8_t *occ, uint32_t *rmax,
                   int32_t *counts, hipStream_t s);
int launch_klt_track(int H, int W, int levels, const uint8_t *pyr1, const uint8_t *pyr2, int cap, const float *pos_in,
                     const int32_t *state_in, int r, int iters, float eps, float min_eig, float max_err, float fb, float *pos_out,
                     int32_t *state_out, float *err, float *back, int32_t *counts, hipStream_t s);

static thread_local char g_err[512] = "";

int dflow_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int dflow_check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dflow_set_error(DFLOW_EHIP, "%s: %s", what, hipGetErrorString(e));
    return DFLOW_OK;
}

// The checks the gates are made of.  `fn` is the entry point's __func__: the message starts with it.
static int check_frame_size(const char *fn, int32_t h, int32_t w)
{
    return h < 1 || w < 1 || h > 8192 || w > 8192 ? dflow_set_error(DFLOW_EINVAL, "%s: image size %dx%d outside [1,8192]", fn, w, h) : DFLOW_OK;
}

// `name` is what the message calls the argument: layout, test_layout, layout_fwd, ...
static int check_layout(const char *fn, const char *name, int32_t layout)
{
    return layout != DFLOW_EVAL_UVV && layout != DFLOW_EVAL_DYDX ? dflow_set_error(DFLOW_EINVAL, "%s: unknown %s %d", fn, name, layout) : DFLOW_OK;
}

static int check_flags(const char *fn, uint32_t flags, uint32_t known)
{
    return flags & ~known ? dflow_set_error(DFLOW_EINVAL, "%s: unknown flags 0x%x", fn, flags) : DFLOW_OK;
}

// a value outside what its argument takes: `must` says what that is, `note` ends the message where a value has a meaning of its own
static int refuse_value(const char *fn, const char *name, double v, const char *must, const char *note = "")
{
    return dflow_set_error(DFLOW_EINVAL, "%s: %s=%g must be %s%s", fn, name, v, must, note);
}

static int check_finite_ge0(const char *fn, const char *name, double v, const char *note = "")
{
    return !isfinite(v) || v < 0.0 ? refuse_value(fn, name, v, "finite and >= 0", note) : DFLOW_OK;
}

static int check_finite_gt0(const char *fn, const char *name, double v)
{
    return !isfinite(v) || !(v > 0.0) ? refuse_value(fn, name, v, "finite and > 0") : DFLOW_OK;
}

// a value that may be infinite but not NaN
static int check_not_nan(const char *fn, const char *name, double v)
{
    return isnan(v) ? refuse_value(fn, name, v, "a number") : DFLOW_OK;
}

// the two ends of a closed range
static int check_ordered(const char *fn, const char *lo_name, double lo, const char *hi_name, double hi)
{
    char must[64];
    snprintf(must, sizeof(must), "<= %s=%g", hi_name, hi);
    return lo > hi ? refuse_value(fn, lo_name, lo, must) : DFLOW_OK;
}

// fn may be NULL: the fields of dflow_params, and phase and npass of the BCD entry points, are reported without a prefix
static int check_int_range(const char *fn, const char *name, int v, int lo, int hi)
{
    if (v < lo || v > hi) return dflow_set_error(DFLOW_EINVAL, "%s%s%s=%d outside [%d,%d]", fn ? fn : "", fn ? ": " : "", name, v, lo, hi);
    return DFLOW_OK;
}

// a required pointer, or a group of optional outputs of which a call needs at least one (`names` lists them for the message)
static int refuse_null(const char *fn, const char *name) { return dflow_set_error(DFLOW_EINVAL, "%s: %s is NULL", fn, name); }
static int check_any_given(const char *fn, const char *names, std::initializer_list<const void *> ptrs)
{
    for (const void *q : ptrs)
        if (q) return DFLOW_OK;
    return refuse_null(fn, names);
}

// a pointer the kernels move several elements of at a time; NULL (an optional output left out) passes
struct AlignedPtr { const char *name; const void *p; uintptr_t align; };
static int check_aligned(const char *fn, std::initializer_list<AlignedPtr> ptrs)
{
    for (const AlignedPtr &q : ptrs)
        if ((uintptr_t)q.p % q.align) return dflow_set_error(DFLOW_EINVAL, "%s: %s is not %d-byte aligned", fn, q.name, (int)q.align);
    return DFLOW_OK;
}

// entry i of a batch form's host array of device pointers: the message names it name[i]
static int check_aligned_entry(const char *fn, const char *name, int i, const void *p, uintptr_t align)
{
    char entry[48];
    snprintf(entry, sizeof(entry), "%s[%d]", name, i);
    return check_aligned(fn, {{entry, p, align}});
}

// The boundaries of the data planes (include/dflow.h, "Alignment of data planes"): the widest access a kernel makes to the plane,
// one number per plane wherever it is passed.  Descriptor rows move as float4 / 8 x binary16 and through 16-byte LDS-DMA
// (dflow_common.h desc_load_row, knn.hip, row_stage.h); label and cost rows are read 16 bytes at a time (prior.hip,
// label_conf.hip); [dy,dx] flows move as float2 (post.hip, variational.hip); the EPIC distance lists hold uint64.
#define ALIGN_DESCR 16
#define ALIGN_LABEL_ROWS 16
#define ALIGN_FLOW2 8
#define ALIGN_WORD 4
// the state of a pass: the planes every main-path stage and the statistics share
#define STATE_ROWS_ALIGNED {"d_proposals", d_proposals, ALIGN_LABEL_ROWS}, {"d_lcosts", d_lcosts, ALIGN_LABEL_ROWS}
#define STATE_COUNTS_ALIGNED {"d_nprop", d_nprop, ALIGN_WORD}, {"d_bestlabels", d_bestlabels, ALIGN_WORD}
#define DESCR_PAIR_ALIGNED {"d_descr1", d_descr1, ALIGN_DESCR}, {"d_descr2", d_descr2, ALIGN_DESCR}
#define CHECK_ALIGNED(...) do { int rc_al_ = check_aligned(__func__, {__VA_ARGS__}); if (rc_al_) return rc_al_; } while (0)

// no output that is given is the plane of an input or of an output listed before it
struct NamedPlane { const char *name; const void *p; };
static int check_distinct(const char *fn, std::initializer_list<NamedPlane> ins, std::initializer_list<NamedPlane> outs)
{
    for (const NamedPlane *o = outs.begin(); o != outs.end(); o++) {
        const NamedPlane *same = nullptr;
        for (const NamedPlane &q : ins)
            if (!same && q.p == o->p) same = &q;
        for (const NamedPlane *q = outs.begin(); q != o; q++)
            if (!same && q->p == o->p) same = q;
        if (o->p && same) return dflow_set_error(DFLOW_EINVAL, "%s: %s is the same plane as %s", fn, o->name, same->name);
    }
    return DFLOW_OK;
}

static int check_ws_size(const char *fn, const void *d_ws, size_t ws_bytes, size_t need)
{
    return !d_ws || ws_bytes < need ? dflow_set_error(DFLOW_ENOSPC, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need) : DFLOW_OK;
}

// The size of d_ws, then the boundary its stage needs: the widest access a kernel of the stage makes to a region WsCarver hands out
// (regions start at multiples of 256 bytes from d_ws).  include/dflow.h, Conventions, lists them: 16 for the main-path stages, 8
// where a region holds doubles or uint64 (bcd_stats.hip, flow_eval.hip, flow_picture.hip's warp, epic.h), 4 for int32 / uint32 /
// float regions (edges.hip, variational.hip, flow_picture.hip's colour, prior.hip, segments.hip), 2 for pb_edges.hip's uint16
// plane.  A NULL or short workspace is DFLOW_ENOSPC whatever its alignment, as it always was; the entry points that have
// always named d_ws among their aligned pointers (bcd_stats, flow_advance, segment_filter) check it there, before its size.
static int check_ws(const char *fn, const void *d_ws, size_t ws_bytes, uintptr_t align, size_t need)
{
    int rc = check_ws_size(fn, d_ws, ws_bytes, need);
    return rc ? rc : check_aligned(fn, {{"d_ws", d_ws, align}});
}
#define CHECK_PTR(x) do { if (!(x)) return refuse_null(__func__, #x); } while (0)
#define CHECK_WS(align, need) do { int rc_ws_ = check_ws(__func__, d_ws, ws_bytes, (align), (need)); if (rc_ws_) return rc_ws_; } while (0)
// the main-path stages carve float4, int4 and uint4 regions (daisy.hip, knn_mfma.hip, bcd.hip)
#define WS_ALIGN_MAIN 16
// the size function of an image-plane stage: 0, and the message, outside the frame sizes the stage takes
#define FRAME_WS_BYTES(entry, stage_bytes) \
    size_t entry(int32_t h, int32_t w) { return check_frame_size(#entry, h, w) == DFLOW_OK ? stage_bytes(h, w) : 0; }

int dflow_check_params(const dflow_params *p)
{
    if (!p) return dflow_set_error(DFLOW_EINVAL, "params is NULL");
    if (p->pich < 8 || p->picw < 8 || p->pich > 8192 || p->picw > 8192)
        return dflow_set_error(DFLOW_EINVAL, "image size %dx%d outside [8,8192]", p->picw, p->pich);
    if (p->cellh < 1 || p->cellw < 1 || p->cellh > p->pich || p->cellw > p->picw)
        return dflow_set_error(DFLOW_EINVAL, "cell size %dx%d does not fit the image", p->cellw, p->cellh);
    if (p->knn != 5) return dflow_set_error(DFLOW_EINVAL, "knn=%d unsupported (kernels are built for 5)", p->knn);
    if (p->cellh * p->cellw < p->knn) return dflow_set_error(DFLOW_EINVAL, "cells hold fewer than knn points");
    int rc;
    if ((rc = check_int_range(NULL, "window", p->window, 0, 2))) return rc;
    if ((rc = check_int_range(NULL, "ngauss", p->ngauss, 0, 64))) return rc;
    int maxknn = (2 * p->window + 1) * (2 * p->window + 1) * p->knn;
    if (p->maxnprop < maxknn + p->ngauss || p->maxnprop > DFLOW_MAX_LABELS)
        return dflow_set_error(DFLOW_EINVAL, "maxnprop=%d must be in [%d,%d]", p->maxnprop, maxknn + p->ngauss, DFLOW_MAX_LABELS);
    if (p->label_pitch < p->maxnprop || p->label_pitch % 16 != 0 || p->label_pitch > DFLOW_MAX_LABELS)
        return dflow_set_error(DFLOW_EINVAL, "label_pitch=%d must be a multiple of 16 in [maxnprop,%d]", p->label_pitch, DFLOW_MAX_LABELS);
    // pair costs below tpsi travel as 3-bit fields in the BCD label records (bcd.hip)
    if ((rc = check_int_range(NULL, "tpsi", p->tpsi, 1, 8))) return rc;
    // the chain kernel picks the fallback predecessor as an unsigned minimum over the bit patterns of tpsi + dp (bcd.hip),
    // which orders like the doubles only while they are >= 0; the reference starts that minimum (and the end label's) at
    // 800000 (python bcd.py:152-157,231): dp stays in [0, 800000) for every chain when the last rule holds (include/dflow.h)
    if (!isfinite(p->lamda) || p->lamda < 0.0) return dflow_set_error(DFLOW_EINVAL, "lamda=%g must be finite and >= 0", p->lamda);
    if (!isfinite(p->tphi) || p->tphi < 0.0f) return dflow_set_error(DFLOW_EINVAL, "tphi=%g must be finite and >= 0", (double)p->tphi);
    {
        const double n = (double)(p->pich > p->picw ? p->pich : p->picw);
        const double dpmax = n * (3.0 * (double)p->tpsi + p->lamda * (double)p->tphi);
        if (!(dpmax < DFLOW_DP_SENTINEL))
            return dflow_set_error(DFLOW_EINVAL, "max(pich,picw)*(3*tpsi+lamda*tphi)=%.17g (lamda=%g, tphi=%g, tpsi=%d) must be below %g",
                                   dpmax, p->lamda, (double)p->tphi, p->tpsi, DFLOW_DP_SENTINEL);
    }
    if (!(p->sigma > 0.0f) || p->sigma > 8.0f) return dflow_set_error(DFLOW_EINVAL, "sigma=%g outside (0,8]", (double)p->sigma);
    if (p->max_attempts < p->ngauss) return dflow_set_error(DFLOW_EINVAL, "max_attempts < ngauss");
    if (p->flags & ~(DFLOW_FLAG_KNN_EXACT | DFLOW_FLAG_DESCR_F16)) return dflow_set_error(DFLOW_EINVAL, "unknown flags 0x%x", (unsigned)p->flags);
    return DFLOW_OK;
}

extern "C" {

int dflow_version(void) { return DFLOW_VERSION; }

const char *dflow_last_error(void) { return g_err; }

void dflow_default_params(dflow_params *p, int32_t pich, int32_t picw, int32_t cellh, int32_t cellw)
{
    memset(p, 0, sizeof(*p));
    p->pich = pich; p->picw = picw; p->cellh = cellh; p->cellw = cellw;
    p->maxnprop = 150; p->knn = 5; p->window = 2; p->ngauss = 25; p->tpsi = 8; p->max_attempts = 1 << 16;
    p->tphi = 2.5f; p->sigma = 8.0f; p->lamda = 0.05; p->seed = 0; p->label_pitch = 160;
}

size_t dflow_workspace_bytes(const dflow_params *p)
{
    if (dflow_check_params(p) != DFLOW_OK) return 0;
    size_t m = daisy_pair_ws_bytes(p);
    for (size_t b : {bcd_ws_bytes(p), neighbour_ws_bytes(p), knn_mfma_supported(p) ? knn_mfma_ws_bytes(p) : (size_t)0})
        if (b > m) m = b;
    return m + DFLOW_WS_SLACK;
}

int dflow_daisy(const dflow_params *p, const uint8_t *d_bgr, void *d_descr, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_bgr); CHECK_PTR(d_descr);
    CHECK_ALIGNED({"d_descr", d_descr, ALIGN_DESCR});
    CHECK_WS(WS_ALIGN_MAIN, daisy_ws_bytes(p));
    return launch_daisy(p, d_bgr, d_descr, d_ws, (hipStream_t)stream);
}

int dflow_daisy_pair(const dflow_params *p, const uint8_t *d_bgr1, const uint8_t *d_bgr2, void *d_descr1, void *d_descr2,
                     void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_bgr1); CHECK_PTR(d_bgr2); CHECK_PTR(d_descr1); CHECK_PTR(d_descr2);
    CHECK_ALIGNED(DESCR_PAIR_ALIGNED);
    CHECK_WS(WS_ALIGN_MAIN, daisy_pair_ws_bytes(p));
    // the two images run side by side: the outputs must be two planes
    if (d_descr1 == d_descr2) return dflow_set_error(DFLOW_EINVAL, "%s: d_descr1 and d_descr2 are the same plane", __func__);
    return launch_daisy_pair(p, d_bgr1, d_bgr2, d_descr1, d_descr2, d_ws, (hipStream_t)stream);
}

// DFLOW_FLAG_KNN_EXACT selects the brute-force VALU kernel (same results; used to cross-check the MFMA path)
static bool knn_is_screened(const dflow_params *p) { return !(p->flags & DFLOW_FLAG_KNN_EXACT) && knn_mfma_supported(p); }

// The end of the gate of whatever needs the MFMA-screened search: that it runs for *p, then its workspace.
static int knn_check_screened(const char *fn, const dflow_params *p, const void *d_ws, size_t ws_bytes)
{
    if (!knn_is_screened(p)) return dflow_set_error(DFLOW_EINVAL, "%s: the MFMA-screened search does not run for these parameters", fn);
    return check_ws(fn, d_ws, ws_bytes, WS_ALIGN_MAIN, knn_mfma_ws_bytes(p));
}

int dflow_knn_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2, uint32_t *d_proposals,
                        float *d_lcosts, int32_t *d_nprop, int32_t *d_bestlabels, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_descr1); CHECK_PTR(d_descr2); CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels);
    CHECK_ALIGNED(DESCR_PAIR_ALIGNED, STATE_ROWS_ALIGNED, STATE_COUNTS_ALIGNED);
    if (!knn_is_screened(p)) return launch_knn(p, d_descr1, d_descr2, d_proposals, d_lcosts, d_nprop, d_bestlabels, (hipStream_t)stream);
    if ((rc = knn_check_screened(__func__, p, d_ws, ws_bytes))) return rc;
    return launch_knn_mfma(p, d_descr1, d_descr2, d_proposals, d_lcosts, d_nprop, d_bestlabels, d_ws, (hipStream_t)stream);
}

int dflow_knn_proposals_timed(const dflow_params *p, const void *d_descr1, const void *d_descr2, uint32_t *d_proposals,
                              float *d_lcosts, int32_t *d_nprop, int32_t *d_bestlabels, void *d_ws, size_t ws_bytes, void *stream,
                              float *h_ms, double *h_mfma_issued)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_descr1); CHECK_PTR(d_descr2); CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels);
    CHECK_PTR(h_ms);
    CHECK_ALIGNED(DESCR_PAIR_ALIGNED, STATE_ROWS_ALIGNED, STATE_COUNTS_ALIGNED);
    if ((rc = knn_check_screened(__func__, p, d_ws, ws_bytes))) return rc;
    hipEvent_t ev[KNN_MFMA_EVENTS] = {};
    rc = [&]() {
        for (hipEvent_t &e : ev) DFLOW_HIP(hipEventCreate(&e));
        const int r = launch_knn_mfma(p, d_descr1, d_descr2, d_proposals, d_lcosts, d_nprop, d_bestlabels, d_ws, (hipStream_t)stream, ev);
        if (r) return r;
        DFLOW_HIP(hipEventSynchronize(ev[KNN_MFMA_EVENTS - 1]));
        for (int k = 0; k + 1 < KNN_MFMA_EVENTS; k++) DFLOW_HIP(hipEventElapsedTime(&h_ms[k], ev[k], ev[k + 1]));
        return DFLOW_OK;
    }();
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);        // clean-up: the first error, if any, is the one reported
    if (h_mfma_issued) *h_mfma_issued = knn_mfma_issued(p);
    return rc;
}

int dflow_knn_screen_stats_n(const dflow_params *p, void *d_ws, size_t ws_bytes, void *stream, int64_t *h_stats, int n_stats)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(h_stats);
    if (n_stats < 1 || n_stats > DFLOW_KNN_STATS_ALL_N)
        return dflow_set_error(DFLOW_EINVAL, "%s: n_stats = %d outside 1..%d", __func__, n_stats, DFLOW_KNN_STATS_ALL_N);
    if ((rc = knn_check_screened(__func__, p, d_ws, ws_bytes))) return rc;
    int64_t all[DFLOW_KNN_STATS_ALL_N];
    rc = knn_mfma_stats(p, d_ws, (hipStream_t)stream, all);
    if (rc == DFLOW_OK) memcpy(h_stats, all, (size_t)n_stats * sizeof(int64_t));
    return rc;
}

int dflow_knn_screen_stats(const dflow_params *p, void *d_ws, size_t ws_bytes, void *stream, int64_t *h_stats)
{
    return dflow_knn_screen_stats_n(p, d_ws, ws_bytes, stream, h_stats, DFLOW_KNN_STATS_N);
}

int dflow_neighbour_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2, uint32_t *d_proposals,
                              float *d_lcosts, int32_t *d_nprop, const int32_t *d_bestlabels, void *d_ws, size_t ws_bytes,
                              void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_descr1); CHECK_PTR(d_descr2); CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels);
    CHECK_ALIGNED(DESCR_PAIR_ALIGNED, STATE_ROWS_ALIGNED, STATE_COUNTS_ALIGNED);
    CHECK_WS(WS_ALIGN_MAIN, neighbour_ws_bytes(p));
    return launch_neighbour(p, d_descr1, d_descr2, d_proposals, d_lcosts, d_nprop, d_bestlabels, d_ws, (hipStream_t)stream);
}

int dflow_bcd_prepare(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                      void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop);
    CHECK_ALIGNED(STATE_ROWS_ALIGNED, {"d_nprop", d_nprop, ALIGN_WORD});
    CHECK_WS(WS_ALIGN_MAIN, bcd_ws_bytes(p));
    return launch_bcd_prepare(p, d_proposals, d_lcosts, d_nprop, d_ws, (hipStream_t)stream);
}

int dflow_bcd_phase(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop, int32_t *d_bestlabels,
                    int32_t phase, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels);
    if ((rc = check_int_range(NULL, "phase", phase, 0, 3))) return rc;
    // d_proposals is not read (the records of dflow_bcd_prepare hold the flows): it is held to what the stages that read it ask
    CHECK_ALIGNED({"d_proposals", d_proposals, ALIGN_LABEL_ROWS}, STATE_COUNTS_ALIGNED);
    CHECK_WS(WS_ALIGN_MAIN, bcd_ws_bytes(p));
    return launch_bcd_phase(p, d_nprop, d_bestlabels, phase, d_ws, (hipStream_t)stream);
}

int dflow_bcd_sweep(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop, int32_t *d_bestlabels,
                    void *d_ws, size_t ws_bytes, void *stream)
{
    for (int ph = 0; ph < 4; ph++) {
        int rc = dflow_bcd_phase(p, d_proposals, d_nprop, d_bestlabels, ph, d_ws, ws_bytes, stream);
        if (rc) return rc;
    }
    return DFLOW_OK;
}

int dflow_bcd_phase_batch(const dflow_params *p, int32_t npass, const int32_t *const *d_nprop, int32_t *const *d_bestlabels,
                          int32_t phase, void *const *d_ws, size_t ws_bytes, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels); CHECK_PTR(d_ws);
    if ((rc = check_int_range(NULL, "npass", npass, 1, 1024))) return rc;
    if ((rc = check_int_range(NULL, "phase", phase, 0, 3))) return rc;
    // one size for every pass, before the passes' own pointers
    if ((rc = check_ws_size(__func__, d_ws, ws_bytes, bcd_ws_bytes(p)))) return rc;
    for (int i = 0; i < npass; i++)
        if (!d_nprop[i] || !d_bestlabels[i] || !d_ws[i]) return dflow_set_error(DFLOW_EINVAL, "%s: pass %d has a NULL pointer", __func__, i);
    for (int i = 0; i < npass; i++) {
        if ((rc = check_aligned_entry(__func__, "d_nprop", i, d_nprop[i], ALIGN_WORD))) return rc;
        if ((rc = check_aligned_entry(__func__, "d_bestlabels", i, d_bestlabels[i], ALIGN_WORD))) return rc;
    }
    for (int i = 0; i < npass; i++)
        if ((rc = check_aligned_entry(__func__, "d_ws", i, d_ws[i], WS_ALIGN_MAIN))) return rc;
    return launch_bcd_phase_batch(p, npass, d_nprop, d_bestlabels, phase, d_ws, (hipStream_t)stream);
}

int dflow_bcd_sweep_batch(const dflow_params *p, int32_t npass, const int32_t *const *d_nprop, int32_t *const *d_bestlabels,
                          void *const *d_ws, size_t ws_bytes, void *stream)
{
    for (int ph = 0; ph < 4; ph++) {
        int rc = dflow_bcd_phase_batch(p, npass, d_nprop, d_bestlabels, ph, d_ws, ws_bytes, stream);
        if (rc) return rc;
    }
    return DFLOW_OK;
}

// the fields of *p that say how a labelling's state is laid out and compared; no cell grid, so frames below 8 x 8 pass
static int labelling_check_params(const char *fn, const dflow_params *p)
{
    if (!p) return dflow_set_error(DFLOW_EINVAL, "%s: params is NULL", fn);
    int rc = check_frame_size(fn, p->pich, p->picw); if (rc) return rc;
    if (p->label_pitch < 16 || p->label_pitch % 16 != 0 || p->label_pitch > DFLOW_MAX_LABELS)
        return dflow_set_error(DFLOW_EINVAL, "%s: label_pitch=%d must be a multiple of 16 in [16,%d]", fn, p->label_pitch, DFLOW_MAX_LABELS);
    if (p->maxnprop < 1 || p->maxnprop > p->label_pitch)
        return dflow_set_error(DFLOW_EINVAL, "%s: maxnprop=%d outside [1,label_pitch=%d]", fn, p->maxnprop, p->label_pitch);
    return check_int_range(fn, "tpsi", p->tpsi, 1, 8);
}

// the fields of *p a labelling's statistics depend on
static int bcd_stats_check_params(const char *fn, const dflow_params *p)
{
    int rc = labelling_check_params(fn, p);
    return rc ? rc : check_finite_ge0(fn, "tphi", p->tphi);
}

// The end of the gates of dflow_bcd_stats and dflow_bcd_stats_batch.  d_stats and d_ws both hold doubles; d_ws has always been
// named among the aligned pointers here, so its alignment is checked before its size.
static int bcd_stats_check_out(const char *fn, const dflow_params *p, int32_t npass, const void *d_stats, const void *d_ws, size_t ws_bytes)
{
    int rc = check_aligned(fn, {{"d_stats", d_stats, 8}, {"d_ws", d_ws, 8}}); if (rc) return rc;
    return check_ws(fn, d_ws, ws_bytes, 8, (size_t)npass * bcd_stats_ws_bytes(p->pich, p->picw));
}

size_t dflow_bcd_stats_workspace_bytes(const dflow_params *p)
{
    if (bcd_stats_check_params(__func__, p) != DFLOW_OK) return 0;
    return bcd_stats_ws_bytes(p->pich, p->picw);
}

int dflow_bcd_stats_batch(const dflow_params *p, int32_t npass, const uint32_t *const *d_proposals, const float *const *d_lcosts,
                          const int32_t *const *d_nprop, const int32_t *const *d_bestlabels, int32_t *const *d_prev,
                          struct dflow_bcd_stats *d_stats, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = bcd_stats_check_params(__func__, p); if (rc) return rc;
    if ((rc = check_int_range(__func__, "npass", npass, 1, 1024))) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels); CHECK_PTR(d_stats);
    for (int i = 0; i < npass; i++)
        if (!d_proposals[i] || !d_lcosts[i] || !d_nprop[i] || !d_bestlabels[i])
            return dflow_set_error(DFLOW_EINVAL, "%s: pass %d has a NULL pointer", __func__, i);
    for (int i = 0; i < npass; i++) {
        if ((rc = check_aligned_entry(__func__, "d_proposals", i, d_proposals[i], ALIGN_LABEL_ROWS))) return rc;
        if ((rc = check_aligned_entry(__func__, "d_lcosts", i, d_lcosts[i], ALIGN_LABEL_ROWS))) return rc;
        if ((rc = check_aligned_entry(__func__, "d_nprop", i, d_nprop[i], ALIGN_WORD))) return rc;
        if ((rc = check_aligned_entry(__func__, "d_bestlabels", i, d_bestlabels[i], ALIGN_WORD))) return rc;
        if (d_prev && (rc = check_aligned_entry(__func__, "d_prev", i, d_prev[i], ALIGN_WORD))) return rc;
    }
    if ((rc = bcd_stats_check_out(__func__, p, npass, d_stats, d_ws, ws_bytes))) return rc;
    return launch_bcd_stats_batch(p, npass, d_proposals, d_lcosts, d_nprop, d_bestlabels, d_prev, d_prev, d_stats, d_ws,
                                  (hipStream_t)stream);
}

int dflow_bcd_stats(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                    const int32_t *d_bestlabels, const int32_t *d_prev_labels, int32_t *d_prev_out, struct dflow_bcd_stats *d_stats,
                    void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = bcd_stats_check_params(__func__, p); if (rc) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels); CHECK_PTR(d_stats);
    CHECK_ALIGNED(STATE_ROWS_ALIGNED, STATE_COUNTS_ALIGNED, {"d_prev_labels", d_prev_labels, ALIGN_WORD}, {"d_prev_out", d_prev_out, ALIGN_WORD});
    if ((rc = bcd_stats_check_out(__func__, p, 1, d_stats, d_ws, ws_bytes))) return rc;
    return launch_bcd_stats_batch(p, 1, &d_proposals, &d_lcosts, &d_nprop, &d_bestlabels, &d_prev_labels, &d_prev_out, d_stats,
                                  d_ws, (hipStream_t)stream);
}

int dflow_labels_to_flow(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_bestlabels, float *d_flow,
                         void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_bestlabels); CHECK_PTR(d_flow);
    // labels_to_flow_kernel stores a pixel's [dy,dx] as one float2
    CHECK_ALIGNED({"d_proposals", d_proposals, ALIGN_LABEL_ROWS}, {"d_bestlabels", d_bestlabels, ALIGN_WORD}, {"d_flow", d_flow, ALIGN_FLOW2});
    return launch_labels_to_flow(p, d_proposals, d_bestlabels, d_flow, (hipStream_t)stream);
}

int dflow_fb_consistency(const dflow_params *p, const float *d_fwd, const float *d_bwd, float tresh, float *d_sparse,
                         void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_fwd); CHECK_PTR(d_bwd); CHECK_PTR(d_sparse);
    // fb_consistency_kernel loads a pixel's [dy,dx] as one float2 and stores [U,V,valid] a float at a time
    CHECK_ALIGNED({"d_fwd", d_fwd, ALIGN_FLOW2}, {"d_bwd", d_bwd, ALIGN_FLOW2}, {"d_sparse", d_sparse, ALIGN_WORD});
    return launch_fb_consistency(p, d_fwd, d_bwd, tresh, d_sparse, (hipStream_t)stream);
}

int dflow_pack_compat(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop, uint8_t *d_packed,
                      void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_nprop); CHECK_PTR(d_packed);
    // d_packed is written byte by byte
    CHECK_ALIGNED({"d_proposals", d_proposals, ALIGN_LABEL_ROWS}, {"d_nprop", d_nprop, ALIGN_WORD});
    return launch_pack_compat(p, d_proposals, d_nprop, d_packed, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_canny_workspace_bytes, canny_ws_bytes)

int dflow_canny_edges(int32_t h, int32_t w, const uint8_t *d_bgr, double low, double high, uint8_t *d_edges, float *d_ivice,
                      void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    // one message names both thresholds
    if (!isfinite(low) || !isfinite(high) || low < 0.0 || high < 0.0)
        return dflow_set_error(DFLOW_EINVAL, "%s: thresholds %g, %g must be finite and >= 0", __func__, low, high);
    CHECK_PTR(d_bgr); CHECK_PTR(d_edges);
    // the image and d_edges move byte by byte
    CHECK_ALIGNED({"d_ivice", d_ivice, ALIGN_WORD});
    CHECK_WS(4, canny_ws_bytes(h, w));
    if (low > high) { const double t = low; low = high; high = t; }      // cv::Canny swaps them
    // m <= 4 * 255 * 2: larger thresholds all mean "no candidate" / "no strong pixel"
    const int lo = (int)floor(fmin(low, 1 << 20)), hi = (int)floor(fmin(high, 1 << 20));
    return launch_canny(h, w, d_bgr, lo, hi, d_edges, d_ivice, d_ws, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_pb_workspace_bytes, pb_ws_bytes)

int dflow_pb_edges(int32_t h, int32_t w, const uint8_t *d_bgr, int32_t radius, float *d_strength, float *d_orient_strength,
                   void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "radius", radius, 1, DFLOW_PB_MAX_RADIUS))) return rc;
    CHECK_PTR(d_bgr); CHECK_PTR(d_strength);
    CHECK_ALIGNED({"d_strength", d_strength, ALIGN_WORD}, {"d_orient_strength", d_orient_strength, ALIGN_WORD});
    CHECK_WS(2, pb_ws_bytes(h, w));
    return launch_pb(h, w, d_bgr, radius, d_strength, d_orient_strength, d_ws, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_epic_workspace_bytes, epic_ws_bytes)

int dflow_epic_interpolate(int32_t h, int32_t w, const float *d_sparse, const float *d_edges, int32_t nn, double k,
                           int32_t method, float *d_flow, int32_t *d_seed_of, uint32_t *d_dist, int32_t *d_lists,
                           uint64_t *d_list_g, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "nn", nn, 1, 256))) return rc;
    if ((rc = check_finite_gt0(__func__, "k", k))) return rc;
    if (method != DFLOW_EPIC_LA && method != DFLOW_EPIC_NW)
        return dflow_set_error(DFLOW_EINVAL, "%s: unknown method %d", __func__, method);
    CHECK_PTR(d_sparse); CHECK_PTR(d_edges); CHECK_PTR(d_flow);
    // every plane moves an element at a time: floats and int32, and the uint64 distances of d_list_g
    CHECK_ALIGNED({"d_sparse", d_sparse, ALIGN_WORD}, {"d_edges", d_edges, ALIGN_WORD}, {"d_flow", d_flow, ALIGN_WORD},
                  {"d_seed_of", d_seed_of, ALIGN_WORD}, {"d_dist", d_dist, ALIGN_WORD}, {"d_lists", d_lists, ALIGN_WORD},
                  {"d_list_g", d_list_g, 8});
    CHECK_WS(8, epic_ws_bytes(h, w));
    return launch_epic(h, w, d_sparse, d_edges, nn, k, method, d_flow, d_seed_of, d_dist, d_lists, d_list_g, d_ws,
                       (hipStream_t)stream);
}

int dflow_epic_last_stats(int32_t *rounds, float *stage_ms) { return epic_last_stats(rounds, stage_ms); }

FRAME_WS_BYTES(dflow_epic_prefilter_workspace_bytes, epic_prefilter_ws_bytes)

int dflow_epic_prefilter(int32_t h, int32_t w, const uint8_t *d_bgr, const float *d_sparse_in, const float *d_edges,
                         double saliency_th, int32_t pref_nn, double pref_th, double k, float *d_sparse_out, uint8_t *d_reason,
                         float *d_saliency, float *d_estimate, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_finite_ge0(__func__, "saliency_th", saliency_th))) return rc;
    if ((rc = check_int_range(__func__, "pref_nn", pref_nn, 0, 255))) return rc;
    if ((rc = check_finite_ge0(__func__, "pref_th", pref_th))) return rc;
    if ((rc = check_finite_gt0(__func__, "k", k))) return rc;
    if (saliency_th != 0.0 && !d_bgr)
        return dflow_set_error(DFLOW_EINVAL, "%s: d_bgr is NULL with saliency_th=%g (only saliency_th = 0 runs without the image)",
                               __func__, saliency_th);
    CHECK_PTR(d_sparse_in); CHECK_PTR(d_edges); CHECK_PTR(d_sparse_out);
    // the image and d_reason move byte by byte, the float planes a float at a time
    CHECK_ALIGNED({"d_sparse_in", d_sparse_in, ALIGN_WORD}, {"d_edges", d_edges, ALIGN_WORD}, {"d_sparse_out", d_sparse_out, ALIGN_WORD},
                  {"d_saliency", d_saliency, ALIGN_WORD}, {"d_estimate", d_estimate, ALIGN_WORD});
    CHECK_WS(8, epic_prefilter_ws_bytes(h, w));
    return launch_epic_prefilter(h, w, d_bgr, d_sparse_in, d_edges, saliency_th, pref_nn, pref_th, k, d_sparse_out, d_reason,
                                 d_saliency, d_estimate, d_ws, (hipStream_t)stream);
}

int dflow_epic_prefilter_last_stats(int32_t *counts, float *stage_ms) { return epic_prefilter_last_stats(counts, stage_ms); }

void dflow_var_default_params(dflow_var_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->alpha = 1.0f; p->gamma = 0.71f; p->delta = 0.0f; p->sigma = 1.0f; p->sor_omega = 1.9f;
    p->niter_outer = 5; p->niter_inner = 1; p->niter_solver = 30;
}

FRAME_WS_BYTES(dflow_var_workspace_bytes, var_ws_bytes)

int dflow_var_refine(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2, const float *d_flow_in,
                     const dflow_var_params *p, float *d_flow_out, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    CHECK_PTR(p); CHECK_PTR(d_bgr1); CHECK_PTR(d_bgr2); CHECK_PTR(d_flow_in); CHECK_PTR(d_flow_out);
    if ((rc = check_finite_ge0(__func__, "alpha", p->alpha))) return rc;
    if ((rc = check_finite_ge0(__func__, "gamma", p->gamma))) return rc;
    if ((rc = check_finite_ge0(__func__, "delta", p->delta))) return rc;
    if (!isfinite(p->sigma) || p->sigma < 0.0f || p->sigma > 5.0f)
        return dflow_set_error(DFLOW_EINVAL, "%s: sigma=%g outside [0,5]", __func__, (double)p->sigma);
    if (!(p->sor_omega > 0.0f && p->sor_omega < 2.0f))
        return dflow_set_error(DFLOW_EINVAL, "%s: sor_omega=%g outside (0,2)", __func__, (double)p->sor_omega);
    if ((rc = check_int_range(__func__, "niter_outer", p->niter_outer, 0, 1000))) return rc;
    if ((rc = check_int_range(__func__, "niter_inner", p->niter_inner, 1, 1000))) return rc;
    if ((rc = check_int_range(__func__, "niter_solver", p->niter_solver, 1, 10000))) return rc;
    if ((rc = check_flags(__func__, p->flags, DFLOW_VAR_FLAG_SOR_UNFUSED))) return rc;
    // var_split_kernel and var_join_kernel move a pixel's [dy,dx] as one float2; the images are read byte by byte
    CHECK_ALIGNED({"d_flow_in", d_flow_in, ALIGN_FLOW2}, {"d_flow_out", d_flow_out, ALIGN_FLOW2});
    CHECK_WS(4, var_ws_bytes(h, w));
    return launch_var(h, w, d_bgr1, d_bgr2, d_flow_in, p, d_flow_out, d_ws, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_eval_workspace_bytes, eval_ws_bytes)

int dflow_flow_eval(int32_t h, int32_t w, const float *d_test, int32_t test_layout, const float *d_gt, float abs_thresh,
                    uint32_t flags, dflow_eval_stats *d_stats, float *d_err, uint8_t *d_err_bgr, void *d_ws, size_t ws_bytes,
                    void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "test_layout", test_layout))) return rc;
    if ((rc = check_finite_ge0(__func__, "abs_thresh", abs_thresh))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_EVAL_FLAG_ACCUMULATE))) return rc;
    CHECK_PTR(d_test); CHECK_PTR(d_gt); CHECK_PTR(d_stats);
    // the kernel moves four pixels per lane with 16-byte loads and stores
    rc = check_aligned(__func__, {{"d_test", d_test, 16}, {"d_gt", d_gt, 16}, {"d_stats", d_stats, 8}, {"d_err", d_err, 16},
                                  {"d_err_bgr", d_err_bgr, 4}});
    if (rc) return rc;
    CHECK_WS(8, eval_ws_bytes(h, w));
    return launch_flow_eval(h, w, d_test, test_layout, d_gt, abs_thresh, flags, d_stats, d_err, d_err_bgr, d_ws, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_flow_color_workspace_bytes, flow_color_ws_bytes)

int dflow_flow_color(int32_t h, int32_t w, const float *d_flow, int32_t layout, float max_flow, uint8_t *d_bgr, float *d_maxrad,
                     void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_finite_ge0(__func__, "max_flow", max_flow, " (0: the field's own maximum)"))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_bgr);
    // the kernels move four pixels per lane: 16-byte loads of the flow, 12-byte stores of the picture
    rc = check_aligned(__func__, {{"d_flow", d_flow, 16}, {"d_bgr", d_bgr, 4}, {"d_maxrad", d_maxrad, 4}}); if (rc) return rc;
    CHECK_WS(4, flow_color_ws_bytes(h, w));
    return launch_flow_color(h, w, d_flow, layout, max_flow, d_bgr, d_maxrad, d_ws, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_warp_eval_workspace_bytes, warp_eval_ws_bytes)

int dflow_warp_eval(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2, const float *d_flow, int32_t layout,
                    float err_thresh, float err_max, uint32_t flags, dflow_photo_stats *d_stats, uint8_t *d_warped, float *d_err,
                    uint8_t *d_err_bgr, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_finite_ge0(__func__, "err_thresh", err_thresh))) return rc;
    if ((rc = check_finite_gt0(__func__, "err_max", err_max))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_WARP_FLAG_ACCUMULATE))) return rc;
    CHECK_PTR(d_bgr1); CHECK_PTR(d_bgr2); CHECK_PTR(d_flow); CHECK_PTR(d_stats);
    // the kernel moves four pixels per lane: 16-byte loads and stores of the float planes, 12-byte ones of the uint8 planes
    rc = check_aligned(__func__, {{"d_bgr1", d_bgr1, 4}, {"d_flow", d_flow, 16}, {"d_stats", d_stats, 8}, {"d_warped", d_warped, 4},
                                  {"d_err", d_err, 16}, {"d_err_bgr", d_err_bgr, 4}});
    if (rc) return rc;
    CHECK_WS(8, warp_eval_ws_bytes(h, w));
    return launch_warp_eval(h, w, d_bgr1, d_bgr2, d_flow, layout, err_thresh, err_max, flags, d_stats, d_warped, d_err, d_err_bgr,
                            d_ws, (hipStream_t)stream);
}

int dflow_prior_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2, const float *d_prior, int32_t layout,
                          int32_t stride, uint32_t flags, uint32_t *d_proposals, float *d_lcosts, int32_t *d_nprop,
                          int32_t *d_bestlabels, int32_t *d_counts, void *stream)
{
    int rc = dflow_check_params(p); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_int_range(__func__, "stride", stride, 0, 8192))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_PRIOR_SEED_LABELS))) return rc;
    CHECK_PTR(d_descr1); CHECK_PTR(d_descr2); CHECK_PTR(d_prior); CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop);
    CHECK_PTR(d_bestlabels);
    // the kernel reads the label rows and the descriptors' tails 16 bytes at a time
    rc = check_aligned(__func__, {{"d_descr1", d_descr1, 16}, {"d_descr2", d_descr2, 16}, {"d_prior", d_prior, 4},
                                  {"d_proposals", d_proposals, 16}, {"d_lcosts", d_lcosts, 4}, {"d_nprop", d_nprop, 4},
                                  {"d_bestlabels", d_bestlabels, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the prior is read while the state is written
    for (const void *q : {d_descr1, d_descr2, (const void *)d_proposals, (const void *)d_lcosts, (const void *)d_nprop,
                          (const void *)d_bestlabels, (const void *)d_counts})
        if (q == (const void *)d_prior) return dflow_set_error(DFLOW_EINVAL, "%s: d_prior is one of the state pointers", __func__);
    return launch_prior(p, d_descr1, d_descr2, d_prior, layout, stride, flags, d_proposals, d_lcosts, d_nprop, d_bestlabels, d_counts,
                        (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_flow_advance_workspace_bytes, flow_advance_ws_bytes)

int dflow_flow_advance(int32_t h, int32_t w, const float *d_flow, int32_t layout, uint32_t flags, float *d_out, int32_t *d_counts,
                       void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_ADVANCE_NEGATE))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_out);
    rc = check_aligned(__func__, {{"d_flow", d_flow, 4}, {"d_out", d_out, 4}, {"d_counts", d_counts, 4}, {"d_ws", d_ws, 4}});
    if (rc) return rc;
    // a target's winner is read from d_flow after other targets have been written
    if (d_out == d_flow) return dflow_set_error(DFLOW_EINVAL, "%s: d_out and d_flow are the same plane", __func__);
    CHECK_WS(4, flow_advance_ws_bytes(h, w));
    return launch_flow_advance(h, w, d_flow, layout, flags, d_out, d_counts, d_ws, (hipStream_t)stream);
}

int dflow_pyr_down(int32_t h, int32_t w, const uint8_t *d_in1, const uint8_t *d_in2, uint8_t *d_out1, uint8_t *d_out2, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    CHECK_PTR(d_in1); CHECK_PTR(d_out1);
    if ((d_in2 == NULL) != (d_out2 == NULL))
        return dflow_set_error(DFLOW_EINVAL, "%s: d_in2 and d_out2 must both be NULL or both be given", __func__);
    // the kernel reads and writes the aligned dwords of the planes
    rc = check_aligned(__func__, {{"d_in1", d_in1, 4}, {"d_in2", d_in2, 4}, {"d_out1", d_out1, 4}, {"d_out2", d_out2, 4}});
    if (rc) return rc;
    // a tile's input is read while other tiles' output is written, and the two images run side by side
    for (const uint8_t *in : {d_in1, d_in2})
        for (const uint8_t *out : {(const uint8_t *)d_out1, (const uint8_t *)d_out2})
            if (in && in == out) return dflow_set_error(DFLOW_EINVAL, "%s: an output is the same plane as an input", __func__);
    if (d_out1 == d_out2) return dflow_set_error(DFLOW_EINVAL, "%s: d_out1 and d_out2 are the same plane", __func__);
    return launch_pyr_down(h, w, d_in1, d_in2, d_out1, d_out2, (hipStream_t)stream);
}

int dflow_flow_upsample(int32_t h, int32_t w, const float *d_coarse, int32_t layout, float *d_out, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    CHECK_PTR(d_coarse); CHECK_PTR(d_out);
    rc = check_aligned(__func__, {{"d_coarse", d_coarse, 4}, {"d_out", d_out, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a fine pixel's corners are read after other fine pixels have been written
    if (d_out == d_coarse) return dflow_set_error(DFLOW_EINVAL, "%s: d_out and d_coarse are the same plane", __func__);
    if ((const void *)d_counts == (const void *)d_coarse || (const void *)d_counts == (const void *)d_out)
        return dflow_set_error(DFLOW_EINVAL, "%s: d_counts is the same plane as d_coarse or d_out", __func__);
    return launch_flow_upsample(h, w, d_coarse, layout, d_out, d_counts, (hipStream_t)stream);
}

int dflow_flow_consistency(int32_t h, int32_t w, const float *d_fwd, int32_t layout_fwd, const float *d_bwd, int32_t layout_bwd,
                           float thresh, uint32_t flags, float *d_out_fwd, float *d_out_bwd, float *d_err_fwd, float *d_err_bwd,
                           int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout_fwd))) return rc;     // neither message says which of the two it is
    if ((rc = check_layout(__func__, "layout", layout_bwd))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_FBC_BILINEAR))) return rc;
    if ((rc = check_finite_ge0(__func__, "thresh", thresh))) return rc;
    CHECK_PTR(d_fwd); CHECK_PTR(d_bwd); CHECK_PTR(d_out_fwd);
    if (d_err_bwd && !d_out_bwd) return dflow_set_error(DFLOW_EINVAL, "%s: d_err_bwd needs d_out_bwd", __func__);
    rc = check_aligned(__func__, {{"d_fwd", d_fwd, 4}, {"d_bwd", d_bwd, 4}, {"d_out_fwd", d_out_fwd, 4}, {"d_out_bwd", d_out_bwd, 4},
                                  {"d_err_fwd", d_err_fwd, 4}, {"d_err_bwd", d_err_bwd, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a pixel's target is read after other pixels have been written, and the two directions run side by side
    const void *outs[] = {d_out_fwd, d_out_bwd, d_err_fwd, d_err_bwd, d_counts};
    for (size_t i = 0; i < 5; i++) {
        if (!outs[i]) continue;
        if (outs[i] == (const void *)d_fwd || outs[i] == (const void *)d_bwd)
            return dflow_set_error(DFLOW_EINVAL, "%s: an output is the same plane as an input", __func__);
        for (size_t j = 0; j < i; j++)
            if (outs[i] == outs[j]) return dflow_set_error(DFLOW_EINVAL, "%s: two outputs are the same plane", __func__);
    }
    return launch_flow_consistency(h, w, d_fwd, layout_fwd, d_bwd, layout_bwd, thresh, flags, d_out_fwd, d_out_bwd, d_err_fwd, d_err_bwd,
                                   d_counts, (hipStream_t)stream);
}

FRAME_WS_BYTES(dflow_segment_filter_workspace_bytes, segment_filter_ws_bytes)

int dflow_segment_filter(int32_t h, int32_t w, const float *d_flow, int32_t layout, float thresh, int32_t min_size, uint32_t flags,
                         float *d_out, int32_t *d_segment, int32_t *d_size, int32_t *d_counts, void *d_ws, size_t ws_bytes, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_SEG_KEEP_SINGLETONS))) return rc;
    if ((rc = check_finite_ge0(__func__, "thresh", thresh))) return rc;
    if (min_size < 0) return dflow_set_error(DFLOW_EINVAL, "%s: min_size=%d must be >= 0", __func__, min_size);
    CHECK_PTR(d_flow); CHECK_PTR(d_out);
    rc = check_aligned(__func__, {{"d_flow", d_flow, 4}, {"d_out", d_out, 4}, {"d_segment", d_segment, 4}, {"d_size", d_size, 4},
                                  {"d_counts", d_counts, 4}, {"d_ws", d_ws, 4}});
    if (rc) return rc;
    // Every plane is read or written by lanes other than the pixel's own, but for d_out: seg_write_kernel reads a pixel of d_flow
    // and writes the same pixel of d_out, so under UVV (equal pitch) the two may be one plane.  Nothing else may share a byte.
    const size_t n = (size_t)h * (size_t)w, need = segment_filter_ws_bytes(h, w);
    const struct { const char *name; const void *p; size_t bytes; } planes[] = {
        {"d_flow", d_flow, n * (layout == DFLOW_EVAL_UVV ? 3 : 2) * sizeof(float)}, {"d_out", d_out, n * 3 * sizeof(float)},
        {"d_segment", d_segment, n * sizeof(int32_t)}, {"d_size", d_size, n * sizeof(int32_t)},
        {"d_counts", d_counts, 4 * sizeof(int32_t)}, {"d_ws", d_ws, ws_bytes < need ? ws_bytes : need}};
    for (size_t i = 0; i < 6; i++)
        for (size_t j = 0; j < i; j++) {
            if (!planes[i].p || !planes[j].p) continue;
            if (i == 1 && j == 0 && d_out == d_flow && layout == DFLOW_EVAL_UVV) continue;
            const uintptr_t a = (uintptr_t)planes[i].p, b = (uintptr_t)planes[j].p;
            if (a < b + planes[j].bytes && b < a + planes[i].bytes)
                return dflow_set_error(DFLOW_EINVAL, "%s: %s and %s overlap", __func__, planes[j].name, planes[i].name);
        }
    CHECK_WS(4, need);
    return launch_segment_filter(h, w, d_flow, layout, thresh, min_size, flags, d_out, d_segment, d_size, d_counts, d_ws,
                                 (hipStream_t)stream);
}

int dflow_frame_interp(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2, const float *d_fwd, int32_t layout_fwd,
                       const float *d_bwd, int32_t layout_bwd, float t, int32_t fill_rounds, float occl_thresh, uint32_t flags,
                       uint8_t *d_out, uint64_t *d_keys, float *d_motion, float *d_motion_tmp, uint8_t *d_source, int32_t *d_counts,
                       void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout_fwd", layout_fwd))) return rc;
    if (d_bwd && (rc = check_layout(__func__, "layout_bwd", layout_bwd))) return rc;
    if (!isfinite(t) || !(t > 0.0f && t < 1.0f)) return dflow_set_error(DFLOW_EINVAL, "%s: t=%g must lie in (0, 1)", __func__, (double)t);
    if ((rc = check_int_range(__func__, "fill_rounds", fill_rounds, 0, 64))) return rc;
    if ((rc = check_finite_ge0(__func__, "occl_thresh", occl_thresh))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_bgr1); CHECK_PTR(d_bgr2); CHECK_PTR(d_fwd); CHECK_PTR(d_out); CHECK_PTR(d_keys); CHECK_PTR(d_motion);
    if (fill_rounds > 0 && !d_motion_tmp) return dflow_set_error(DFLOW_EINVAL, "%s: d_motion_tmp is NULL with fill_rounds > 0", __func__);
    // the keys are updated with 64-bit atomics; every other plane is read and written a float, an int32 or a byte at a time
    rc = check_aligned(__func__, {{"d_keys", d_keys, 8}, {"d_fwd", d_fwd, 4}, {"d_bwd", d_bwd, 4}, {"d_motion", d_motion, 4},
                                  {"d_motion_tmp", d_motion_tmp, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // every plane is read or written by lanes other than the pixel's own
    rc = check_distinct(__func__, {{"d_bgr1", d_bgr1}, {"d_bgr2", d_bgr2}, {"d_fwd", d_fwd}, {"d_bwd", d_bwd}},
                        {{"d_out", d_out}, {"d_keys", d_keys}, {"d_motion", d_motion}, {"d_motion_tmp", d_motion_tmp},
                         {"d_source", d_source}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_frame_interp(h, w, d_bgr1, d_bgr2, d_fwd, layout_fwd, d_bwd, layout_bwd, t, fill_rounds, occl_thresh, d_out, d_keys,
                               d_motion, d_motion_tmp, d_source, d_counts, (hipStream_t)stream);
}

int dflow_flow_wmedian(int32_t h, int32_t w, const float *d_flow, int32_t layout, const uint8_t *d_bgr, int32_t radius,
                       const uint8_t *d_wspace, const uint8_t *d_wcolor, float reject_thresh, uint32_t flags, float *d_out,
                       int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_int_range(__func__, "radius", radius, 1, 8))) return rc;
    if ((rc = check_flags(__func__, flags, DFLOW_WMED_KEEP_HOLES | DFLOW_WMED_REJECT))) return rc;
    if ((flags & DFLOW_WMED_REJECT) && (rc = check_finite_ge0(__func__, "reject_thresh", reject_thresh))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_out);
    if (!d_bgr != !d_wcolor) return dflow_set_error(DFLOW_EINVAL, "%s: d_bgr and d_wcolor must both be NULL or both be given", __func__);
    rc = check_aligned(__func__, {{"d_flow", d_flow, 4}, {"d_out", d_out, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a pixel's neighbours are read after other pixels have been written
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_bgr", d_bgr}, {"d_wspace", d_wspace}, {"d_wcolor", d_wcolor}},
                        {{"d_out", d_out}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_flow_wmedian(h, w, d_flow, layout, d_bgr, radius, d_wspace, d_wcolor, reject_thresh, flags, d_out, d_counts,
                               (hipStream_t)stream);
}

int dflow_motion_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout, const uint8_t *d_exclude, int32_t model, float thresh,
                     int32_t n_hyp, int32_t lo_rounds, int32_t polish, int32_t step, uint64_t seed, uint32_t flags, float *d_model,
                     float *d_models, int32_t *d_hyp_counts, int64_t *d_state, uint8_t *d_class, float *d_model_flow,
                     float *d_residual, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_int_range(__func__, "model", model, DFLOW_MOTION_AFFINE, DFLOW_MOTION_HOMOGRAPHY))) return rc;
    if ((rc = check_finite_gt0(__func__, "thresh", thresh))) return rc;
    if ((rc = check_int_range(__func__, "n_hyp", n_hyp, 1, 65536))) return rc;
    if ((rc = check_int_range(__func__, "lo_rounds", lo_rounds, 0, 4))) return rc;
    if ((rc = check_int_range(__func__, "polish", polish, 0, 4))) return rc;
    if ((rc = check_int_range(__func__, "step", step, 1, 64))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_model); CHECK_PTR(d_models); CHECK_PTR(d_hyp_counts); CHECK_PTR(d_state);
    // the best key and the polish sums are updated with 64-bit atomics
    rc = check_aligned(__func__, {{"d_state", d_state, 8}, {"d_flow", d_flow, 4}, {"d_model", d_model, 4}, {"d_models", d_models, 4},
                                  {"d_hyp_counts", d_hyp_counts, 4}, {"d_model_flow", d_model_flow, 4}, {"d_residual", d_residual, 4},
                                  {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the field is read in every launch, after the planes of the launches before it have been written
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_exclude", d_exclude}},
                        {{"d_model", d_model}, {"d_models", d_models}, {"d_hyp_counts", d_hyp_counts}, {"d_state", d_state},
                         {"d_class", d_class}, {"d_model_flow", d_model_flow}, {"d_residual", d_residual}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_motion_fit(h, w, d_flow, layout, d_exclude, model, thresh, n_hyp, lo_rounds, polish, step, seed, d_model, d_models,
                             d_hyp_counts, d_state, d_class, d_model_flow, d_residual, d_counts, (hipStream_t)stream);
}

int dflow_epipolar_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout, const uint8_t *d_exclude, float thresh, int32_t n_hyp,
                       int32_t lo_rounds, int32_t step, uint64_t seed, uint32_t flags, float *d_model, float *d_models,
                       int32_t *d_hyp_counts, int64_t *d_state, uint8_t *d_class, float *d_residual, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_finite_gt0(__func__, "thresh", thresh))) return rc;
    // three slots per sample, and a slot's index has 16 bits of the best key
    if ((rc = check_int_range(__func__, "n_hyp", n_hyp, 1, 21845))) return rc;
    if ((rc = check_int_range(__func__, "lo_rounds", lo_rounds, 0, 4))) return rc;
    if ((rc = check_int_range(__func__, "step", step, 1, 64))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_model); CHECK_PTR(d_models); CHECK_PTR(d_hyp_counts); CHECK_PTR(d_state);
    // the best key and the counters are updated with 64-bit atomics
    rc = check_aligned(__func__, {{"d_state", d_state, 8}, {"d_flow", d_flow, 4}, {"d_model", d_model, 4}, {"d_models", d_models, 4},
                                  {"d_hyp_counts", d_hyp_counts, 4}, {"d_residual", d_residual, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the field is read in every launch, after the planes of the launches before it have been written
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_exclude", d_exclude}},
                        {{"d_model", d_model}, {"d_models", d_models}, {"d_hyp_counts", d_hyp_counts}, {"d_state", d_state},
                         {"d_class", d_class}, {"d_residual", d_residual}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_epipolar_fit(h, w, d_flow, layout, d_exclude, thresh, n_hyp, lo_rounds, step, seed, d_model, d_models, d_hyp_counts,
                               d_state, d_class, d_residual, d_counts, (hipStream_t)stream);
}

int dflow_label_confidence(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                           const int32_t *d_bestlabels, int32_t mode, int32_t min_sep, float thresh, float *d_margin, int32_t *d_alt,
                           float *d_sparse, int32_t *d_counts, void *stream)
{
    int rc = labelling_check_params(__func__, p); if (rc) return rc;
    if ((rc = check_finite_ge0(__func__, "lamda", p->lamda))) return rc;
    if ((rc = check_int_range(__func__, "mode", mode, DFLOW_CONF_LOCAL, DFLOW_CONF_DATA))) return rc;
    if ((rc = check_int_range(__func__, "min_sep", min_sep, 0, 1024))) return rc;
    if ((rc = check_not_nan(__func__, "thresh", thresh))) return rc;
    if ((rc = check_any_given(__func__, "each of d_margin, d_alt, d_sparse and d_counts", {d_margin, d_alt, d_sparse, d_counts}))) return rc;
    CHECK_PTR(d_proposals); CHECK_PTR(d_lcosts); CHECK_PTR(d_nprop); CHECK_PTR(d_bestlabels);
    // the kernel reads the label and cost rows 16 bytes at a time
    rc = check_aligned(__func__, {{"d_proposals", d_proposals, 16}, {"d_lcosts", d_lcosts, 16}, {"d_sparse", d_sparse, 16},
                                  {"d_nprop", d_nprop, 4}, {"d_bestlabels", d_bestlabels, 4}, {"d_margin", d_margin, 4},
                                  {"d_alt", d_alt, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a pixel's neighbours are read while other pixels are written
    rc = check_distinct(__func__, {{"d_proposals", d_proposals}, {"d_lcosts", d_lcosts}, {"d_nprop", d_nprop}, {"d_bestlabels", d_bestlabels}},
                        {{"d_margin", d_margin}, {"d_alt", d_alt}, {"d_sparse", d_sparse}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_label_confidence(p, d_proposals, d_lcosts, d_nprop, d_bestlabels, mode, min_sep, thresh, d_margin, d_alt, d_sparse,
                                   d_counts, (hipStream_t)stream);
}

int dflow_flow_gate(int32_t h, int32_t w, const float *d_flow, int32_t layout, const float *d_score, float lo, float hi, float *d_out,
                    int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_not_nan(__func__, "lo", lo))) return rc;
    if ((rc = check_not_nan(__func__, "hi", hi))) return rc;
    if ((rc = check_ordered(__func__, "lo", lo, "hi", hi))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_score); CHECK_PTR(d_out);
    // the kernel moves four pixels per lane with 16-byte loads and stores
    rc = check_aligned(__func__, {{"d_flow", d_flow, 16}, {"d_score", d_score, 16}, {"d_out", d_out, 16}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a lane reads its own four pixels before it writes them: under [U,V,valid], where the pitches agree, d_out may be d_flow
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_score", d_score}},
                        {{"d_out", layout == DFLOW_EVAL_UVV && d_out == d_flow ? nullptr : d_out}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_flow_gate(h, w, d_flow, layout, d_score, lo, hi, d_out, d_counts, (hipStream_t)stream);
}

// a track set's capacity, and the planes every track call names; positions move as one float2 per track
#define TRACK_CAP_MAX (1 << 26)

int dflow_track_advance(int32_t h, int32_t w, const float *d_fwd, int32_t layout_fwd, const float *d_bwd, int32_t layout_bwd, int32_t cap,
                        const float *d_pos_in, const int32_t *d_state_in, float rel, float abs, uint32_t flags, float *d_pos_out,
                        int32_t *d_state_out, float *d_err, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout_fwd", layout_fwd))) return rc;
    if (d_bwd && (rc = check_layout(__func__, "layout_bwd", layout_bwd))) return rc;
    if ((rc = check_int_range(__func__, "cap", cap, 1, TRACK_CAP_MAX))) return rc;
    if ((rc = check_finite_ge0(__func__, "rel", rel))) return rc;
    if ((rc = check_finite_ge0(__func__, "abs", abs))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_fwd); CHECK_PTR(d_pos_in); CHECK_PTR(d_state_in); CHECK_PTR(d_pos_out); CHECK_PTR(d_state_out);
    rc = check_aligned(__func__, {{"d_pos_in", d_pos_in, ALIGN_FLOW2}, {"d_pos_out", d_pos_out, ALIGN_FLOW2}, {"d_fwd", d_fwd, 4},
                                  {"d_bwd", d_bwd, 4}, {"d_state_in", d_state_in, 4}, {"d_state_out", d_state_out, 4}, {"d_err", d_err, 4},
                                  {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a lane reads its own slot before it writes it: d_pos_out may be d_pos_in and d_state_out may be d_state_in, nothing else
    rc = check_distinct(__func__, {{"d_fwd", d_fwd}, {"d_bwd", d_bwd}, {"d_pos_in", d_pos_in}, {"d_state_in", d_state_in}},
                        {{"d_pos_out", d_pos_out == d_pos_in ? nullptr : d_pos_out},
                         {"d_state_out", d_state_out == d_state_in ? nullptr : d_state_out}, {"d_err", d_err}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_track_advance(h, w, d_fwd, layout_fwd, d_bwd, layout_bwd, cap, d_pos_in, d_state_in, rel, abs, d_pos_out, d_state_out,
                                d_err, d_counts, (hipStream_t)stream);
}

int dflow_track_seed(int32_t h, int32_t w, int32_t cap, int32_t step, int32_t frame, const uint8_t *d_mask, float *d_pos, int32_t *d_state,
                     int32_t *d_birth, int32_t *d_n, int32_t *d_scan, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "cap", cap, 1, TRACK_CAP_MAX))) return rc;
    if ((rc = check_int_range(__func__, "step", step, 1, 256))) return rc;
    CHECK_PTR(d_pos); CHECK_PTR(d_state); CHECK_PTR(d_birth); CHECK_PTR(d_n); CHECK_PTR(d_scan);
    rc = check_aligned(__func__, {{"d_pos", d_pos, ALIGN_FLOW2}, {"d_state", d_state, 4}, {"d_birth", d_birth, 4}, {"d_n", d_n, 4},
                                  {"d_scan", d_scan, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the set is read by the launches that come before the ones that write it
    rc = check_distinct(__func__, {{"d_mask", d_mask}},
                        {{"d_pos", d_pos}, {"d_state", d_state}, {"d_birth", d_birth}, {"d_n", d_n}, {"d_scan", d_scan}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_track_seed(h, w, cap, step, frame, d_mask, d_pos, d_state, d_birth, d_n, d_scan, d_counts, (hipStream_t)stream);
}

int dflow_track_flow(int32_t h, int32_t w, int32_t cap, const float *d_pos_a, const int32_t *d_state_a, const float *d_pos_b,
                     const int32_t *d_state_b, int32_t *d_owner, float *d_out, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "cap", cap, 1, TRACK_CAP_MAX))) return rc;
    CHECK_PTR(d_pos_a); CHECK_PTR(d_state_a); CHECK_PTR(d_pos_b); CHECK_PTR(d_state_b); CHECK_PTR(d_owner); CHECK_PTR(d_out);
    rc = check_aligned(__func__, {{"d_pos_a", d_pos_a, ALIGN_FLOW2}, {"d_pos_b", d_pos_b, ALIGN_FLOW2}, {"d_state_a", d_state_a, 4},
                                  {"d_state_b", d_state_b, 4}, {"d_owner", d_owner, 4}, {"d_out", d_out, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the two snapshots may be one; the winners and the field are written while the snapshots are read
    rc = check_distinct(__func__, {{"d_pos_a", d_pos_a}, {"d_state_a", d_state_a}, {"d_pos_b", d_pos_b}, {"d_state_b", d_state_b}},
                        {{"d_owner", d_owner}, {"d_out", d_out}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_track_flow(h, w, cap, d_pos_a, d_state_a, d_pos_b, d_state_b, d_owner, d_out, d_counts, (hipStream_t)stream);
}

// the largest number of segments and the largest min_size: the pixels of the largest frame
#define SEGMENTS_MAX (1 << 26)

int dflow_superpixels(int32_t h, int32_t w, const uint8_t *d_bgr, int32_t step, int32_t compactness, int32_t iters, int32_t min_size,
                      uint32_t flags, int32_t *d_label, int32_t *d_centers, int32_t *d_slic, int32_t *d_counts, int32_t *d_sums,
                      int32_t *d_comp, int32_t *d_size, int32_t *d_final, int32_t *d_scan, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "step", step, 4, 64))) return rc;
    if ((rc = check_int_range(__func__, "compactness", compactness, 0, 255))) return rc;
    if ((rc = check_int_range(__func__, "iters", iters, 1, 32))) return rc;
    if ((rc = check_int_range(__func__, "min_size", min_size, 0, SEGMENTS_MAX))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_bgr); CHECK_PTR(d_label); CHECK_PTR(d_centers); CHECK_PTR(d_sums); CHECK_PTR(d_comp); CHECK_PTR(d_size);
    CHECK_PTR(d_final); CHECK_PTR(d_scan);
    rc = check_aligned(__func__, {{"d_label", d_label, 4}, {"d_centers", d_centers, 4}, {"d_slic", d_slic, 4}, {"d_counts", d_counts, 4},
                                  {"d_sums", d_sums, 4}, {"d_comp", d_comp, 4}, {"d_size", d_size, 4}, {"d_final", d_final, 4},
                                  {"d_scan", d_scan, 4}});
    if (rc) return rc;
    // the image is read in every iteration, and every plane is read by a launch after the one that wrote it
    rc = check_distinct(__func__, {{"d_bgr", d_bgr}},
                        {{"d_label", d_label}, {"d_centers", d_centers}, {"d_slic", d_slic}, {"d_counts", d_counts}, {"d_sums", d_sums},
                         {"d_comp", d_comp}, {"d_size", d_size}, {"d_final", d_final}, {"d_scan", d_scan}});
    if (rc) return rc;
    return launch_superpixels(h, w, d_bgr, step, compactness, iters, min_size, d_label, d_centers, d_slic, d_counts, d_sums, d_comp,
                              d_size, d_final, d_scan, (hipStream_t)stream);
}

int dflow_segment_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout, const int32_t *d_label, int32_t n_seg, float thresh,
                      int32_t rounds, uint32_t flags, float *d_models, int32_t *d_seg_counts, float *d_out, uint8_t *d_class,
                      int32_t *d_counts, int64_t *d_acc, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_int_range(__func__, "n_seg", n_seg, 1, SEGMENTS_MAX))) return rc;
    if ((rc = check_finite_gt0(__func__, "thresh", thresh))) return rc;
    if ((rc = check_int_range(__func__, "rounds", rounds, 1, 6))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_label); CHECK_PTR(d_models); CHECK_PTR(d_seg_counts); CHECK_PTR(d_acc);
    // the sums are updated with 64-bit atomics
    rc = check_aligned(__func__, {{"d_acc", d_acc, 8}, {"d_flow", d_flow, 4}, {"d_label", d_label, 4}, {"d_models", d_models, 4},
                                  {"d_seg_counts", d_seg_counts, 4}, {"d_out", d_out, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the field and the labels are read in every launch
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_label", d_label}},
                        {{"d_models", d_models}, {"d_seg_counts", d_seg_counts}, {"d_out", d_out}, {"d_class", d_class},
                         {"d_counts", d_counts}, {"d_acc", d_acc}});
    if (rc) return rc;
    return launch_segment_fit(h, w, d_flow, layout, d_label, n_seg, thresh, rounds, d_models, d_seg_counts, d_out, d_class, d_counts,
                              d_acc, (hipStream_t)stream);
}

int dflow_remove_small_segments_host(float *h_sparse, int32_t dim0, int32_t dim1, float tresh, int32_t min_segment_size)
{
    if (!h_sparse) return dflow_set_error(DFLOW_EINVAL, "h_sparse is NULL");
    if (dim0 <= 0 || dim1 <= 0) return dflow_set_error(DFLOW_EINVAL, "field size %dx%d", dim0, dim1);
    return host_remove_small_segments(h_sparse, dim0, dim1, tresh, min_segment_size);
}

int dflow_two_view(int32_t h, int32_t w, const float *d_flow, int32_t layout, const float *d_model, const uint8_t *d_part, double fx,
                   double fy, double cx, double cy, int32_t step, uint32_t flags, double *d_pose, int64_t *d_state, float *d_depth,
                   uint8_t *d_class, float *d_err, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_layout(__func__, "layout", layout))) return rc;
    if ((rc = check_finite_gt0(__func__, "fx", fx))) return rc;
    if ((rc = check_finite_gt0(__func__, "fy", fy))) return rc;
    if (!isfinite(cx)) return refuse_value(__func__, "cx", cx, "finite");
    if (!isfinite(cy)) return refuse_value(__func__, "cy", cy, "finite");
    if ((rc = check_int_range(__func__, "step", step, 1, 64))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_flow); CHECK_PTR(d_model); CHECK_PTR(d_pose); CHECK_PTR(d_state);
    // the pose is float64, the votes are updated with 64-bit atomics
    rc = check_aligned(__func__, {{"d_pose", d_pose, 8}, {"d_state", d_state, 8}, {"d_flow", d_flow, 4}, {"d_model", d_model, 4},
                                  {"d_depth", d_depth, 4}, {"d_err", d_err, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the field, the model and the voters' plane are read in launches that follow the first writes
    rc = check_distinct(__func__, {{"d_flow", d_flow}, {"d_model", d_model}, {"d_part", d_part}},
                        {{"d_pose", d_pose}, {"d_state", d_state}, {"d_depth", d_depth}, {"d_class", d_class}, {"d_err", d_err},
                         {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_two_view(h, w, d_flow, layout, d_model, d_part, fx, fy, cx, cy, step, d_pose, d_state, d_depth, d_class, d_err,
                           d_counts, (hipStream_t)stream);
}

// ---- sparse feature tracking (include/dflow_klt.h): the shared checks alone, in the order the header states
#define KLT_LEVELS_MAX 8

size_t dflow_klt_pyramid_bytes(int32_t h, int32_t w, int32_t levels)
{
    if (check_frame_size(__func__, h, w) || check_int_range(__func__, "levels", levels, 1, KLT_LEVELS_MAX)) return 0;
    return klt_pyramid_bytes(h, w, levels);
}

int dflow_klt_pyramid(int32_t h, int32_t w, int32_t levels, const uint8_t *d_bgr, uint8_t *d_pyr, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "levels", levels, 1, KLT_LEVELS_MAX))) return rc;
    CHECK_PTR(d_bgr); CHECK_PTR(d_pyr);
    // four pixels move at a time: three dwords in, one out
    if ((rc = check_aligned(__func__, {{"d_bgr", d_bgr, 4}, {"d_pyr", d_pyr, 4}}))) return rc;
    if ((rc = check_distinct(__func__, {{"d_bgr", d_bgr}}, {{"d_pyr", d_pyr}}))) return rc;
    return launch_klt_pyramid(h, w, levels, d_bgr, d_pyr, (hipStream_t)stream);
}

int dflow_corners(int32_t h, int32_t w, const uint8_t *d_pyr, int32_t rc_win, int32_t min_dist, int32_t border, float quality,
                  float min_response, int32_t cap, const float *d_pos, const int32_t *d_state, const int32_t *d_n, float *d_response,
                  uint8_t *d_mask, uint8_t *d_occ, uint32_t *d_rmax, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "rc", rc_win, 1, 7))) return rc;
    if ((rc = check_int_range(__func__, "min_dist", min_dist, 1, 32))) return rc;
    if ((rc = check_int_range(__func__, "border", border, 0, 8192))) return rc;
    if ((rc = check_finite_ge0(__func__, "quality", quality))) return rc;
    if (quality > 1.0f) return refuse_value(__func__, "quality", quality, "<= 1");
    if ((rc = check_finite_ge0(__func__, "min_response", min_response))) return rc;
    // a track set is given whole or not at all
    if (d_pos || d_state || d_n || d_occ) {
        if ((rc = check_int_range(__func__, "cap", cap, 1, TRACK_CAP_MAX))) return rc;
        CHECK_PTR(d_pos); CHECK_PTR(d_state); CHECK_PTR(d_n); CHECK_PTR(d_occ);
    }
    CHECK_PTR(d_pyr); CHECK_PTR(d_response); CHECK_PTR(d_mask); CHECK_PTR(d_rmax);
    rc = check_aligned(__func__, {{"d_pos", d_pos, ALIGN_FLOW2}, {"d_state", d_state, 4}, {"d_n", d_n, 4}, {"d_response", d_response, 4},
                                  {"d_rmax", d_rmax, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // the response is read by the launch after the one that writes it, the set by the one between them
    rc = check_distinct(__func__, {{"d_pyr", d_pyr}, {"d_pos", d_pos}, {"d_state", d_state}, {"d_n", d_n}},
                        {{"d_response", d_response}, {"d_mask", d_mask}, {"d_occ", d_occ}, {"d_rmax", d_rmax}, {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_corners(h, w, d_pyr, rc_win, min_dist, border, quality, min_response, cap, d_pos, d_state, d_n, d_response, d_mask, d_occ,
                          d_rmax, d_counts, (hipStream_t)stream);
}

int dflow_klt_track(int32_t h, int32_t w, int32_t levels, const uint8_t *d_pyr1, const uint8_t *d_pyr2, int32_t cap, const float *d_pos_in,
                    const int32_t *d_state_in, int32_t r, int32_t iters, float eps, float min_eig, float max_err, float fb, uint32_t flags,
                    float *d_pos_out, int32_t *d_state_out, float *d_err, float *d_back, int32_t *d_counts, void *stream)
{
    int rc = check_frame_size(__func__, h, w); if (rc) return rc;
    if ((rc = check_int_range(__func__, "levels", levels, 1, KLT_LEVELS_MAX))) return rc;
    if ((rc = check_int_range(__func__, "cap", cap, 1, TRACK_CAP_MAX))) return rc;
    if ((rc = check_int_range(__func__, "r", r, 1, 10))) return rc;
    if ((rc = check_int_range(__func__, "iters", iters, 1, 64))) return rc;
    if ((rc = check_finite_gt0(__func__, "eps", eps))) return rc;
    if ((rc = check_finite_ge0(__func__, "min_eig", min_eig))) return rc;
    if ((rc = check_finite_ge0(__func__, "max_err", max_err))) return rc;
    if ((rc = check_finite_ge0(__func__, "fb", fb))) return rc;
    if ((rc = check_flags(__func__, flags, 0))) return rc;
    CHECK_PTR(d_pyr1); CHECK_PTR(d_pyr2); CHECK_PTR(d_pos_in); CHECK_PTR(d_state_in); CHECK_PTR(d_pos_out); CHECK_PTR(d_state_out);
    rc = check_aligned(__func__, {{"d_pos_in", d_pos_in, ALIGN_FLOW2}, {"d_pos_out", d_pos_out, ALIGN_FLOW2}, {"d_back", d_back, ALIGN_FLOW2},
                                  {"d_state_in", d_state_in, 4}, {"d_state_out", d_state_out, 4}, {"d_err", d_err, 4}, {"d_counts", d_counts, 4}});
    if (rc) return rc;
    // a lane group reads its own slot before it writes it: d_pos_out may be d_pos_in and d_state_out may be d_state_in, nothing else
    rc = check_distinct(__func__, {{"d_pyr1", d_pyr1}, {"d_pyr2", d_pyr2}, {"d_pos_in", d_pos_in}, {"d_state_in", d_state_in}},
                        {{"d_pos_out", d_pos_out == d_pos_in ? nullptr : d_pos_out},
                         {"d_state_out", d_state_out == d_state_in ? nullptr : d_state_out}, {"d_err", d_err}, {"d_back", d_back},
                         {"d_counts", d_counts}});
    if (rc) return rc;
    return launch_klt_track(h, w, levels, d_pyr1, d_pyr2, cap, d_pos_in, d_state_in, r, iters, eps, min_eig, max_err, fb, d_pos_out,
                            d_state_out, d_err, d_back, d_counts, (hipStream_t)stream);
}

}  // extern "C"
