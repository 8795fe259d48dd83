/*
 * dflow.h -- C-ABI of libdflow.so: the MI355X (gfx950) dense discrete optical-flow stage.
 *
 * The reference (pfe-rs/lk-s-2022-estimacija-pokreta) has no FFI: its hot path is two flat Python scripts
 * that talk through .npy files.  Each entry point below replaces the reference function(s) named next to
 * it; INTEGRATION.md shows the ctypes binding a maintainer would add to the reference scripts.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  All d_* pointers are DEVICE pointers owned by the caller.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous with
 *     respect to the host and ordered on that stream; the library never synchronises and never allocates
 *     device memory: scratch comes from the caller's workspace (dflow_workspace_bytes).
 *   - Return 0 on success, a negative DFLOW_E* code otherwise; dflow_last_error() gives the message
 *     (thread-local).  No global state; re-entrant across devices.
 *   - Alignment of d_ws.  A stage carves typed regions out of its workspace, each at a multiple of 256 bytes from d_ws, and
 *     needs exactly the bytes its size function (or dflow_workspace_bytes) promises: what the workspace holds before the call
 *     does not matter (dflow_bcd_phase / _sweep and dflow_knn_screen_stats read what dflow_bcd_prepare / dflow_knn_proposals
 *     left), and nothing beyond those bytes is written.  d_ws must be aligned for the widest access the stage makes to a
 *     region; a device allocation (256 bytes and more) serves every stage:
 *       16  dflow_daisy, dflow_daisy_pair (float4 planes), dflow_knn_proposals, dflow_knn_proposals_timed,
 *           dflow_knn_screen_stats(_n) (int4 lists), dflow_neighbour_proposals (uint32 flows: 4 would do; one value for the
 *           buffer the main-path stages share), dflow_bcd_prepare, dflow_bcd_phase, dflow_bcd_sweep and every d_ws[i] of
 *           dflow_bcd_phase_batch / dflow_bcd_sweep_batch (uint2 records, back-pointers staged 16 bytes at a time)
 *        8  dflow_bcd_stats, dflow_bcd_stats_batch, dflow_flow_eval, dflow_warp_eval (partial results that hold a double),
 *           dflow_epic_interpolate, dflow_epic_prefilter (uint64 keys updated atomically, uint64 edges)
 *        4  dflow_canny_edges (int32 labels updated atomically), dflow_var_refine (float planes), dflow_flow_color (float
 *           partial maxima), dflow_flow_advance (uint32 winners, atomicMin), dflow_segment_filter (int32 labels and sizes)
 *        2  dflow_pb_edges (uint16 bins)
 *     A d_ws that is not returns DFLOW_EINVAL ("d_ws is not N-byte aligned") before anything is launched.  Every other argument
 *     error is reported first, and so is a NULL or too small workspace (DFLOW_ENOSPC), except by dflow_bcd_stats(_batch),
 *     dflow_flow_advance and dflow_segment_filter, which check d_ws with their other pointers, before its size.
 *   - Alignment of data planes.  A plane needs exactly the bytes of its layout (below, and at each entry point): nothing before
 *     or beyond them is read or written.  Its address must be a multiple of the widest access a kernel makes to it, never less
 *     than the element size, and the state planes of a pass have one number wherever they are passed: 16 for descriptor planes
 *     in both storages (rows move as float4 / 8 x binary16 and through 16-byte LDS-DMA) and for proposals and lcosts (rows are
 *     read 16 bytes at a time; dflow_prior_proposals, which writes costs a float at a time, keeps the 4 it has always asked of
 *     d_lcosts), 8 for (H,W,2) flows that move as float2 and for uint64 / double planes, 4 for other float, int32 and uint32
 *     planes, 1 for images and byte planes unless a stage moves them four pixels at a time.  A device allocation (256 bytes and
 *     more) serves every plane, and so does a view at a multiple of 16 bytes into one.  NULL optional outputs pass.  Per entry
 *     point (d_ws above; planes that are not named need 1):
 *       dflow_daisy                 d_descr 16
 *       dflow_daisy_pair            d_descr1, d_descr2 16
 *       dflow_knn_proposals, dflow_knn_proposals_timed, dflow_neighbour_proposals
 *                                   d_descr1, d_descr2, d_proposals, d_lcosts 16; d_nprop, d_bestlabels 4
 *       dflow_bcd_prepare           d_proposals, d_lcosts 16; d_nprop 4
 *       dflow_bcd_phase, dflow_bcd_sweep
 *                                   d_proposals 16 (not read: what the stages that read it ask); d_nprop, d_bestlabels 4
 *       dflow_bcd_phase_batch, dflow_bcd_sweep_batch
 *                                   every d_nprop[i], d_bestlabels[i] 4
 *       dflow_bcd_stats             d_proposals, d_lcosts 16; d_nprop, d_bestlabels, d_prev_labels, d_prev_out 4; d_stats 8
 *       dflow_bcd_stats_batch       every d_proposals[i], d_lcosts[i] 16; d_nprop[i], d_bestlabels[i], d_prev[i] 4; d_stats 8
 *       dflow_labels_to_flow        d_proposals 16; d_bestlabels 4; d_flow 8 (float2 stores)
 *       dflow_fb_consistency        d_fwd, d_bwd 8 (float2 loads); d_sparse 4
 *       dflow_pack_compat           d_proposals 16; d_nprop 4; d_packed 1
 *       dflow_canny_edges           d_ivice 4; d_bgr, d_edges 1
 *       dflow_pb_edges              d_strength, d_orient_strength 4; d_bgr 1
 *       dflow_epic_interpolate      d_sparse, d_edges, d_flow, d_seed_of, d_dist, d_lists 4; d_list_g 8
 *       dflow_epic_prefilter        d_sparse_in, d_edges, d_sparse_out, d_saliency, d_estimate 4; d_bgr, d_reason 1
 *       dflow_var_refine            d_flow_in, d_flow_out 8 (float2); d_bgr1, d_bgr2 1
 *       dflow_flow_eval             d_test, d_gt, d_err 16; d_stats 8; d_err_bgr 4
 *       dflow_flow_color            d_flow 16; d_bgr, d_maxrad 4
 *       dflow_warp_eval             d_flow, d_err 16; d_stats 8; d_bgr1, d_warped, d_err_bgr 4; d_bgr2 1
 *       dflow_prior_proposals       d_descr1, d_descr2, d_proposals 16; d_prior, d_lcosts, d_nprop, d_bestlabels, d_counts 4
 *       dflow_flow_advance          d_flow, d_out, d_counts 4
 *       dflow_pyr_down              d_in1, d_in2, d_out1, d_out2 4
 *       dflow_flow_upsample         d_coarse, d_out, d_counts 4
 *       dflow_flow_consistency      d_fwd, d_bwd, d_out_fwd, d_out_bwd, d_err_fwd, d_err_bwd, d_counts 4
 *       dflow_segment_filter        d_flow, d_out, d_segment, d_size, d_counts 4
 *       dflow_frame_interp          d_keys 8; d_fwd, d_bwd, d_motion, d_motion_tmp, d_counts 4; d_bgr1, d_bgr2, d_out, d_source 1
 *       dflow_flow_wmedian          d_flow, d_out, d_counts 4; d_bgr, d_wspace, d_wcolor 1
 *       dflow_motion_fit            d_state 8; d_flow, d_model, d_models, d_hyp_counts, d_model_flow, d_residual, d_counts 4;
 *                                   d_exclude, d_class 1
 *       dflow_epipolar_fit          d_state 8; d_flow, d_model, d_models, d_hyp_counts, d_residual, d_counts 4; d_exclude, d_class 1
 *       dflow_label_confidence      d_proposals, d_lcosts, d_sparse 16; d_nprop, d_bestlabels, d_margin, d_alt, d_counts 4
 *       dflow_flow_gate             d_flow, d_score, d_out 16; d_counts 4
 *       dflow_track_advance         d_pos_in, d_pos_out 8 (a position moves as one float2); d_fwd, d_bwd, d_state_in, d_state_out,
 *                                   d_err, d_counts 4
 *       dflow_track_seed            d_pos 8; d_state, d_birth, d_n, d_scan, d_counts 4; d_mask 1
 *       dflow_track_flow            d_pos_a, d_pos_b 8; d_state_a, d_state_b, d_owner, d_out, d_counts 4
 *       dflow_superpixels           d_label, d_centers, d_slic, d_counts, d_sums, d_comp, d_size, d_final, d_scan 4; d_bgr 1
 *       dflow_segment_fit           d_acc 8; d_flow, d_label, d_models, d_seg_counts, d_out, d_counts 4; d_class 1
 *       dflow_two_view              d_pose, d_state 8; d_flow, d_model, d_depth, d_err, d_counts 4; d_part, d_class 1
 *     A plane below its number returns DFLOW_EINVAL ("NAME is not N-byte aligned", the batch forms name the entry NAME[i]) before
 *     anything is launched, after the NULL checks and before the workspace is looked at (the batch forms of the sweeps check the
 *     one size of their workspaces before any per-pass pointer, as they always have).
 *
 * Device layouts (H = pich, W = picw, LP = label_pitch >= maxnprop, multiple of 16)
 *   image      uint8   (H,W,3)   BGR, as cv2.imread returns it            daisy i flann.py:26-27,52-53
 *   descr      float32 (H,W,68)  row y*W+x = keypoint order               daisy i flann.py:69-77
 *              or, with DFLOW_FLAG_DESCR_F16, binary16 (H,W,72): 68 values + 4 zero pads per pixel (144-byte rows)
 *   proposals  uint32  (H,W,LP)  one label = int16 dy | int16 dx << 16,   daisy i flann.py:89 (int64 (H,W,150,2), -1 fill)
 *                                unused slots 0xFFFFFFFF (= [-1,-1])
 *   lcosts     float32 (H,W,LP)  unused slots 1000.0f                     daisy i flann.py:90 (float64; values are float32-exact)
 *   nprop      int32   (H,W)                                              daisy i flann.py:91
 *   bestlabels int32   (H,W)                                              daisy i flann.py:95
 *   flow       float32 (H,W,2)   [dy,dx]                                  python bcd.py:90-95 (float64; values are small integers)
 *   sparse     float32 (H,W,3)   [U=dx, V=dy, valid]                      postprocessing.py:7-17,123-135
 *   prior      float32 (H,W,2)   [dy,dx] (DFLOW_EVAL_DYDX) or (H,W,3) [U,V,valid] (DFLOW_EVAL_UVV): a flow somebody already has,
 *                                read by dflow_prior_proposals and dflow_flow_advance (no counterpart in the reference)
 */
#ifndef DFLOW_H
#define DFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFLOW_VERSION 1
#define DFLOW_DESC 68            /* (4 rings * 4 angles + 1) * 4 bins, daisy i flann.py:66 */
#define DFLOW_MAX_LABELS 160     /* kernels are built for maxnprop <= 160 (reference: 150) */

/* dflow_params.flags */
#define DFLOW_FLAG_KNN_EXACT 1   /* dflow_knn_proposals: brute-force VALU search instead of the MFMA-screened one (same
                                    results bit for bit; the cross-check of the screen's error bound) */

#define DFLOW_FLAG_DESCR_F16 8    /* BASELINE configs[4] "fp16 DAISY descriptors": dflow_daisy rounds the descriptor values to IEEE
                                    binary16 (round to nearest even) and stores them as binary16, (H,W,72) with 4 zero pads per
                                    pixel; dflow_knn_proposals / dflow_neighbour_proposals called with the flag read that layout.
                                    All arithmetic downstream (canonical float32 distance, costs, BCD) is on those values widened to
                                    float32; the reference has no such mode (cv2 returns float32) */
#define DFLOW_DESC_PITCH_F16 72  /* elements per pixel of a binary16 descriptor plane */

#define DFLOW_OK 0
#define DFLOW_EINVAL (-1)        /* bad parameter / null pointer / unsupported geometry */
#define DFLOW_ENOSPC (-2)        /* workspace too small */
#define DFLOW_EHIP (-3)          /* HIP runtime error (launch failure, no device) */

/* The reference starts the DP's fallback minimum (permmincost) and the end label's minimum at 800000.0 (python bcd.py:152-157,
 * :231), and the chain kernel takes the fallback minimum over the bit patterns of tpsi + dp, which order like the doubles only
 * while they are >= 0.  Every entry point therefore refuses (DFLOW_EINVAL) a lamda or tphi that is not finite or below 0, and
 * any parameter set with
 *     max(pich, picw) * (3*tpsi + lamda*tphi) >= DFLOW_DP_SENTINEL       (evaluated in double, tphi widened from float)
 * Within it, with data costs in [0, tphi]: the chain start is dp <= 2*tpsi + lamda*tphi, each step adds at most
 * tpsi (fallback) + 2*tpsi (side terms) + lamda*tphi, so 0 <= dp and tpsi + dp < DFLOW_DP_SENTINEL on every chain, and the
 * sentinels never bind: the kernel, the reference and the chain's Viterbi minimum agree.  At tpsi = 8 and 8192-pixel chains this
 * allows lamda*tphi up to about 73 (the reference constants give 0.125). */
#define DFLOW_DP_SENTINEL 800000.0

/* Algorithm constants.  Field-for-field the module globals of the reference scripts. */
typedef struct dflow_params {
    int32_t pich, picw;          /* daisy i flann.py:34-35 */
    int32_t cellh, cellw;        /* daisy i flann.py:42-43; ragged last row/column of cells absorbs the remainder */
    int32_t maxnprop;            /* daisy i flann.py:88   (150) */
    int32_t knn;                 /* daisy i flann.py:172  (5; kernels require 5) */
    int32_t window;              /* daisy i flann.py:167-168 (2 cells each side) */
    int32_t ngauss;              /* daisy i flann.py:207  (25) */
    int32_t tpsi;                /* daisy i flann.py:47   (8; kernels support 1..8) */
    int32_t max_attempts;        /* bound on draws per pixel in the neighbour sampler (65536) */
    float tphi;                  /* daisy i flann.py:46   (2.5; finite, >= 0, and see DFLOW_DP_SENTINEL) */
    float sigma;                 /* daisy i flann.py:208  (8)  */
    double lamda;                /* daisy i flann.py:48   (0.05; finite, >= 0, and see DFLOW_DP_SENTINEL) */
    uint64_t seed;               /* key of the counter-based sampler (reference: unseeded np.random, :219) */
    int32_t label_pitch;         /* LP, elements per pixel in proposals/lcosts (160; multiple of 16) */
    int32_t flags;               /* DFLOW_FLAG_* bits (0 = defaults); per call, the library keeps no process-global switches */
} dflow_params;

int dflow_version(void);
const char *dflow_last_error(void);

/* Fills *p with the reference constants for the given geometry. */
void dflow_default_params(dflow_params *p, int32_t pich, int32_t picw, int32_t cellh, int32_t cellw);

/* Scratch bytes any entry point may need for these parameters (one buffer serves all stages): the largest need of the main-path
 * stages (dflow_daisy_pair, dflow_knn_proposals where the screened search runs, dflow_neighbour_proposals, dflow_bcd_prepare and
 * the sweeps) plus 256 spare bytes.  A stage called with less than its own need answers DFLOW_ENOSPC and names that need. */
size_t dflow_workspace_bytes(const dflow_params *p);

/* izracunajDaisy, daisy i flann.py:69-77 (cv2.xfeatures2d.DAISY_create(radius=5,q_radius=4,q_theta=4,q_hist=4)
 * .compute on every pixel).  d_bgr (H,W,3) uint8 -> d_descr (H,W,68) float32 (binary16 (H,W,72) with DFLOW_FLAG_DESCR_F16). */
int dflow_daisy(const dflow_params *p, const uint8_t *d_bgr, void *d_descr,
                void *d_ws, size_t ws_bytes, void *stream);

/* The same for the two images of a pair (daisy i flann.py:406-407) in one set of launches: 7 kernels instead of 14, the image
 * as a grid dimension.  d_descr1 / d_descr2 are bit for bit what two dflow_daisy calls write; they must be two planes. */
int dflow_daisy_pair(const dflow_params *p, const uint8_t *d_bgr1, const uint8_t *d_bgr2, void *d_descr1, void *d_descr2,
                     void *d_ws, size_t ws_bytes, void *stream);

/* napraviCD2 + generisi, daisy i flann.py:144-189: per-cell exact 5-NN proposals, truncated-L1 costs,
 * WTA labels.  Initialises and fills proposals/lcosts/nprop/bestlabels. */
int dflow_knn_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2,
                        uint32_t *d_proposals, float *d_lcosts, int32_t *d_nprop, int32_t *d_bestlabels,
                        void *d_ws, size_t ws_bytes, void *stream);

/* Measurement aid (bench.py's roofline object): the launches of dflow_knn_proposals with HIP events between the kernels on
 * `stream`.  Same kernels, same results; unlike every other entry point it WAITS for the stream.  h_ms[6] (host) receives the
 * milliseconds of { basis (centre, covariance, principal axes), prep (both images), knn_screen_kernel, knn_resolve_kernel,
 * knn_fix_kernel, knn_finalize_kernel }, *h_mfma_issued (host, optional) the number of v_mfma_f32_32x32x16_f16 (32768 flop
 * each) the screen issues for these parameters.  No reference counterpart. */
int dflow_knn_proposals_timed(const dflow_params *p, const void *d_descr1, const void *d_descr2,
                              uint32_t *d_proposals, float *d_lcosts, int32_t *d_nprop, int32_t *d_bestlabels,
                              void *d_ws, size_t ws_bytes, void *stream, float *h_ms, double *h_mfma_issued);

/* Measurement aid (bench.py's other_configs, the low-texture tests): what the MFMA screen of the LAST dflow_knn_proposals call on
 * this workspace did, read back from the workspace (WAITS for the stream; call it before another stage reuses the workspace).
 * h_stats[DFLOW_KNN_STATS_N] (host): [0] event lists handed to the exact brute-force search (rows outside the f16 range / NaN, or
 * a lane's list ran out), [1] flags (bit 0: the whole pass went to the exact search: the basis failed its orthonormality check),
 * [2] event lists the workspace holds (every (query cell, 64-query wave, window slot), the unused ones of clipped windows and
 * smaller cells included), [3] list entries written, [4] events = (query, candidate) pairs evaluated exactly, [5] most entries in one lane's list,
 * [6] all-zero queries (answered from their cells' own lists), [7] queries outside the screen's range, [8] all-zero candidate
 * rows, [9] of those removed as duplicates, [10] (query, cell) pairs of the pass, [11] list capacity per lane, [12] (query, cell)
 * pairs with so many events that one wave took the query alone (its 64 lanes over the events).  [3], [4] and [5] count the
 * lists that did not run out ([0] counts those that did).
 * No reference counterpart. */
#define DFLOW_KNN_STATS_N 13
int dflow_knn_screen_stats(const dflow_params *p, void *d_ws, size_t ws_bytes, void *stream, int64_t *h_stats);

/* The same statistics followed by those added since, into a caller array of n_stats values (1 <= n_stats <=
 * DFLOW_KNN_STATS_ALL_N; the first n_stats are written): [0..12] as above, [13] (query, cell) pairs with that many events that
 * stayed in the lane-per-query kernel because the list of [12] was full.  dflow_knn_screen_stats keeps writing exactly
 * DFLOW_KNN_STATS_N values, the array size its callers were built with. */
#define DFLOW_KNN_STATS_ALL_N 14
int dflow_knn_screen_stats_n(const dflow_params *p, void *d_ws, size_t ws_bytes, void *stream, int64_t *h_stats, int n_stats);

/* nasumicni, daisy i flann.py:205-233: appends up to ngauss neighbour proposals per pixel (in place).
 * d_bestlabels must still hold the WTA labels written by dflow_knn_proposals.  Uses 4 bytes per pixel of the workspace
 * (the WTA flow of every pixel, gathered once). */
int dflow_neighbour_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2,
                              uint32_t *d_proposals, float *d_lcosts, int32_t *d_nprop,
                              const int32_t *d_bestlabels, void *d_ws, size_t ws_bytes, void *stream);

/* Builds the compat bit matrices of pakovanje (daisy i flann.py:256-309) into the workspace, in the layout the chain
 * kernel reads: per pixel, per chain direction and per label one record with the compatible labels of the predecessor
 * on that chain and their pairwise costs, plus per pixel every label's own flow and data cost (what ucitajSvePodatkeDoBCD,
 * python bcd.py:67-81, loads for bcd()).  Must be called after proposals and lcosts are final (after
 * dflow_neighbour_proposals / an upload) and before dflow_bcd_phase / dflow_bcd_sweep; the records stay valid until
 * another dflow_* stage call (daisy, knn) reuses the same workspace.  The costs of used slots (below nprop) must lie in
 * [0, tphi], which is what the kNN and neighbour stages write (min(tphi, a sum of absolute values)): the bound of
 * DFLOW_DP_SENTINEL assumes it, and uploaded costs outside it are not checked here (the host wrapper refuses them). */
int dflow_bcd_prepare(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                      void *d_ws, size_t ws_bytes, void *stream);

/* One of the four loops of ceoBCD's body, python bcd.py:265-277 (phase 0 even columns top->bottom,
 * 1 even rows right->left, 2 odd columns bottom->top, 3 odd rows left->right); every chain is one call of
 * bcd(), python bcd.py:101-257, reading the records dflow_bcd_prepare left in the workspace (label costs included).
 * Updates d_bestlabels in place. */
int dflow_bcd_phase(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop,
                    int32_t *d_bestlabels, int32_t phase, void *d_ws, size_t ws_bytes, void *stream);

/* One iteration of ceoBCD's loop (all four phases), python bcd.py:264-277. */
int dflow_bcd_sweep(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop,
                    int32_t *d_bestlabels, void *d_ws, size_t ws_bytes, void *stream);

/* The same loops for a BATCH of independent passes ((pair, direction) runs share nothing: README.md:40 of the reference)
 * with identical parameters: the chains of all npass passes go into one launch, which fills the GPU where one pass
 * alone (218-512 chains) cannot.  d_nprop / d_bestlabels / d_ws are HOST arrays of npass device pointers; every pass has its
 * own workspace of ws_bytes, prepared by dflow_bcd_prepare.  Results are identical to npass separate calls. */
int dflow_bcd_phase_batch(const dflow_params *p, int32_t npass, const int32_t *const *d_nprop, int32_t *const *d_bestlabels,
                          int32_t phase, void *const *d_ws, size_t ws_bytes, void *stream);
int dflow_bcd_sweep_batch(const dflow_params *p, int32_t npass, const int32_t *const *d_nprop, int32_t *const *d_bestlabels,
                          void *const *d_ws, size_t ws_bytes, void *stream);

/* How well the optimiser is doing: the energy of a labelling and the labels that differ from an earlier one (DESIGN.md "BCD
 * statistics and the stop rule").  No counterpart in the reference, which runs a fixed number of sweeps.
 * With l_p = d_bestlabels[p] and f_p the (dy, dx) of d_proposals[p][l_p], unpacked as everywhere else:
 *   smooth_sum     sum over the 4-adjacent pairs (p, right of p) and (p, below p) of min(tpsi, |f_p - f_q|_1); pixels of the
 *                  last column have no right pair, those of the last row no lower pair
 *   n_pairs_trunc  pairs with |f_p - f_q|_1 >= tpsi
 *   data_sum       sum over p of d_lcosts[p][l_p], each float32 widened to double, NOT multiplied by lamda
 *   n_data_trunc   pixels with d_lcosts[p][l_p] >= tphi (a float32 compare)
 *   n_changed      pixels with d_bestlabels[p] != d_prev_labels[p]; 0 when d_prev_labels is NULL
 *   n_bad_label    pixels with l_p < 0 or l_p >= d_nprop[p] (or >= label_pitch, which no slot lies beyond).  Such a pixel adds
 *                  1 to n_bad_label, 1 to n_changed (when d_prev_labels is given) and nothing else: it has no data cost, and
 *                  the pairs it is in are skipped
 * The image energy is E = lamda * data_sum + smooth_sum; the caller forms it on the host in double.  This is the energy
 * sum lamda lcost + sum_{4-adjacent} min(tpsi, |f_p - f_q|_1) of the whole labelling.  It is NOT the per-chain energy a phase
 * of the reference algorithm minimises (the side terms of a chain look along it at its own old labels, and its pair cost
 * forbids incompatible pairs where a compatible one exists), so E can rise in a phase and in a sweep.
 * d_prev_out (NULL to skip) receives a copy of d_bestlabels, bad labels included; it may be d_prev_labels itself, which then
 * holds the labels to compare the next sweep against.
 * Only pich, picw, maxnprop, label_pitch, tpsi and tphi of *p are read and checked: 1 <= pich, picw <= 8192 (a labelling needs
 * no cell grid), 1 <= maxnprop <= label_pitch <= DFLOW_MAX_LABELS, label_pitch a multiple of 16, 1 <= tpsi <= 8, tphi finite
 * and >= 0.
 * All integer fields are exact and independent of any order.  data_sum is a sum in double in the fixed order of
 * dflow_flow_eval (per lane, a fixed tree per block, the blocks' partial sums in block order in a second launch; no floating
 * atomics): the same inputs give the same 8 bytes on every call.
 * dflow_bcd_stats_batch does the same for npass passes of identical parameters in one pair of launches per 8 passes, the
 * pass as a grid dimension: the arrays are HOST arrays of npass device pointers (as for dflow_bcd_sweep_batch); d_prev[i] is
 * both d_prev_labels and d_prev_out of pass i, the array or any entry may be NULL; d_stats[i] receives, byte for byte, what
 * the single call writes for pass i.  Its workspace is npass times dflow_bcd_stats_workspace_bytes.
 * A bad parameter, a NULL required pointer (every one but d_prev_labels, d_prev_out, d_prev and its entries), a d_stats or
 * d_ws that is not 8-byte aligned (both hold doubles) or an npass outside [1, 1024] returns DFLOW_EINVAL, a NULL or too small
 * workspace DFLOW_ENOSPC, both before anything is launched.  The calls are asynchronous on `stream`, allocate nothing, read nothing back and can be captured into a graph.
 * The workspace is the calls' own (one partial result per block of the first launch, at most 32 KiB per pass): the records
 * dflow_bcd_prepare left in the passes' workspaces are neither read nor written, so statistics may be taken between sweeps.
 * dflow_bcd_stats_workspace_bytes returns 0 (and sets dflow_last_error) for parameters outside the range. */
struct dflow_bcd_stats {        /* no typedef: the entry point has the name, so write `struct dflow_bcd_stats` */
    uint64_t smooth_sum, n_pairs_trunc, n_data_trunc, n_changed, n_bad_label;
    double data_sum;
};
size_t dflow_bcd_stats_workspace_bytes(const dflow_params *p);
int dflow_bcd_stats(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                    const int32_t *d_bestlabels, const int32_t *d_prev_labels, int32_t *d_prev_out,
                    struct dflow_bcd_stats *d_stats, void *d_ws, size_t ws_bytes, void *stream);
int dflow_bcd_stats_batch(const dflow_params *p, int32_t npass, const uint32_t *const *d_proposals, const float *const *d_lcosts,
                          const int32_t *const *d_nprop, const int32_t *const *d_bestlabels, int32_t *const *d_prev,
                          struct dflow_bcd_stats *d_stats, void *d_ws, size_t ws_bytes, void *stream);

/* vratiKonacniFlow, python bcd.py:90-95 / daisy i flann.py:192-197. */
int dflow_labels_to_flow(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_bestlabels,
                         float *d_flow, void *stream);

/* postProcessing = FlowImage.ucitajFlow x2 + fowardBackwardConsistency, postprocessing.py:7-17,79-135
 * (including its transposed indexing).  d_fwd/d_bwd (H,W,2) [dy,dx] -> d_sparse (H,W,3) [U,V,valid]. */
int dflow_fb_consistency(const dflow_params *p, const float *d_fwd, const float *d_bwd, float tresh,
                         float *d_sparse, void *stream);

/* The packedksets file of pakovanje, daisy i flann.py:256-309, for users who feed the reference's own `python bcd.py`:
 * d_packed (H,W,2,maxnprop*maxnprop/8+1) uint8, slot 0 = pixel vs the pixel below, slot 1 = vs the pixel to the right,
 * np.packbits bit order.  Every matrix is computed from clean scratch; the reference's bottom-row / right-column loops
 * (:283-307) reuse theirs, which the host wrapper (compat.py) replays on those H+W matrices. */
int dflow_pack_compat(const dflow_params *p, const uint32_t *d_proposals, const int32_t *d_nprop, uint8_t *d_packed,
                      void *stream);

/* removeSmallSegments, postprocessing.py:29-76 (unused upstream, :129), on a HOST (dim0,dim1,3) float32 [U,V,valid]
 * field, in place.  Host code: the reference's region growing depends on its scan order. */
int dflow_remove_small_segments_host(float *h_sparse, int32_t dim0, int32_t dim1, float tresh, int32_t min_segment_size);

/* Canny edge map, canny_ivice, edge.py:19-35: cv2.cvtColor(BGR2GRAY) -> cv2.GaussianBlur(gray, (3,3), 0) ->
 * cv2.Canny(threshold1=low, threshold2=high) (aperture 3, L1 gradient) -> np.array((255 - edges) / 255, float32), the
 * ivice.bin that spremiZaEpic.py:26 hands to epicflow-static.  Plain sizes instead of dflow_params: an edge map is not tied
 * to the flow geometry.  1 <= h, w <= 8192; low, high finite and >= 0 (swapped when low > high, then floored).
 * d_bgr (h,w,3) uint8 BGR -> d_edges (h,w) uint8 0/255 (required) and, if d_ivice is not NULL, d_ivice (h,w) float32 = 0.0 on
 * edges, 1.0 elsewhere.  Integer arithmetic restated from the algorithm; parity with a cv2 build is not pinned (DESIGN.md
 * "Canny edge maps").  dflow_canny_workspace_bytes returns 0 (and sets dflow_last_error) for sizes outside the range. */
size_t dflow_canny_workspace_bytes(int32_t h, int32_t w);
int dflow_canny_edges(int32_t h, int32_t w, const uint8_t *d_bgr, double low, double high, uint8_t *d_edges, float *d_ivice,
                      void *d_ws, size_t ws_bytes, void *stream);

/* Soft edge strength without a trained model: a Pb-style oriented half-disc histogram gradient (Martin, Fowlkes, Malik, PAMI
 * 2004: brightness and colour gradient as the chi^2 distance between the histograms of the two halves of a disc).  This
 * build's own definition (DESIGN.md "Pb edge strength"), not bit-matched to any binary; it stands in for the reference's
 * structured edge detector (sed_ivice, edge.py:4-17), whose trained model the reference does not ship.
 * d_bgr (h,w,3) uint8 BGR, 1 <= h, w <= 8192; 1 <= radius R <= DFLOW_PB_MAX_RADIUS.
 * 1. Channels, integers in 0..255, per pixel: c0 = the fixed-point BGR2GRAY of the Canny entry, (1868 B + 9617 G + 4899 R +
 *    8192) >> 14; c1 = (R - G + 255) >> 1; c2 = (2 B - R - G + 510) >> 2.  Bin = c >> 4: 16 bins.
 * 2. Disc: the offsets (dx,dy) with 0 < dx^2 + dy^2 <= R^2; a pixel outside the frame is read at the clamped coordinate
 *    (replicate border).
 * 3. Orientations o = 0..7 have the integer normals (nx,ny) = (1,0), (2,1), (1,1), (1,2), (0,1), (-1,2), (-1,1), (-2,1).  An
 *    offset is on side A of o when dx nx + dy ny > 0, on side B when it is < 0, on neither side when it is 0.  The disc is
 *    point-symmetric: both sides hold the same number N_o(R) of offsets.
 * 4. For channel c and orientation o, with G_b, H_b the integer counts of bin b on side A and side B,
 *    chi_{c,o} = (sum over b = 0..15 with G_b + H_b > 0 of (G_b - H_b)^2 / (G_b + H_b)) / (2 N_o), in [0,1]: the sum in
 *    ascending b in float32, every numerator and denominator converted exactly from an integer, one IEEE operation per
 *    written operation.
 * 5. m_o = (2 chi_{0,o} + chi_{1,o} + chi_{2,o}) / 4, in that order in float32; e = max over o of m_o.  No non-maximum
 *    suppression and no gain: a constant image gives exactly 0.0 everywhere.
 * d_strength (h,w) float32 e (required); d_orient_strength (h,w,8) float32 m_o (optional, NULL to skip; e is the same
 * either way).  A size or radius outside its range or a NULL required pointer returns DFLOW_EINVAL, a NULL or too small
 * workspace DFLOW_ENOSPC, both before anything is launched.  The call is asynchronous on `stream`, allocates nothing, reads
 * nothing back and can be captured into a graph.  The workspace is 2 bytes per pixel; dflow_pb_workspace_bytes returns 0
 * (and sets dflow_last_error) for sizes outside the range. */
#define DFLOW_PB_MAX_RADIUS 7
size_t dflow_pb_workspace_bytes(int32_t h, int32_t w);
int dflow_pb_edges(int32_t h, int32_t w, const uint8_t *d_bgr, int32_t radius, float *d_strength, float *d_orient_strength,
                   void *d_ws, size_t ws_bytes, void *stream);

/* Edge-aware interpolation of a sparse flow field: EpicFlow's sparse-to-dense step (Revaud et al., CVPR 2015), with integer
 * geodesics so that the result is unique (DESIGN.md "EpicFlow interpolation").  1 <= h, w <= 8192.
 * d_sparse (h,w,3) float32 [U,V,valid] (what dflow_fb_consistency writes): a seed is a pixel with valid > 0.5 and finite U,
 * V; its id is y*w + x.  d_edges (h,w) float32 edge strength e = clamp(E, 0, 1), NaN read as 1; pixel cost
 * c = 1 + rint(1000 e) in float32.  S, D: the 4-connected geodesic Voronoi diagram with step cost c(p) + c(q), the
 * lexicographic minimum of (D, seed id).  The seed graph joins the seeds of 4-neighbours p, q with weight
 * D(p) + c(p) + c(q) + D(q); every seed keeps its nn nearest seeds by (G, id), G the graph distance, itself first, and fits
 * with weights exp(-k G / 2000) either a Nadaraya-Watson mean (DFLOW_EPIC_NW) or a locally-weighted affine model
 * (DFLOW_EPIC_LA; the mean when fewer than 3 seeds are listed or the smallest eigenvalue of their weighted position
 * covariance is below DFLOW_EPIC_TAU px^2).  Every pixel takes the model of its seed: d_flow (h,w,2) float32 [dy,dx].
 * 1 <= nn <= 256; k finite and > 0; with no seed the flow is all zeros.
 * Optional outputs (NULL to skip): d_seed_of (h,w) S (-1 without seeds), d_dist (h,w) D (0xFFFFFFFF without seeds),
 * d_lists (h*w, nn) int32 and d_list_g (h*w, nn) uint64: row y*w + x lists the seed's neighbours and their G in order,
 * padded with -1 / UINT64_MAX; the rows of non-seed pixels are all padding.
 * The call reads a change counter back after every few Voronoi rounds, so it synchronises its stream and cannot be
 * captured into a graph.  The workspace grows linearly with h*w; the workspace-size function returns 0 (and sets
 * dflow_last_error) for sizes outside the range.  dflow_epic_last_stats reports the Voronoi rounds and the HIP-event
 * times of the last call on the calling thread: stage_ms[4] = seed init + Voronoi, seed graph, lists + models, dense fill. */
#define DFLOW_EPIC_LA 0
#define DFLOW_EPIC_NW 1
#define DFLOW_EPIC_TAU 1e-3
size_t dflow_epic_workspace_bytes(int32_t h, int32_t w);
int dflow_epic_interpolate(int32_t h, int32_t w, const float *d_sparse, const float *d_edges, int32_t nn, double k,
                           int32_t method, float *d_flow, int32_t *d_seed_of, uint32_t *d_dist, int32_t *d_lists,
                           uint64_t *d_list_g, void *d_ws, size_t ws_bytes, void *stream);
int dflow_epic_last_stats(int32_t *rounds, float *stage_ms);

/* EpicFlow's match pre-filter, the step epicflow-static takes before it interpolates: this build's own definition (DESIGN.md
 * "EpicFlow interpolation", "Match pre-filter"), not bit-matched to that binary.  The defaults the callers use (saliency_th
 * 0.045, pref_nn 25, pref_th 5, image smoothing sigma 0.8, tensor smoothing sigma 1.0) are EpicFlow's as
 * recalled, not checked against the binary.  1 <= h, w <= 8192.  Seeds, d_edges, the Voronoi diagram, the seed graph, G and k
 * as above.
 * Stage A, saliency (skipped when saliency_th == 0; d_bgr may then be NULL and is not read): every channel of d_bgr (h,w,3)
 * uint8 BGR as float32, smoothed by the separable Gaussian of the variational refinement (sigma 0.8), central differences
 * 0.5 (f[+1] - f[-1]) with a replicate border, the structure tensor summed over the channels, its three planes smoothed
 * (sigma 1.0), s = sqrt(max(0, lambda_min)), all float32.  A seed with s < saliency_th (s widened to double) is dropped,
 * reason 2.
 * Stage B, neighbour consistency (skipped when pref_nn == 0), over the seeds left: every seed lists its pref_nn + 1 nearest
 * seeds by (G, id), itself first, and forms the Nadaraya-Watson estimate (u^, v^) of the others with weights exp(-k G / 2000),
 * in double in list order; it is dropped, reason 3, when (u^ - u)^2 + (v^ - v)^2 > pref_th^2 in double.  A seed that reaches
 * no other seed is kept (its estimate is its own flow), and so is one whose estimate is not a number (every weight 0).
 * All seeds are judged against the same set: the result does not depend on any order.
 * d_sparse_out (h,w,3): d_sparse_in with every dropped seed set to [0,0,0]; it may be d_sparse_in itself.  Optional outputs
 * (NULL to skip): d_reason (h,w) uint8, 0 no seed, 1 kept, 2 saliency, 3 consistency; d_saliency (h,w) float32 s (zeros when
 * stage A is skipped); d_estimate (h,w,2) float32 [u^, v^] at the seeds of stage B, 0 elsewhere.
 * 0 <= pref_nn <= 255; saliency_th, pref_th finite and >= 0; k finite and > 0.  A value outside these bounds, a NULL required
 * pointer or a NULL d_bgr with saliency_th != 0 returns DFLOW_EINVAL, a NULL or too small workspace DFLOW_ENOSPC, both before
 * anything is launched.  Like the interpolation the call reads the Voronoi change counters back, and its own three counters at
 * the end: it synchronises its stream and cannot be captured into a graph.  The workspace grows linearly with h*w; the
 * workspace-size function returns 0 (and sets dflow_last_error) for sizes outside the range.
 * dflow_epic_prefilter_last_stats: of the last call on the calling thread, counts[3] = seeds in, dropped by stage A, dropped
 * by stage B, and the HIP-event times stage_ms[4] = stage A, Voronoi + seed graph, consistency, compaction (either may be
 * NULL). */
size_t dflow_epic_prefilter_workspace_bytes(int32_t h, int32_t w);
int dflow_epic_prefilter(int32_t h, int32_t w, const uint8_t *d_bgr, const float *d_sparse_in, const float *d_edges,
                         double saliency_th, int32_t pref_nn, double pref_th, double k, float *d_sparse_out, uint8_t *d_reason,
                         float *d_saliency, float *d_estimate, void *d_ws, size_t ws_bytes, void *stream);
int dflow_epic_prefilter_last_stats(int32_t *counts, float *stage_ms);

/* Variational refinement of a dense flow: the second half of EpicFlow (Revaud et al., CVPR 2015, section 4, after Brox et al.,
 * ECCV 2004): a one-level minimisation of a robust, normalised gradient- (gamma) and colour-constancy (delta) energy with an
 * image-driven smoothness term (alpha), started from d_flow_in.  This build's own definition (DESIGN.md "Variational
 * refinement"): niter_outer warps, niter_inner updates of the lagged weights per warp, niter_solver iterations of RED-BLACK SOR
 * per update, so the result is a function of the inputs alone; it is not bit-matched to epicflow-static, and the defaults are
 * EpicFlow's documented ones as recalled, not checked against that binary.  1 <= h, w <= 8192.
 * d_bgr1, d_bgr2 (h,w,3) uint8 BGR; d_flow_in, d_flow_out (h,w,2) float32 [dy,dx], which may be the same buffer.  A pixel
 * whose flow is not finite is treated as unmatched in the data term (it is sampled at itself), but the smoothness term still
 * reads it.  alpha, gamma, delta finite and >= 0; sigma (Gaussian presmoothing) in [0,5]; sor_omega in (0,2); niter_outer in
 * 0..1000 (0: the output is a copy of the input); niter_inner in 1..1000; niter_solver in 1..10000.
 * A value outside these bounds, a NULL pointer or an unknown flag bit returns DFLOW_EINVAL; a NULL or too small workspace
 * returns DFLOW_ENOSPC, as for every stage; both before anything is launched.  The Gaussian taps are computed in double from
 * the float32 sigma the struct carries.  dflow_var_default_params ignores a NULL p.
 * DFLOW_VAR_FLAG_SOR_UNFUSED runs the solver as one launch per half-sweep instead of the LDS-tiled kernel that does 8 per
 * launch: the same result bit for bit (the cross-check and A/B partner).  The call is asynchronous on `stream` and reads
 * nothing back.  The workspace grows linearly with h*w; the workspace-size function returns 0 (and sets dflow_last_error) for
 * sizes outside the range. */
#define DFLOW_VAR_FLAG_SOR_UNFUSED 1u
typedef struct dflow_var_params {
    float alpha, gamma, delta, sigma, sor_omega;
    int32_t niter_outer, niter_inner, niter_solver;
    uint32_t flags;
} dflow_var_params;
void dflow_var_default_params(dflow_var_params *p);
size_t dflow_var_workspace_bytes(int32_t h, int32_t w);
int dflow_var_refine(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2, const float *d_flow_in,
                     const dflow_var_params *p, float *d_flow_out, void *d_ws, size_t ws_bytes, void *stream);

/* Flow evaluation: how far a flow field is from the ground truth, after errorImage of the reference's visualization.py:128-156
 * (mean end-point error, percentage of outliers, colour error picture).  This build's definition (DESIGN.md "Flow
 * evaluation").  1 <= h, w <= 8192; the planes are walked as h*w pixels in row-major order.
 * d_gt (h,w,3) float32 [U,V,valid].  d_test, by test_layout: DFLOW_EVAL_UVV (h,w,3) float32 [U,V,valid], what
 * dflow_fb_consistency writes and the KITTI reader gives; DFLOW_EVAL_DYDX (h,w,2) float32 [dy,dx] (U = dx, V = dy), every pixel
 * valid: what the dense stages write.  d_test, d_gt and d_err must be 16-byte aligned, d_stats 8-byte, d_err_bgr 4-byte.
 * Which pixels count: a pixel is COMPARED when gt.valid > 0.5 and test.valid > 0.5 (a NaN valid compares false).  n_gt_valid
 * and n_test_valid count the two masks on their own (n_test_valid = h*w under DFLOW_EVAL_DYDX).
 * Per compared pixel, in float32, one correctly rounded IEEE operation per written operation (no fused multiply-add):
 *     dfu = tU - gU, dfv = tV - gV, err = sqrt(dfu*dfu + dfv*dfv)
 * the bits numpy gives.  If err is not finite (NaN or Inf) the pixel adds 1 to n_nonfinite and to nothing else.  Otherwise it
 * adds 1 to n, err (widened to double) to sum_err, and max_err = max(max_err, err); 1 to n_out_abs when err > abs_thresh
 * (the reference: 3); 1 to n_out_kitti when err > 3 and err > 0.05f * sqrt(gU*gU + gV*gV) in float32: KITTI's 3 px / 5 % rule.
 * Mean end-point error = sum_err / n; the reference's outlier percentage = n_out_abs * 100 / n.
 * Optional outputs (NULL to skip):
 *   d_err (h,w) float32: err at compared pixels, whatever it is (a NaN as the quiet NaN 0x7FC00000, an infinity as +Inf);
 *     -1 at all others.
 *   d_err_bgr (h,w,3) uint8: the reference's error picture in the channel order it hands to imwrite.  At a pixel counted in
 *     n: t = min(err, 3) / 3, idx = min(255, (int)(t * 256)), both float32, and the bytes are (b, g, r) of LUT[idx], LUT being
 *     matplotlib's 256-entry 'jet' as uint8(value * 255) (csrc/jet_lut.h: jet's segment data interpolated linearly at
 *     linspace(0,1,256) in float64; the entry matplotlib's cmap(t) picks for a float32 t).  (0,0,0) at every other pixel, the
 *     non-finite ones included.
 * Statistics: the counts and max_err are exact and independent of any order.  sum_err is a sum of float32 values in double in
 * a fixed order (per lane, a fixed tree per block, the blocks' partial sums in block order in a second launch; no floating
 * atomics): the same inputs give the same 8 bytes on every call.  Without DFLOW_EVAL_FLAG_ACCUMULATE *d_stats is
 * overwritten (max_err = 0 when n = 0); with it the call's values are added to what *d_stats holds (max_err by max, sum_err
 * as old + this call's sum), so a batch totals its pairs on the device and reads back once; the caller zeroes it first.
 * An unknown flag bit or layout, an abs_thresh that is not finite or is negative, a NULL or misaligned d_test, d_gt or
 * d_stats, a misaligned optional output or a size out of range returns DFLOW_EINVAL, a NULL or too small workspace
 * DFLOW_ENOSPC, both before anything is launched.  The call is asynchronous on `stream`, allocates nothing, reads nothing
 * back and can be captured into a graph.  The workspace holds one partial result per block of the first launch, a fixed
 * function of h*w; dflow_eval_workspace_bytes returns 0 (and sets dflow_last_error) for sizes outside the range. */
#define DFLOW_EVAL_UVV  0
#define DFLOW_EVAL_DYDX 1
#define DFLOW_EVAL_FLAG_ACCUMULATE 1u
typedef struct dflow_eval_stats {
    uint64_t n, n_out_abs, n_out_kitti, n_nonfinite, n_gt_valid, n_test_valid;
    double sum_err;
    float max_err; uint32_t reserved;
} dflow_eval_stats;
size_t dflow_eval_workspace_bytes(int32_t h, int32_t w);
int dflow_flow_eval(int32_t h, int32_t w, const float *d_test, int32_t test_layout, const float *d_gt, float abs_thresh,
                    uint32_t flags, dflow_eval_stats *d_stats, float *d_err, uint8_t *d_err_bgr,
                    void *d_ws, size_t ws_bytes, void *stream);

/* Looking at a flow without a ground truth: its colour picture, and the second image warped back onto the first with the
 * photometric error that results.  This build's definitions (DESIGN.md "Flow pictures and the warp check"); no counterpart
 * in the reference.  Common to both entry points: 1 <= h, w <= 8192, the planes are walked as h*w pixels in row-major order;
 * d_flow by `layout` is DFLOW_EVAL_UVV (h,w,3) float32 [U,V,valid] or DFLOW_EVAL_DYDX (h,w,2) float32 [dy,dx] (U = dx, V = dy,
 * valid = 1), as for dflow_flow_eval.  A pixel is KNOWN when valid > 0.5 and |U| <= 1e9 and |V| <= 1e9 (float32 compares, so
 * a NaN or an infinity anywhere makes it unknown); every other pixel is UNKNOWN.  d_flow and d_err must be 16-byte aligned,
 * d_stats 8-byte, the uint8 planes the kernels move four pixels at a time (d_bgr of the colour picture, d_bgr1, d_warped,
 * d_err_bgr) and d_maxrad 4-byte; d_bgr2 is read byte by byte.  A size, layout, flag or parameter outside its range, a NULL
 * required pointer or a misaligned pointer returns DFLOW_EINVAL, a NULL or too small workspace DFLOW_ENOSPC, both before
 * anything is launched.  Both calls are asynchronous on `stream`, allocate nothing, read nothing back and can be captured
 * into a graph; their workspace holds one partial result per block of the first launch, a fixed function of h*w, and the
 * *_workspace_bytes functions return 0 (and set dflow_last_error) for sizes outside the range.
 *
 * dflow_flow_color: the Middlebury colour coding (Baker et al., "A Database and Evaluation Methodology for Optical Flow",
 * the colorcode of its flow tools), written from the published algorithm as recalled and not checked against that tool.
 * The wheel has 55 entries (r,g,b), csrc/flow_wheel.h, in the order RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; with i counting
 * within a segment of length n and integer divisions: RY (255, 255*i/n, 0), YG (255 - 255*i/n, 255, 0), GC (0, 255, 255*i/n),
 * CB (0, 255 - 255*i/n, 255), BM (255*i/n, 0, 255), MR (255, 0, 255 - 255*i/n).
 * Radius: max_flow > 0: maxrad = max_flow.  max_flow == 0: maxrad = the maximum over the known pixels of sqrtf(U*U + V*V) in
 * float32, and 1 when that is 0 or no pixel is known; it is found by a first launch and read from the workspace by the one
 * that colours.  Any other max_flow (negative, NaN, Inf) is DFLOW_EINVAL.  d_maxrad (device float, NULL to skip) receives it.
 * Per known pixel, in double, one correctly rounded IEEE operation per written operation, no fused multiply-add:
 *     fx = U / maxrad, fy = V / maxrad, rad = sqrt(fx*fx + fy*fy)
 *     a = atan2(-fy, -fx) / pi, fk = (a + 1) / 2 * 54, k0 = min(54, (int)floor(fk)), k1 = (k0 + 1) % 55, f = fk - k0
 *     per channel: c0 = wheel[k0] / 255, c1 = wheel[k1] / 255, col = c0 + f * (c1 - c0)
 *                  col = 1 - rad * (1 - col) when rad <= 1, col * 0.75 otherwise;  byte = (int)(255 * col)
 * Everything but atan2 is determined to the bit; a channel whose two wheel entries are equal is exact whatever f is.
 * d_bgr (h,w,3) uint8 in (b, g, r) order, as d_err_bgr; (0,0,0) at unknown pixels. */
size_t dflow_flow_color_workspace_bytes(int32_t h, int32_t w);
int dflow_flow_color(int32_t h, int32_t w, const float *d_flow, int32_t layout, float max_flow, uint8_t *d_bgr,
                     float *d_maxrad, void *d_ws, size_t ws_bytes, void *stream);

/* dflow_warp_eval: d_bgr1, d_bgr2 (h,w,3) uint8 BGR, the two frames; the flow takes pixel (x,y) of the first to
 * (x + U, y + V) in the second.  Per known pixel, in float32, one IEEE operation per written operation:
 *     xs = x + U, ys = y + V;  the pixel is INSIDE when 0 <= xs <= w-1 and 0 <= ys <= h-1
 *     x0 = floorf(xs), ax = xs - x0, x1 = min(x0 + 1, w-1), and likewise y0, ay, y1
 *     per channel: top = (1-ax)*I2[y0][x0] + ax*I2[y0][x1], bot the same on row y1, wv = (1-ay)*top + ay*bot
 *     err = ((|wv_b - I1_b| + |wv_g - I1_g|) + |wv_r - I1_r|) / 3
 * (the bilinear operation order of the variational refinement's warp).  Statistics: n counts the inside pixels, n_outside
 * the known pixels that are not inside, n_unknown the unknown ones (the three add up to h*w), n_above the inside pixels
 * with err > err_thresh; sum_err adds err widened to double in the fixed order of dflow_flow_eval (the same inputs give the
 * same 8 bytes on every call), max_err is the largest err (0 when n = 0).  Mean photometric error = sum_err / n.  Without
 * DFLOW_WARP_FLAG_ACCUMULATE *d_stats is overwritten; with it the call's values are added to what it holds (max_err by
 * max, sum_err as old + this call's sum); the caller zeroes it first.
 * Optional outputs (NULL to skip): d_warped (h,w,3) uint8 (int)floorf(wv + 0.5f), (0,0,0) where the pixel is not inside;
 * d_err (h,w) float32 err, -1 where the pixel is not inside; d_err_bgr (h,w,3) uint8: the jet table of dflow_flow_eval at
 * idx = min(255, (int)(t * 256)), t = min(err, err_max) / err_max, black where the pixel is not inside.
 * err_thresh finite and >= 0, err_max finite and > 0. */
#define DFLOW_WARP_FLAG_ACCUMULATE 1u
typedef struct dflow_photo_stats {
    uint64_t n, n_outside, n_unknown, n_above;
    double sum_err;
    float max_err; uint32_t reserved;
} dflow_photo_stats;
size_t dflow_warp_eval_workspace_bytes(int32_t h, int32_t w);
int dflow_warp_eval(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2, const float *d_flow, int32_t layout,
                    float err_thresh, float err_max, uint32_t flags, dflow_photo_stats *d_stats, uint8_t *d_warped,
                    float *d_err, uint8_t *d_err_bgr, void *d_ws, size_t ws_bytes, void *stream);

/* Starting a pass from a flow somebody already has (the previous pair's flow, the inverse of the other direction's, a coarse
 * estimate (dflow_flow_upsample, below, makes one from a half-size level), a sparse ground truth): dflow_prior_proposals appends
 * the prior's vectors to the pixels' label sets and may start the labelling on them; dflow_flow_advance makes such a prior out
 * of a flow.  This build's definitions (DESIGN.md "Prior proposals"); no counterpart in the reference, whose label sets hold kNN
 * matches within +-window cells and copies of neighbouring winners only.  A prior label competes on its DAISY cost like every
 * other; the label space is integer.
 *
 * A VECTOR of a flow plane is USABLE (both entry points): under DFLOW_EVAL_UVV (H,W,3) [U,V,valid] the pixel needs valid > 0.5
 * (a NaN compares false) and dy = V, dx = U; under DFLOW_EVAL_DYDX (H,W,2) [dy,dx] every pixel is valid.  (dy,dx) = rintf of the
 * two components (ties to even); the vector is unusable if a component is not finite or a rounded component lies outside
 * [-32767, 32767] (32767.4 is usable, 32767.5 and 32767.6 are not, nor is -32768).
 *
 * dflow_prior_proposals.  Runs after dflow_neighbour_proposals (the neighbour kernel does not bound nprop itself, so never
 * between it and dflow_knn_proposals); needs no workspace and leaves the caller's alone, but the records of dflow_bcd_prepare
 * describe the old label sets: prepare again before the next sweep.  d_descr1 / d_descr2 as for the kNN stage (binary16 with
 * DFLOW_FLAG_DESCR_F16).  Every pixel (y,x) is handled on its own.  Its candidates are k = 0..4 with the source offsets (oy,ox)
 * = (0,0), (-s,0), (0,-s), (0,+s), (+s,0), s = stride; with s = 0 only k = 0 exists.  They are taken in that order, with
 * n = nprop[y,x] as it stands at that moment:
 *   1. the source (y+oy, x+ox) lies outside the frame: SKIPPED;
 *   2. the prior's vector at the source is not usable: SKIPPED;
 *   3. the target (y+dy, x+dx) lies outside the frame: SKIPPED;
 *   4. the packed label equals proposals[y,x,j] for some j < n (both halves equal: not the component-wise `in` of nasumicni;
 *      a label appended for an earlier candidate of this pixel counts): FOUND, slot = the smallest such j;
 *   5. otherwise, if n < maxnprop: APPENDED, slot = n, proposals[y,x,n] = the label, lcosts[y,x,n] = l1 < tphi ? l1 : tphi with
 *      l1 = sum_k |descr1[y,x][k] - descr2[target][k]| in numpy's float32 pairwise order, the kNN stage's cost (8 running sums,
 *      the tree, then the 4-element tail; not the neighbour stage's |sum(a-b)|), nprop[y,x] = n + 1; a NaN l1 gives tphi, so the
 *      costs of used slots stay in [0, tphi] (DFLOW_DP_SENTINEL);
 *   6. otherwise the row is FULL and nothing happens for this candidate;
 *   7. if k = 0 was found or appended and DFLOW_PRIOR_SEED_LABELS is set: bestlabels[y,x] = slot.
 * Slots at or above nprop keep what they hold (the fills).  d_counts (NULL to skip) receives int32 {appended, found, full,
 * skipped} over all (pixel, candidate), which add up to H*W*(s ? 5 : 1); the call zeroes them itself, on the stream (integer
 * atomics: exact in any order).  The results do not depend on any order and a second identical call changes nothing.
 * DFLOW_EINVAL before anything is launched: whatever dflow_check_params refuses, a layout other than the two, a stride outside
 * [0, 8192], an unknown flag bit, a NULL pointer (d_counts excepted), d_descr1, d_descr2 or d_proposals not 16-byte aligned,
 * another pointer not 4-byte aligned, d_prior equal to one of the other pointers.  Asynchronous on `stream`, allocates nothing,
 * reads nothing back, can be captured into a graph. */
#define DFLOW_PRIOR_SEED_LABELS 1u
int dflow_prior_proposals(const dflow_params *p, const void *d_descr1, const void *d_descr2,
                          const float *d_prior, int32_t layout, int32_t stride, uint32_t flags,
                          uint32_t *d_proposals, float *d_lcosts, int32_t *d_nprop, int32_t *d_bestlabels,
                          int32_t *d_counts /* NULL or int32[4] */, void *stream);

/* dflow_flow_advance carries every vector to the pixel it points at: the flow of t -> t+1 becomes a prior for t+1 -> t+2
 * (constant velocity), and with DFLOW_ADVANCE_NEGATE a prior for the backward pass (the inverse flow).  1 <= h, w <= 8192.
 * A source with raster index i = y*w + x TAKES PART if its vector is usable (above) and its target (y+dy, x+dx) lies inside the
 * frame.  Each target takes the claimant with the smallest i; its output is [dx, dy, 1], the integers as floats, with NEGATE
 * [(float)(-dx), (float)(-dy), 1] (the integer is negated, so 0 stays +0.0).  A target nobody claims gets [0,0,0].  d_out is
 * (h,w,3) float32 [U,V,valid]; d_counts (NULL to skip) receives int32 {claimed targets, claimants that lost, sources that did
 * not take part}, which add up to h*w.  The workspace holds a uint32 winner per pixel, set to 0xFFFFFFFF, written with
 * atomicMin and resolved by a second launch: the result does not depend on the order of arrival.
 * A size, layout or flag outside its range, a NULL d_flow or d_out, a pointer that is not 4-byte aligned or d_out == d_flow
 * returns DFLOW_EINVAL, a NULL or too small workspace DFLOW_ENOSPC, both before anything is launched.  Asynchronous on
 * `stream`, allocates nothing, reads nothing back, can be captured into a graph; dflow_flow_advance_workspace_bytes returns 0
 * (and sets dflow_last_error) for sizes outside the range. */
#define DFLOW_ADVANCE_NEGATE 1u
size_t dflow_flow_advance_workspace_bytes(int32_t h, int32_t w);
int dflow_flow_advance(int32_t h, int32_t w, const float *d_flow, int32_t layout, uint32_t flags,
                       float *d_out /* (H,W,3) [U,V,valid] */, int32_t *d_counts /* NULL or int32[3] */,
                       void *d_ws, size_t ws_bytes, void *stream);

/* Coarse to fine (DESIGN.md "Coarse to fine"): the two image-plane steps that connect two levels of a pyramid.  A level of
 * size (h,w) has the coarser level (hc,wc) = ((h+1)/2, (w+1)/2) above it; coarse pixel j sits at fine position 2j.  This build's
 * definitions; the reference runs one level and has no counterpart.  Both: 1 <= h, w <= 8192, asynchronous on `stream`, allocate
 * nothing, need no workspace, read nothing back, can be captured into a graph; every refusal happens before anything is launched.
 *
 * dflow_pyr_down makes the next coarser level of one image, or of the two images of a pair in one launch (d_in2 and d_out2 both
 * NULL or both given).  d_in* (h,w,3) uint8 BGR, d_out* (hc,wc,3) uint8.  With k = [1,4,6,4,1], i, j = -2..2 and the border
 * replicated:
 *     out[y][x][c] = (sum_i sum_j k_i k_j in[clamp(2y+i, 0, h-1)][clamp(2x+j, 0, w-1)][c] + 128) >> 8
 * in integers, with the one rounding at the end (the kernel forms the sum separably, which changes nothing).  A constant image
 * stays constant; 255 stays 255.  The planes of a pair equal those of two single calls.
 * DFLOW_EINVAL: a size outside the range, a NULL d_in1 or d_out1, only one of d_in2 / d_out2 given, a pointer that is not 4-byte
 * aligned, an output that is an input, d_out1 == d_out2.
 *
 * dflow_flow_upsample turns the flow of the coarser level into a prior for level (h,w): d_coarse (hc,wc,.) float32 in
 * DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout, d_out (h,w,3) float32 [U,V,valid], what dflow_prior_proposals reads under
 * DFLOW_EVAL_UVV.  A coarse vector is GOOD when it is valid (valid > 0.5 under UVV, always under DYDX) and both components are
 * finite.  For fine pixel (y,x): y0 = y>>1, y1 = min((y+1)>>1, hc-1), x0 = x>>1, x1 = min((x+1)>>1, wc-1).  In float32, one IEEE
 * operation per written operation:
 *   BILINEAR  the four corners (y0|y1, x0|x1) are all good, U = ((U00 + U01) + (U10 + U11)) * 0.5f, V likewise, and both are
 *             finite: [U, V, 1].  Twice the mean of the corners: a + b or 2a where corners coincide;
 *   NEAREST   otherwise, corner (y0,x0) is good and 2*U00, 2*V00 are finite: [2*U00, 2*V00, 1];
 *   INVALID   otherwise: [0, 0, 0].
 * d_counts (NULL to skip) receives int32 {bilinear, nearest, invalid}, which add up to h*w; the call zeroes them itself, on the
 * stream (integer atomics: exact in any order).
 * DFLOW_EINVAL: a size or layout outside its range, a NULL d_coarse or d_out, a pointer that is not 4-byte aligned, d_out ==
 * d_coarse, d_counts equal to either. */
int dflow_pyr_down(int32_t h, int32_t w, const uint8_t *d_in1, const uint8_t *d_in2 /* NULL: one image */,
                   uint8_t *d_out1, uint8_t *d_out2 /* NULL with d_in2 */, void *stream);
int dflow_flow_upsample(int32_t h, int32_t w, const float *d_coarse, int32_t layout,
                        float *d_out /* (h,w,3) [U,V,valid] */, int32_t *d_counts /* NULL or int32[3] */, void *stream);

/* The forward/backward check in image coordinates (DESIGN.md "Forward/backward check in image coordinates"): the vector at p
 * against the other direction's vector at p + f(p).  This build's definition: dflow_fb_consistency, above, restates the
 * reference's check, which adds U to the row and V to the column, and stays what it is; the reference has no
 * counterpart to this one.  1 <= h, w <= 8192.  d_fwd and d_bwd are (h,w,.) float32, each in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX
 * layout.  A vector is GOOD as in dflow_flow_upsample: valid under its layout (valid > 0.5 under UVV, always under DYDX) and
 * both components finite.  Float32, one IEEE operation per written operation.  For pixel (y,x) of the forward output, with
 * (V,U) = (dy,dx) of d_fwd there, the class is the first that applies:
 *   FWD_INVALID  the forward vector is not good;
 *   OUTSIDE      nearest (no flag): (ry,rx) = rintf of (V,U), ties to even; a rounded component outside [-32767, 32767], or a
 *                target (ty,tx) = (y+ry, x+rx) outside the frame.  DFLOW_FBC_BILINEAR: py = (float)y + V, px = (float)x + U, and
 *                not (py >= 0 && py <= (float)(h-1) && px >= 0 && px <= (float)(w-1));
 *   BWD_INVALID  nearest: the vector of d_bwd at (ty,tx) is not good; else (bv,bu) is that vector.  Bilinear: y0 = (int)floorf(py),
 *                ay = py - (float)y0, y1 = ay > 0 ? y0+1 : y0, and x0, ax, x1 likewise (a corner of weight zero is not looked
 *                at); one of the corners (y0|y1, x0|x1) is not good; else t = U00 + ax*(U01 - U00), b = U10 + ax*(U11 - U10),
 *                bu = t + ay*(b - t), and bv likewise;
 *   ABOVE        du = U + bu, dv = V + bv, err = sqrtf(du*du + dv*dv), and not err <= thresh (a NaN or infinite err is above);
 *   CONSISTENT   otherwise.
 * d_out_fwd (h,w,3) float32 receives [U, V, 1], the forward vector's own bits, for CONSISTENT and [0,0,0] for every other class;
 * d_err_fwd (NULL to skip) (h,w) float32 receives err for ABOVE and CONSISTENT and -1 otherwise; d_counts (NULL to skip) receives
 * int32 {consistent, above, bwd_invalid, outside, fwd_invalid}, which add up to h*w; the call zeroes them itself, on the stream
 * (integer atomics: exact in any order).  With d_out_bwd the same is done with the roles of d_fwd and d_bwd swapped, in the same
 * launch, into d_out_bwd, d_err_bwd and d_counts[5..9]; outputs and counts equal those of two single calls.  On integer-valued
 * fields (every BCD output) bilinear equals nearest bit for bit.
 * DFLOW_EINVAL before anything is launched: a size, layout or flag outside its range, thresh not finite or negative, a NULL
 * d_fwd, d_bwd or d_out_fwd, d_err_bwd without d_out_bwd, a pointer that is not 4-byte aligned, an output equal to an input or to
 * another output.  Asynchronous on `stream`, allocates nothing, needs no workspace, reads nothing back, can be captured into a
 * graph. */
#define DFLOW_FBC_BILINEAR 1u
int dflow_flow_consistency(int32_t h, int32_t w,
        const float *d_fwd, int32_t layout_fwd, const float *d_bwd, int32_t layout_bwd,
        float thresh, uint32_t flags,
        float *d_out_fwd /* (h,w,3) [U,V,valid] */, float *d_out_bwd /* NULL: forward only */,
        float *d_err_fwd /* NULL or (h,w) */, float *d_err_bwd /* NULL or (h,w); needs d_out_bwd */,
        int32_t *d_counts /* NULL, or int32[5], int32[10] with d_out_bwd */, void *stream);

/* The small-segment filter of a sparse flow field (DESIGN.md "Small-segment filter"): the second post-processing step of Menze,
 * Heipke and Geiger, on the device.  This build's definition: dflow_remove_small_segments_host, above, restates the reference's
 * removeSmallSegments, a sequential flood fill whose result depends on its scan order, and stays what it is; the two agree only
 * on a field where nothing is removed and no non-member touches a member it could absorb (DESIGN.md names the differences).
 * 1 <= h, w <= 8192.  d_flow is (h,w,.) float32 in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout.
 *   MEMBER   a pixel whose vector is GOOD as in dflow_flow_consistency: valid under its layout (valid > 0.5 under UVV, always
 *            under DYDX) and both components finite.
 *   JOINED   two 4-adjacent members p and q with fabsf(Up - Uq) + fabsf(Vp - Vq) <= thresh, in float32, one IEEE operation per
 *            written operation.  The test is symmetric in p and q; a difference that overflows does not join.
 *   SEGMENT  a connected component of the members under "joined".  Its id is the smallest raster index y*w + x among its
 *            pixels, its size its pixel count.
 *   REMOVED  a segment with size < min_size; with DFLOW_SEG_KEEP_SINGLETONS segments of size 1 are kept whatever min_size is
 *            (the reference's `1 < count`).  min_size 0 or 1 removes nothing.
 * d_out (h,w,3) float32 receives [U, V, 1], the pixel's own U and V bits, at a member of a segment that is kept and [0,0,0] at
 * every other pixel.  d_segment (NULL to skip) (h,w) int32 receives the id, -1 at a pixel that is no member; d_size (NULL to skip)
 * (h,w) int32 the size of the pixel's segment, 0 at a pixel that is no member: both describe the segments of the input, so a
 * removed segment keeps its id and size there.  d_counts (NULL to skip) receives int32 {segments, segments removed, members,
 * pixels removed}; the call zeroes them itself, on the stream.  Everything is an integer or a copy of input bits: the result
 * depends on no order, two calls give the same bytes, and a second call on the first one's output changes nothing (removing
 * segments joins no others).  Under DFLOW_EVAL_UVV d_out may be d_flow itself; any other overlap of d_flow, d_out, d_segment,
 * d_size, d_counts and the workspace, and d_out == d_flow under DFLOW_EVAL_DYDX, is refused.
 * DFLOW_EINVAL before anything is launched: a size, layout or flag bit outside its range, thresh not finite or below 0, min_size
 * below 0, a NULL d_flow or d_out, a pointer that is not 4-byte aligned, a forbidden overlap.  DFLOW_ENOSPC: a NULL or too small
 * workspace (a label and a size per pixel, 8 bytes per pixel plus alignment).  Four launches whatever the field holds; no
 * workgroup waits for another.  Asynchronous on `stream`, allocates nothing, reads nothing back, can be captured into a graph;
 * dflow_segment_filter_workspace_bytes returns 0 (and sets dflow_last_error) for sizes outside the range. */
#define DFLOW_SEG_KEEP_SINGLETONS 1u
size_t dflow_segment_filter_workspace_bytes(int32_t h, int32_t w);
int dflow_segment_filter(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        float thresh, int32_t min_size, uint32_t flags,
        float *d_out      /* (h,w,3) [U,V,valid] */,
        int32_t *d_segment /* NULL or (h,w) */, int32_t *d_size /* NULL or (h,w) */,
        int32_t *d_counts  /* NULL or int32[4] */,
        void *d_ws, size_t ws_bytes, void *stream);

/* Motion-compensated frame interpolation (DESIGN.md "Frame interpolation"): the frame at time t, 0 < t < 1, between frame 1
 * (time 0) and frame 2 (time 1), from the forward flow alone or from both flows.  This build's definition; the reference has no
 * counterpart.  1 <= h, w <= 8192.  d_bgr1, d_bgr2 (h,w,3) uint8 BGR; d_fwd (frame 1 -> 2) and d_bwd (frame 2 -> 1, NULL: forward
 * only) are (h,w,.) float32, each in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout (layout_bwd is not looked at without d_bwd).  A
 * vector is GOOD as in dflow_flow_consistency, a position INSIDE, a picture sampled bilinearly and two colours compared as in
 * dflow_warp_eval (the same formulas in the same order).  Float32, one IEEE operation per written operation; s = 1.0f - t, formed
 * once.  n = h*w.
 *   A. CLAIMANTS.  Source i = y*w + x of frame 1, with (U,V) of d_fwd there, TAKES PART if (U,V) is good, its end point
 *      (x + U, y + V) is inside, and its place at time t, (tx,ty) = (rintf(x + t*U), rintf(y + t*V)) (ties to even), lies in the
 *      frame.  Its error e is dflow_warp_eval's err of that pixel: frame 2 sampled at the end point against I1[i].  Its key is
 *      (uint64)bits(e) << 32 | i (e is a sum of absolute values: non-negative, its bits order like its value) and it carries the
 *      motion m = (U,V).  With d_bwd, source j of frame 2 with (Ub,Vb) of d_bwd takes part likewise: end point (x + Ub, y + Vb)
 *      inside, place (rintf(x + s*Ub), rintf(y + s*Vb)), e the same expression with the frames' roles swapped (frame 1 sampled
 *      against I2[j]), key bits(e) << 32 | (n + j), motion m = (-Ub, -Vb), each float negated.  Every target takes the claimant
 *      with the smallest key: the smaller error, at equal error frame 1 before frame 2 and the smaller raster index.  d_keys
 *      (h,w) uint64 is set to all ones by the call, written with 64-bit atomicMin and left holding the winning key, all ones
 *      where nobody claimed; a second launch resolves the winners into the motion field, [mU, mV, 1] or [0,0,0].  The result does
 *      not depend on the order of arrival.  Provenance src: 1 (frame 1), 2 (frame 2), 0 (none).
 *   B. FILL.  fill_rounds Jacobi rounds, 0 <= fill_rounds <= 64: a pixel unknown before the round takes the motion of the first
 *      of its neighbours known before the round, in the order up (y-1), left, right, down, and becomes [mU, mV, 1] with src = 3.
 *      Every round is launched whatever the field holds.  The rounds alternate between d_motion and d_motion_tmp, both (h,w,3)
 *      float32, and the last writes d_motion: after the call d_motion holds the final field for any fill_rounds and d_motion_tmp
 *      (NULL allowed with fill_rounds = 0, and then untouched) the field before the last round.
 *   C. RENDER, pixel q = (x,y).  FALLBACK, per channel: v = s*I1[q] + t*I2[q].  An unknown pixel takes the fallback.  A known
 *      pixel with motion (U,V): side 1 is frame 1 at (x - t*U, y - t*V), side 2 frame 2 at (x + s*U, y + s*V); a side is usable
 *      when its position is inside, and c1 / c2 is its bilinear sample.  Both usable, d = ((|c1_b-c2_b| + |c1_g-c2_g|) +
 *      |c1_r-c2_r|) / 3: d <= occl_thresh gives v = s*c1 + t*c2 (BLENDED); otherwise (ONE-SIDED) c1 if src = 1, c2 if src = 2, and
 *      for src = 3 c1 when t <= 0.5f, else c2.  One side usable: that side (ONE-SIDED).  No side usable: the fallback.
 *      d_out (h,w,3) uint8 = (int)floorf(v + 0.5f).
 * Optional outputs (NULL to skip): d_source (h,w) uint8, src after the fill (0, 1, 2 or 3); d_counts int32[8] {from frame 1, from
 * frame 2, filled, unknown after the fill | blended, one-sided, fallback | claimants that lost}: the first four add up to h*w, so
 * do the next three, and from frame 1 + from frame 2 + lost is the number of sources that took part; the call zeroes them itself,
 * on the stream (integer atomics: exact in any order).  Every output is an integer or a float32 chain in a fixed order: two calls
 * give the same bytes.
 * There is no d_ws: the scratch is the caller's typed planes d_keys, d_motion and d_motion_tmp, which are outputs as well.
 * DFLOW_EINVAL before anything is launched: a size or layout outside its range, t not finite or not in (0, 1), fill_rounds
 * outside [0, 64], occl_thresh not finite or below 0, any flag bit (there are none yet), a NULL d_bgr1, d_bgr2, d_fwd, d_out,
 * d_keys or d_motion, a NULL d_motion_tmp with fill_rounds > 0, d_keys not 8-byte aligned, a float or int32 plane not 4-byte
 * aligned, an output equal to an input or to another output.  3 + fill_rounds launches and two memsets.  Asynchronous on
 * `stream`, allocates nothing, reads nothing back, can be captured into a graph. */
int dflow_frame_interp(int32_t h, int32_t w, const uint8_t *d_bgr1, const uint8_t *d_bgr2,
        const float *d_fwd, int32_t layout_fwd, const float *d_bwd /* NULL: forward only */, int32_t layout_bwd,
        float t, int32_t fill_rounds, float occl_thresh, uint32_t flags,
        uint8_t *d_out /* (h,w,3) */, uint64_t *d_keys /* (h,w) */, float *d_motion /* (h,w,3) */,
        float *d_motion_tmp /* (h,w,3); NULL allowed when fill_rounds == 0 */,
        uint8_t *d_source /* NULL or (h,w) */, int32_t *d_counts /* NULL or int32[8] */, void *stream);

/* Edge-aware weighted median filter of a flow field (DESIGN.md "Weighted median filter"): every pixel gets the weighted median,
 * per component, of the good vectors in the (2 radius + 1)^2 window around it, weighted by distance and by the similarity of a
 * guide image (the non-local term of Sun, Roth and Black; with the guide the joint-bilateral median).  This build's definition;
 * the reference has no counterpart.  1 <= h, w <= 8192, 1 <= radius <= 8.  d_flow is (h,w,.) float32 in DFLOW_EVAL_UVV or
 * DFLOW_EVAL_DYDX layout; a vector is GOOD as in dflow_flow_consistency.  Everything below is an integer or a copy of input bits:
 * the result depends on no order, and two calls give the same bytes.
 *   SAMPLES of pixel p = (y,x): the good pixels q = (y+dy, x+dx), |dy|, |dx| <= radius, inside the frame (the window is clipped,
 *     not padded); p itself is a sample when it is good.
 *   WEIGHT  (uint32) wq = S * C.  S = d_wspace[|dy|*(radius+1) + |dx|], or 1 without d_wspace.  C = d_wcolor[|b_p - b_q| +
 *     |g_p - g_q| + |r_p - r_q|] with the channels of d_bgr (h,w,3) uint8, or 1 without d_wcolor.  W = the sum of the wq, at most
 *     289 * 255 * 255, so 2 W fits 32 bits.  A sample of weight 0 does not take part.
 *   KEY     of a float with bits b: b ^ 0xFFFFFFFF if the sign bit is set, else b | 0x80000000: a total order in which -0 < +0.
 *   MEDIAN  the lower weighted median, U and V each on its own: the value mU (mV) of the sample with the smallest key k such that
 *     2 * sum{wq : key_q <= k} >= W.  The output carries that sample's own bits.
 *   OUTPUT  d_out (h,w,3) float32 [U,V,valid].  W == 0: [0,0,0].  Otherwise, with no flag, [mU, mV, 1] whether p is good or not
 *     (holes are filled).  DFLOW_WMED_KEEP_HOLES: a p that is not good gets [0,0,0].  DFLOW_WMED_REJECT: a p that is not good gets
 *     [0,0,0]; a good p keeps its own [U,V,1] bits if fabsf(U - mU) + fabsf(V - mV) <= reject_thresh and becomes [0,0,0]
 *     otherwise (float32, one IEEE operation per written operation; a difference that overflows rejects): surviving vectors are
 *     never altered.  reject_thresh is looked at only under DFLOW_WMED_REJECT.
 * d_counts (NULL to skip) int32[4] {good inputs, valid outputs, filled, altered}: filled counts the p that are not good and have a
 * valid output, altered the good p whose output U or V bits differ from their own or whose output is [0,0,0]; the call zeroes them
 * itself, on the stream (integer atomics: exact in any order).
 * There is no workspace: the kernel needs no global scratch.
 * DFLOW_EINVAL before anything is launched: a size, layout or radius outside its range, an unknown flag bit, reject_thresh not
 * finite or below 0 under DFLOW_WMED_REJECT, a NULL d_flow or d_out, d_bgr and d_wcolor not both NULL or both given, a float or
 * int32 plane not 4-byte aligned, an output equal to an input (neighbours are read) or to the other output.  One launch and the
 * memset of the counts.  Asynchronous on `stream`, allocates nothing, reads nothing back, can be captured into a graph. */
#define DFLOW_WMED_KEEP_HOLES 1u
#define DFLOW_WMED_REJECT 2u
int dflow_flow_wmedian(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        const uint8_t *d_bgr    /* guide (h,w,3); NULL iff d_wcolor is NULL */,
        int32_t radius,
        const uint8_t *d_wspace /* NULL (all ones) or uint8[(radius+1)*(radius+1)], [|dy|*(radius+1)+|dx|] */,
        const uint8_t *d_wcolor /* NULL (all ones) or uint8[766], indexed by |db|+|dg|+|dr| */,
        float reject_thresh, uint32_t flags,
        float *d_out /* (h,w,3) [U,V,valid] */, int32_t *d_counts /* NULL or int32[4] */, void *stream);

/* Robust global-motion fit of a flow field (DESIGN.md "Global-motion fit"): the affine map or the homography that most vectors of
 * a flow field agree with, found by random minimal samples (RANSAC with local rounds and a least-squares polish), with the
 * inlier / outlier classes, the model's own dense flow and the residual flow.  This build's definition; the reference has no
 * counterpart.  1 <= h, w <= 8192, n = h*w.  d_flow is (h,w,.) float32 in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout; a vector is
 * GOOD as in dflow_flow_consistency.  d_exclude (NULL: nothing) is (h,w) uint8, non-zero = the pixel takes no part.  Pixel i = y*w
 * + x TAKES PART if its vector (U,V) is good and it is not excluded; it is SCORED if it takes part and y % step == 0 && x % step
 * == 0.  xf = (float)x, yf = (float)y, and its target is tx = xf + U, ty = yf + V (float32).  A model is float32[9], row-major M:
 * (x,y,1) -> (X,Y,W), the position in frame 2 being (X/W, Y/W).  Float32 and float64 chains are one IEEE operation per written
 * operation; everything else is an integer.  The result depends on no order of arrival, and two calls give the same bytes.
 *   INLIER of model m (float32): X = (m0*xf + m1*yf) + m2, Y = (m3*xf + m4*yf) + m5, W = (m6*xf + m7*yf) + m8, ex = X - W*tx,
 *     ey = Y - W*ty; inlier iff W > 0 && ex*ex + ey*ey <= (thresh*W)*(thresh*W).  A NaN anywhere makes it false.
 *   A. HYPOTHESES.  The current model starts as the identity.  Rounds r = 0 .. lo_rounds, hypotheses j = 0 .. n_hyp-1, each of
 *     m = 3 (DFLOW_MOTION_AFFINE) or 4 (DFLOW_MOTION_HOMOGRAPHY) points.  Point k = 0 .. m-1 tries attempts a = 0 .. 15: Philox4x32-10
 *     with counter (j, (r*4 + k)*16 + a, 0, 0) and key (seed & 0xFFFFFFFF, seed >> 32), word 0 = u, i = ((uint64)u * n) >> 32.  The
 *     first i is accepted that takes part, differs from the points accepted before it and, in rounds r > 0, is an inlier of the
 *     current model (the best of the rounds before; the identity if there is none).  A point without one in 16 attempts makes the
 *     hypothesis DEGENERATE.  Solve, in float64: P = the smallest power of two >= max(h,w), s = 1/P, cx = (w-1)/2, cy = (h-1)/2,
 *     a_k = (xf - cx)*s, b_k = (yf - cy)*s, p_k = (tx - cx)*s, q_k = (ty - cy)*s.  Affine: rows [a_k, b_k, 1 | p_k, q_k], k = 0..2,
 *     one elimination with two right-hand sides -> N = [[n0,n1,n2],[n3,n4,n5],[0,0,1]].  Homography: rows 2k = [a,b,1,0,0,0,
 *     -(a*p), -(b*p) | p] and 2k+1 = [0,0,0,a,b,1, -(a*q), -(b*q) | q], k = 0..3 -> N = [[n0,n1,n2],[n3,n4,n5],[n6,n7,1]].
 *     ELIMINATION of an N x N system: for column c = 0.., the pivot is the row r >= c with the largest |A[r][c]|, the first such
 *     row winning; a pivot that is not >= 2^-40 makes the hypothesis degenerate; rows c and pivot are swapped; for every row r > c:
 *     f = A[r][c] / A[c][c], A[r][k] = A[r][k] - f*A[c][k] for k > c.  Back substitution from the last row: t = rhs[r]; for k =
 *     r+1.. ascending t = t - A[r][k]*x[k]; x[r] = t / A[r][r].  To pixel coordinates, row i of N: r0 = n_i0*s, r1 = n_i1*s, r2 =
 *     (n_i2 - r0*cx) - r1*cy -> R; M_0c = P*R_0c + cx*R_2c, M_1c = P*R_1c + cy*R_2c, M_2c = R_2c; each entry is then cast to
 *     float32 (for affine the last row is exactly (0,0,1)).  Also degenerate: a float32 entry that is not finite; for a homography,
 *     W <= 0 (in the float32 expression above) at one of its own sample points.  A degenerate hypothesis stores the identity and
 *     its count is 0.
 *   B. SCORE.  d_hyp_counts[j] = the number of scored pixels that are inliers of hypothesis j (int32, integer adds).
 *   C. BEST.  Every hypothesis that is not degenerate offers the key (uint64)count << 32 | (0xFFFFFFFF - (r*65536 + j)) to a
 *     64-bit maximum in d_state[0], which starts at 0 and is kept across the rounds: the larger count wins, at equal counts the
 *     earlier round, then the smaller j.  After a round whose hypothesis holds the maximum, that hypothesis is the current model.
 *     d_state[0] == 0 (every hypothesis of every round degenerate): the model is the identity, the best round and index are -1, and
 *     there is no polish.
 *   E. POLISH, affine only (`polish` is ignored for a homography: its sums would overflow int64), `polish` times: over the
 *     scored inliers of the current model with fabsf(tx) <= 32768 && fabsf(ty) <= 32768 (the others are counted as skipped, once
 *     per step), the int64 sums N, Sa, Sb, Saa, Sab, Sbb, Sp, Sap, Sbp, Sq, Saq, Sbq of a = 2x - (w-1), b = 2y - (h-1), p =
 *     llrintf(tx*64), q = llrintf(ty*64) (|a|, |b| < 2^13, |p|, |q| <= 2^21, at most 2^26 pixels: every sum stays below 2^60).
 *     Each sum is converted to float64 (one rounding), then c00 = Sbb*N - Sb*Sb, c01 = Sb*Sa - Sab*N, c02 = Sab*Sb - Sbb*Sa, c11 =
 *     Saa*N - Sa*Sa, c12 = Sa*Sab - Saa*Sb, c22 = Saa*Sbb - Sab*Sab, det = (Saa*c00 + Sab*c01) + Sa*c02; for (r0,r1,r2) = (Sap,
 *     Sbp, Sp): x0 = ((c00*r0 + c01*r1) + c02*r2)/det, x1 = ((c01*r0 + c11*r1) + c12*r2)/det, x2 = ((c02*r0 + c12*r1) +
 *     c22*r2)/det, m0 = (float)(x0*0.03125), m1 = (float)(x1*0.03125), m2 = (float)(((x2 - x0*(w-1)) - x1*(h-1))*0.015625); m3..m5
 *     likewise from (Saq, Sbq, Sq); last row (0,0,1).  N < 3, det zero or not finite, or an entry not finite: the current model
 *     stays.  Otherwise the candidate's scored inliers are counted and it becomes the current model iff its count >= the current
 *     model's.
 *   F. APPLY, every pixel whatever `step` is, each output optional (NULL to skip).  d_class (h,w) uint8: 0 not good, 1 inlier of
 *     the final model, 2 outlier, 3 good but excluded.  d_model_flow (h,w,3) float32: [X/W - xf, Y/W - yf, 1] if W > 0, else
 *     [0,0,0], at every pixel, good or not.  d_residual (h,w,3) float32: [U - Um, V - Vm, 1] at a good pixel with W > 0, else
 *     [0,0,0].  d_counts int32[8], zeroed by the call on the stream: {scored pixels, scored inliers of the final model, degenerate
 *     hypotheses of all rounds, best round (-1: none), best j (-1: none), the best hypothesis' count, polish steps accepted, pixels
 *     skipped by the polish range, summed over the steps}.
 * d_model receives the final model; d_models (n_hyp*9) and d_hyp_counts (n_hyp) hold the hypotheses of the last round and their
 * counts.  There is no d_ws: the scratch is the caller's typed planes d_models, d_hyp_counts and d_state (int64[32]: [0] the best
 * key, the rest counters, the polish sums and the candidate), which are outputs as well.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout; model outside
 * [0,1]; thresh not finite or not > 0; n_hyp outside [1,65536]; lo_rounds outside [0,4]; polish outside [0,4]; step outside
 * [1,64]; any flag bit (there are none yet); a NULL d_flow, d_model, d_models, d_hyp_counts or d_state; d_state not 8-byte
 * aligned, a float or int32 plane not 4-byte aligned; an output or scratch plane equal to an input or to one listed before it.
 * 3 + 4 (lo_rounds + 1) + 4 polish launches (polish counted as 0 for a homography) and one or two memsets, whatever the field
 * holds.  Asynchronous on `stream`, allocates nothing, reads nothing back, can be captured into a graph. */
#define DFLOW_MOTION_AFFINE 0      /* 3-point minimal sample */
#define DFLOW_MOTION_HOMOGRAPHY 1  /* 4-point minimal sample */
int dflow_motion_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        const uint8_t *d_exclude /* NULL or (h,w): non-zero = take no part */,
        int32_t model, float thresh, int32_t n_hyp /* 1..65536 */, int32_t lo_rounds /* 0..4 */,
        int32_t polish /* 0..4 */, int32_t step /* 1..64 */, uint64_t seed, uint32_t flags /* none yet */,
        float *d_model       /* float32[9] */,
        float *d_models      /* scratch+output float32[n_hyp*9]: the last round's hypotheses */,
        int32_t *d_hyp_counts /* scratch+output int32[n_hyp]: their inlier counts, 0 for a degenerate one */,
        int64_t *d_state     /* scratch+output int64[32], 8-byte aligned */,
        uint8_t *d_class     /* NULL or (h,w) */, float *d_model_flow /* NULL or (h,w,3) */,
        float *d_residual    /* NULL or (h,w,3) */, int32_t *d_counts /* NULL or int32[8] */, void *stream);

/* Epipolar-geometry fit of a flow field (DESIGN.md "Epipolar-geometry fit"): the fundamental matrix that most vectors of a flow
 * field agree with, x'^T F x = 0 for a pixel x and its target x', found by random 7-point samples (RANSAC with local rounds), with
 * the inlier / outlier classes and the per-pixel Sampson distance.  It is the model of a camera moving through a rigid scene with
 * depth, where dflow_motion_fit's homography fits one plane only.  This build's definition; the reference has no counterpart.
 * 1 <= h, w <= 8192, n = h*w.  d_flow, GOOD, d_exclude, TAKES PART, SCORED, xf, yf, tx, ty, thresh (pixels), step and seed are
 * dflow_motion_fit's, unchanged.  Float32 and float64 chains are one IEEE operation per written operation; everything else is an
 * integer.  The result depends on no order of arrival, and two calls give the same bytes.
 *   COORDINATES.  P = the smallest power of two >= max(h,w), s = 1/P, cx = (w-1)/2, cy = (h-1)/2 (all exact in float32).  In
 *     float32: a = (xf - cx)*s, b = (yf - cy)*s (exact), p = (tx - cx)*s, q = (ty - cy)*s.  A model is F^ in these coordinates,
 *     float32[9], row-major, with (p,q,1) F^ (a,b,1)^T = 0: scoring in pixel coordinates would cancel in float32.  The fundamental
 *     matrix in pixels is T^T F^ T, T = [[s,0,-cx*s],[0,s,-cy*s],[0,0,1]] (the host's business: pipeline.epipolar_geometry).
 *   INLIER of model F (float32): l0 = (F0*a + F1*b) + F2, l1 = (F3*a + F4*b) + F5, l2 = (F6*a + F7*b) + F8, e = (p*l0 + q*l1) + l2,
 *     m0 = (F0*p + F3*q) + F6, m1 = (F1*p + F4*q) + F7, den = ((l0*l0 + l1*l1) + m0*m0) + m1*m1, t = thresh*s; inlier iff
 *     0 < den < +Inf && e*e <= (t*t)*den: the Sampson distance is at most thresh pixels, with no division.  A NaN anywhere makes
 *     it false, and so does a den that overflowed (a vector of 1e30 pixels agrees with nothing).
 *   A. SAMPLES.  There is no current model at the start (d_model all zeros: nothing is its inlier).  Rounds r = 0 .. lo_rounds,
 *     samples j = 0 .. n_hyp-1, each of 7 points.  Point k = 0 .. 6 tries attempts t = 0 .. 15: Philox4x32-10 with counter
 *     (j, (r*8 + k)*16 + t, 0, 0) and key (seed & 0xFFFFFFFF, seed >> 32), word 0 = u, i = ((uint64)u * n) >> 32.  The first i is
 *     accepted that takes part, differs from the points accepted before it and, in rounds r > 0, is an inlier of the current model
 *     (the best of the rounds before).  A point without one in 16 attempts makes the three slots of the sample DEGENERATE.
 *     In float64, with a_k = ((double)xf - cx)*s, b_k, p_k = ((double)tx - cx)*s, q_k likewise: row k of the 7 x 9 system A is
 *     [p*a, p*b, p, q*a, q*b, q, a, b, 1].
 *     ELIMINATION with complete pivoting: for c = 0..6 the pivot is the largest |A[r][k]| over r >= c, k >= c, the first in
 *     row-major order winning; a pivot that is not >= 2^-40 makes the sample degenerate; rows c and r are swapped, then columns c
 *     and k (in all seven rows; the permutation is remembered); for every row r > c: f = A[r][c] / A[c][c], A[r][k] = A[r][k] -
 *     f*A[c][k] for k > c.  The columns left at positions 7 and 8 are the free variables.  Solution 1 has (x7,x8) = (1,0) and t =
 *     -A[r][7], solution 2 has (0,1) and t = -A[r][8]; back substitution from row 6: for k = r+1 .. 6 ascending t = t - A[r][k]*x[k];
 *     x[r] = t / A[r][r].  With the column permutation undone they are F1 and F2.  (A fixed choice of free columns would be
 *     systematically degenerate for a pure forward or a pure sideways translation, whose F has exact zeros.)
 *     CUBIC.  det M = (M0*(M4*M8 - M5*M7) - M1*(M3*M8 - M5*M6)) + M2*(M3*M7 - M4*M6), one expression.  k3 = det F1, k0 = det F2,
 *     dp = det(F1 + F2), dm = det(F2 - F1) (entrywise sums), k2 = (dp + dm)*0.5 - k0, k1 = (dp - dm)*0.5 - k3: det(x F1 + F2) =
 *     ((k3*x + k2)*x + k1)*x + k0.  A coefficient that is not finite: no model.
 *     ROOTS over the whole projective line, each once: the roots x of (k3,k2,k1,k0) in [-1,1] give F = x*F1 + F2; then the roots
 *     x of the reversed cubic (k0,k1,k2,k3) in the open (-1,1) give F = F1 + x*F2 (entrywise, two operations).  Roots of
 *     (c3,c2,c1,c0) with g(x) = ((c3*x + c2)*x + c1)*x + c0: qa = 3*c3, qb = 2*c2, disc = qb*qb - (4*qa)*c1; if disc > 0: sq =
 *     sqrt(disc), qq = -0.5*(qb + (qb < 0 ? -sq : sq)), x1 = qq/qa, x2 = c1/qq, and those of min, max (x1 < x2 ? ...) that lie
 *     strictly inside (-1,1) split [-1,1], in that order, into monotone pieces.  g(-1) == 0 is a root of the closed interval.  For
 *     each piece [u,v] in ascending order: g(v) == 0 makes v a root (not v = 1 of the open interval); otherwise, if g(u) and g(v)
 *     are non-zero with opposite signs, 60 times: mid = 0.5*(lo + hi); (g(mid) < 0) == (g(u) < 0) ? lo = mid : hi = mid; the root
 *     is 0.5*(lo + hi).  No cbrt, acos or pow.  The first three roots, in this order, are the models of the slots 3j, 3j+1, 3j+2.
 *     CANONICAL SCALE.  Each entry is divided by the entry of largest magnitude (the first such entry; it becomes +1), then cast
 *     to float32.  A slot without a root, or with an entry that is not finite, is DEGENERATE: it stores zeros and its count is 0.
 *   B. SCORE.  d_hyp_counts[slot] = the number of scored pixels that are inliers of the slot's model (int32, integer adds).
 *   C. BEST.  Every slot that is not degenerate offers the key (uint64)count << 32 | (0xFFFFFFFF - (r*65536 + slot)) to a 64-bit
 *     maximum in d_state[0], which starts at 0 and is kept across the rounds: the larger count wins, at equal counts the earlier
 *     round, then the smaller slot.  After a round whose slot holds the maximum, that model is the current model.  There is no
 *     polish: a least-squares F needs an eigen-solve, and its float sums would depend on the order of arrival.
 *     NO MODEL.  d_state[0] == 0 (every slot of every round degenerate): d_model is all zeros, the best round and slot are -1, and
 *     every good pixel is class 2.  This is the answer for a still camera (zero flow: the system has rank 6), for a line of
 *     pixels, and for fewer than 7 pixels that take part.
 *   D. APPLY, every pixel whatever `step` is, each output optional (NULL to skip).  d_class (h,w) uint8: 0 not good, 1 inlier of
 *     the final model, 2 outlier, 3 good but excluded.  d_residual (h,w) float32: the Sampson distance in pixels, sqrtf((e*e)/den)*P,
 *     at a good pixel with 0 < den < +Inf; +Inf at any other good pixel; -1 at a pixel that is not good.  d_counts int32[8], zeroed
 *     by the call on the stream: {scored pixels, scored inliers of the final model, degenerate slots of all rounds, best round
 *     (-1: none), best slot (-1: none), the best slot's count, (1000 * models of round 0) / n_hyp, 0}.
 * d_model receives the final F^; d_models (3*n_hyp*9) and d_hyp_counts (3*n_hyp) hold the slots of the last round and their counts.
 * There is no d_ws: the scratch is the caller's typed planes d_models, d_hyp_counts and d_state (int64[32]: [0] the best key, the
 * rest counters), which are outputs as well.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout; thresh not
 * finite or not > 0; n_hyp outside [1,21845] (3*n_hyp slots fit the key's 16-bit index); lo_rounds outside [0,4]; step outside
 * [1,64]; any flag bit (there are none yet); a NULL d_flow, d_model, d_models, d_hyp_counts or d_state; d_state not 8-byte
 * aligned, a float or int32 plane not 4-byte aligned; an output or scratch plane equal to an input or to one listed before it.
 * 3 + 4 (lo_rounds + 1) launches and one or two memsets, whatever the field holds.  Asynchronous on `stream`, allocates nothing,
 * reads nothing back, can be captured into a graph. */
#define DFLOW_EPIPOLAR_MAX_HYP 21845
int dflow_epipolar_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        const uint8_t *d_exclude /* NULL or (h,w): non-zero = take no part */,
        float thresh, int32_t n_hyp /* 1..21845 */, int32_t lo_rounds /* 0..4 */, int32_t step /* 1..64 */,
        uint64_t seed, uint32_t flags /* none yet */,
        float *d_model       /* float32[9]: F^, all zeros when there is no model */,
        float *d_models      /* scratch+output float32[3*n_hyp*9]: the last round's slots */,
        int32_t *d_hyp_counts /* scratch+output int32[3*n_hyp]: their inlier counts, 0 for a degenerate one */,
        int64_t *d_state     /* scratch+output int64[32], 8-byte aligned */,
        uint8_t *d_class     /* NULL or (h,w) */, float *d_residual /* NULL or (h,w) */,
        int32_t *d_counts    /* NULL or int32[8] */, void *stream);

/* Two-view reconstruction (DESIGN.md "Two-view reconstruction"): from the F^ that dflow_epipolar_fit leaves on the device and the
 * camera's intrinsics, the rotation and the unit translation of the second camera, X2 = R X1 + t, a depth per pixel in units of
 * the baseline |t| = 1, a reprojection error, and a class plane in which "behind a camera" marks what moves against the epipolar
 * direction, the fit's blind spot.  This build's definition; the reference has no counterpart.  1 <= h, w <= 8192, n = h*w.
 * d_flow, GOOD, xf, yf, the float32 targets tx, ty, P, s and step are dflow_epipolar_fit's, unchanged; its centre is called
 * (cxF, cyF) = ((w-1)/2, (h-1)/2) here.  fx, fy (pixels, finite and > 0) and cx, cy (finite) are the pinhole camera of both
 * frames.  d_model is float32[9], F^ in the fit's coordinates, read on the device.  d_part (NULL: every pixel) is (h,w) uint8: a
 * pixel VOTES iff it is GOOD, y % step == 0 && x % step == 0 and, with d_part, its byte == 1 (the fit's inlier class).  All
 * arithmetic is float64, one IEEE operation (+ - * / sqrt) per written operation; everything else is an integer.  The result
 * depends on no order of arrival, and two calls give the same bytes.
 *   A. ESSENTIAL MATRIX.  With F the float32 entries widened, a00 = s*fx, a02 = s*(cx - cxF), a11 = s*fy, a12 = s*(cy - cyF) (A =
 *     [[a00,0,a02],[0,a11,a12],[0,0,1]] takes camera coordinates to the fit's): G = F A, G[i][0] = F[i][0]*a00, G[i][1] =
 *     F[i][1]*a11, G[i][2] = (F[i][0]*a02 + F[i][1]*a12) + F[i][2]; E = A^T G, E[0][j] = a00*G[0][j], E[1][j] = a11*G[1][j],
 *     E[2][j] = (a02*G[0][j] + a12*G[1][j]) + G[2][j].  x2^T E x1 = 0 for the camera coordinates below.
 *   B. DECOMPOSITION.  M = E^T E, M[i][j] = M[j][i] = (E[0][i]*E[0][j] + E[1][i]*E[1][j]) + E[2][i]*E[2][j] for i <= j; V = I.
 *     8 cyclic Jacobi sweeps (a fixed number and no tolerance: Jacobi converges quadratically, and nothing is tested), each over the
 *     pairs (p,q) = (0,1), (0,2), (1,2) with r the third index: apq = M[p][q]; apq == 0 skips the pair; theta = (M[q][q] -
 *     M[p][p]) / (2*apq); t = 1 / (|theta| + sqrt(theta*theta + 1)), negated if theta < 0 (a theta that overflowed gives t = 0,
 *     the identity rotation); c = 1 / sqrt(t*t + 1), sn = t*c; M[p][p] = M[p][p] - t*apq, M[q][q] = M[q][q] + t*apq, M[p][q] =
 *     M[q][p] = 0; with arp = M[r][p], arq = M[r][q]: M[r][p] = M[p][r] = c*arp - sn*arq, M[r][q] = M[q][r] = sn*arp + c*arq; for
 *     k = 0..2 with vkp = V[k][p], vkq = V[k][q]: V[k][p] = c*vkp - sn*vkq, V[k][q] = sn*vkp + c*vkq.  The eigenpairs (M[i][i],
 *     column i of V) are sorted by descending eigenvalue, ties to the smaller index (an insertion sort with a strict >): v1, v2,
 *     v3.  det = (v1[0]*(v2[1]*v3[2] - v3[1]*v2[2]) - v2[0]*(v1[1]*v3[2] - v3[1]*v1[2])) + v3[0]*(v1[1]*v2[2] - v2[1]*v1[2]); det <
 *     0 negates v3.  (E v)[i] = (E[i][0]*v[0] + E[i][1]*v[1]) + E[i][2]*v[2], a.b = (a[0]*b[0] + a[1]*b[1]) + a[2]*b[2], |a| =
 *     sqrt(a.a).  w1 = E v1, sigma1 = |w1|, u1 = w1 / sigma1; w2 = E v2, g = w2.u1, w2[i] = w2[i] - g*u1[i], sigma2 = |w2|, u2 =
 *     w2 / sigma2; u3 = u1 x u2 (u3[0] = u1[1]*u2[2] - u1[2]*u2[1], cyclic); sigma3 = |E v3|.  R_a = U W V^T and R_b = U W^T V^T
 *     with W = [[0,-1,0],[1,0,0],[0,0,1]]: R_a[i][j] = (u2[i]*v1[j] - u1[i]*v2[j]) + u3[i]*v3[j], R_b[i][j] = (u1[i]*v2[j] -
 *     u2[i]*v1[j]) + u3[i]*v3[j].  The candidates are 0: (R_a, +u3), 1: (R_a, -u3), 2: (R_b, +u3), 3: (R_b, -u3).
 *     NO POSE: F^ all zeros; sigma1 not finite or not > 0; sigma2 not > 2^-20 * sigma1 (an F^ of rank 1); or, below, no vote.
 *   C. VOTE.  x1 = (((double)xf - cx)/fx, ((double)yf - cy)/fy, 1), x2 = (((double)tx - cx)/fx, ((double)ty - cy)/fy, 1).  For a
 *     candidate (R, t): r[i] = (R[i][0]*x1[0] + R[i][1]*x1[1]) + R[i][2]; c = r x x2, c0 = r1 - r2*x2[1], c1 = r2*x2[0] - r0, c2 =
 *     r0*x2[1] - r1*x2[0]; d = (c0*c0 + c1*c1) + c2*c2; a = x2 x t, a0 = x2[1]*t2 - t1, a1 = t0 - x2[0]*t2, a2 = x2[0]*t1 -
 *     x2[1]*t0; n1 = (a0*c0 + a1*c1) + a2*c2; b = r x t, b0 = r1*t2 - r2*t1, b1 = r2*t0 - r0*t2, b2 = r0*t1 - r1*t0; n2 = (b0*c0 +
 *     b1*c1) + b2*c2.  The depths are Z1 = n1/d in camera 1 and Z2 = n2/d in camera 2 (Z2 x2 = Z1 r + t crossed with x2 and with
 *     r); d = |r x x2|^2 is computed directly and not as |r|^2 |x2|^2 - (r.x2)^2, which cancels for a small parallax.  A voting
 *     pixel gives the candidate its vote iff 0 < d < +Inf && n1 > 0 && n2 > 0: in front of both cameras, with no division.
 *     (Negating t negates n1 and n2 exactly.)  Votes are integers in d_state[0..3].
 *   D. SELECT.  The candidate with the most votes, ties to the smaller index; all votes zero: NO POSE.  d_pose float64[16] = {R
 *     row-major [0..8], t [9..11], 1, sigma2/sigma1, sigma3/sigma1 [12..14], the candidate as a double [15]}; under NO POSE all
 *     zeros with [15] = -1.
 *   E. APPLY, every pixel whatever `step` and d_part are, each output optional (NULL to skip), with the winner's (R, t) and PARALLAX
 *     = 0 < d < +Inf.  d_depth (h,w) float32: (float)(n1/d) at a good pixel with parallax (negative behind camera 1), else 0.
 *     d_class (h,w) uint8: 0 not good; 1 parallax, n1 > 0 && n2 > 0; 2 parallax and not both; 3 good without parallax, and every
 *     good pixel under NO POSE.  d_err (h,w) float32: -1 at a pixel that is not good; with Z1 = n1/d, Y[i] = Z1*r[i] + t[i]: at a
 *     good pixel with parallax and Y[2] > 0, ex = ((fx*Y[0])/Y[2] + cx) - (double)tx, ey = ((fy*Y[1])/Y[2] + cy) - (double)ty,
 *     (float)sqrt(ex*ex + ey*ey), the reprojection error in pixels; +Inf at any other good pixel.  d_counts int32[8], zeroed by the
 *     call on the stream: {voting pixels, the winner's votes, the largest vote of the other three, the candidate (-1: none), pixels
 *     of class 1, of class 2, of class 3, 0}; under NO POSE the two votes are 0.
 * There is no d_ws: the scratch is d_state, int64[32], an output as well: [0..3] the votes, [4] the voting pixels, [5..7] the class
 * totals, [8..30] the bits of the float64 R_a, R_b, u3, sigma2/sigma1, sigma3/sigma1 (zeros without candidates), [31] 1 when B
 * gave candidates.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout; fx, then fy,
 * not finite or not > 0; cx, then cy, not finite; step outside [1,64]; any flag bit (there are none yet); a NULL d_flow, d_model,
 * d_pose or d_state; d_pose or d_state not 8-byte aligned, a float or int32 plane not 4-byte aligned; an output or scratch plane
 * equal to an input or to one listed before it.  4 launches and one or two memsets, whatever the planes hold.  Asynchronous on
 * `stream`, allocates nothing, reads nothing back, can be captured into a graph (after dflow_epipolar_fit, on one stream). */
int dflow_two_view(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        const float *d_model /* float32[9]: F^ as dflow_epipolar_fit leaves it */,
        const uint8_t *d_part /* NULL or (h,w): a pixel votes iff its byte == 1 */,
        double fx, double fy, double cx, double cy, int32_t step /* 1..64 */, uint32_t flags /* none yet */,
        double *d_pose       /* float64[16] */,
        int64_t *d_state     /* scratch+output int64[32], 8-byte aligned */,
        float *d_depth       /* NULL or (h,w) */, uint8_t *d_class /* NULL or (h,w) */, float *d_err /* NULL or (h,w) */,
        int32_t *d_counts    /* NULL or int32[8] */, void *stream);

/* Per-pixel confidence of a labelling (DESIGN.md "Label confidence"): how far the chosen label's local energy lies below the best
 * competing motion, the naive peak margin / local min-energy gap of a discrete labelling.  This build's definition; the reference
 * has no counterpart.  It reads the state the sweeps leave on the device and nothing of a pass's workspace.
 * Notation: LP = label_pitch; l = d_bestlabels[p]; n_p = min(d_nprop[p], LP); slot k of pixel p has flow f_k (unpacked as
 * everywhere else) and cost c_k = d_lcosts[p*LP+k].
 *   - p is LABELLED when 0 <= l < n_p.
 *   - s_k = sum over the 4-neighbours q of p that lie inside the frame and are labelled of min(tpsi, |f_k - g_q|_1), where g_q is
 *     the flow of q's chosen label.  An unlabelled neighbour adds nothing, as in dflow_bcd_stats.
 *   - e_k is computed in double, one IEEE operation per written operation, with no fused multiply-add.
 *       DFLOW_CONF_LOCAL: e_k = lamda * (double)c_k + (double)s_k.
 *       DFLOW_CONF_DATA:  e_k = (double)c_k.  This is the matching cost alone.  It is meaningful before any sweep and does not
 *                         need the neighbours.
 *   - Alternatives: A = { k < n_p : |f_k - f_l|_1 > min_sep }.  Duplicates and near-duplicates of the chosen motion do not
 *     compete.  The CLI default is 1, because the +-1 px neighbours of a motion have nearly its DAISY cost.
 *   - alt is the k in A with the smallest (e_k, k), so the smaller index wins a tie.
 *   - margin = (float)(e_alt - e_l): a subtraction in double, then one rounding to float32.
 *   - A negative margin is legal.  A BCD phase minimises chains, not pixels.
 *   - If A is empty: alt = -1, margin = +Inf.  If p is not labelled: alt = -1, margin = -Inf.
 *   - The costs of used slots are what the stages write: finite and >= 0 (no stage writes -0.0), as dflow_bcd_prepare already
 *     requires.  With anything else the values are unspecified, but nothing outside the arrays is touched.
 *   - Slots at or beyond n_p are never part of the result.
 * Outputs, each optional (NULL to skip) but not all four: d_margin (H,W) float32; d_alt (H,W) int32; d_sparse (H,W,3) float32,
 * [dx, dy, 1] where p is labelled and margin >= thresh (a float32 compare), [0,0,0] elsewhere; d_counts int32[DFLOW_CONF_COUNTS],
 * zeroed by the call on the stream = {labelled, not labelled, labelled with A empty, labelled with margin < 0, labelled with
 * margin == 0, kept}; kept is counted whether or not d_sparse is given.  All outputs are exact and independent of any order: the
 * same inputs give the same bytes on every call.
 * Of *p only pich, picw, maxnprop, label_pitch, tpsi and lamda are read and checked.  DFLOW_EINVAL before anything is launched,
 * checked in this order: the parameters as dflow_bcd_stats checks them (1 <= pich, picw <= 8192, label_pitch a multiple of 16 in
 * [16, DFLOW_MAX_LABELS], 1 <= maxnprop <= label_pitch, 1 <= tpsi <= 8); lamda not finite or < 0; mode outside [0,1]; min_sep
 * outside [0,1024]; thresh NaN (infinities are allowed); all four outputs NULL; a NULL input; d_proposals, d_lcosts or d_sparse not
 * 16-byte aligned, another plane not 4-byte aligned; an output equal to an input or to an output listed before it.
 * There is no workspace.  One launch and at most one memset; asynchronous on `stream`, allocates nothing, reads nothing back, can be
 * captured into a graph. */
#define DFLOW_CONF_LOCAL 0   /* e_k = lamda * c_k + s_k */
#define DFLOW_CONF_DATA  1   /* e_k = c_k */
#define DFLOW_CONF_COUNTS 6
int dflow_label_confidence(const dflow_params *p, const uint32_t *d_proposals, const float *d_lcosts, const int32_t *d_nprop,
                           const int32_t *d_bestlabels, int32_t mode, int32_t min_sep, float thresh,
                           float *d_margin, int32_t *d_alt, float *d_sparse, int32_t *d_counts, void *stream);

/* The gate of a flow field by a score plane (DESIGN.md "Label confidence"): a GOOD vector (as in dflow_flow_consistency) of d_flow,
 * (h,w,.) float32 in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout, whose score, d_score (h,w) float32, has lo <= score <= hi (float32
 * compares: a NaN score fails) is written to d_out (h,w,3) as [U,V,1] with its bits unchanged; every other pixel becomes [0,0,0].
 * Under DFLOW_EVAL_UVV d_out may be d_flow.  d_counts (NULL to skip) int32[2], zeroed by the call on the stream = {good, kept}.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout; lo or hi NaN
 * (infinities are allowed); lo > hi; a NULL d_flow, d_score or d_out; d_flow, d_score or d_out not 16-byte aligned (four pixels
 * per lane), d_counts not 4-byte aligned; an output equal to an input (but for d_out = d_flow as above) or to the other output.
 * One launch; asynchronous on `stream`, allocates nothing, reads nothing back, can be captured into a graph. */
int dflow_flow_gate(int32_t h, int32_t w, const float *d_flow, int32_t layout, const float *d_score, float lo, float hi,
                    float *d_out, int32_t *d_counts, void *stream);

/* Point trajectories through a frame sequence (DESIGN.md "Point trajectories"): tracks chained through the forward flows of
 * consecutive pairs and ended where the backward flow does not undo the step, the dense point trajectories of Sundaram, Brox and
 * Keutzer.  This build's definitions; the reference has no counterpart.  1 <= h, w <= 8192.  Flow fields are (h,w,.) float32 in
 * DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout; a vector is GOOD as in dflow_flow_consistency.  A position (x, y) is INSIDE when
 * x >= 0 && x <= (float)(w-1) && y >= 0 && y <= (float)(h-1) (a NaN is not).  Arithmetic is float32, one IEEE operation per
 * written operation; every result is an integer or a fixed float32 chain per track, independent of any order, and two calls give
 * the same bytes.
 * A TRACK SET of capacity cap, 1 <= cap <= 2^26: d_pos (cap,2) float32 [x,y], 8-byte aligned; d_state (cap) int32; d_birth (cap)
 * int32, the frame a track started in; d_n device int32[1], the number of slots handed out so far.  States: DFLOW_TRACK_FREE 0
 * (what a zeroed array holds), _LIVE 1, _LEFT 2 (it left the frame), _NOFLOW 3 (it met a forward vector that is not good),
 * _NOBACK 4 (it met a backward vector that is not good), _INCONSISTENT 5 (it failed the forward/backward test).  States >= 2 are
 * terminal: a slot is never reused and a terminal state never changes, so a track that is LIVE in two snapshots of a set is the
 * same trajectory throughout.
 * There is no workspace: scratch is passed as typed planes.  All three are asynchronous on `stream`, allocate nothing, read nothing
 * back and can be captured into a graph.
 *
 * ADVANCE.  A slot whose state is not LIVE is copied through, position bits included.  A LIVE slot at (x, y) takes the first of:
 *   LEFT          (x, y) is not inside.  Checked before anything is sampled: no value of d_pos_in makes a kernel read outside a plane.
 *   NOFLOW        the SAMPLE of d_fwd at (x, y) meets a vector that is not good.  SAMPLE of field F at an inside (x, y): y0 =
 *                 (int)floorf(y), ay = y - (float)y0, y1 = ay > 0 ? y0+1 : y0; x0, ax, x1 likewise (a corner of weight zero is not
 *                 looked at: it is the corner beside it); with Fij = F[yi][xj]: t = F00 + ax*(F01 - F00), b = F10 + ax*(F11 - F10),
 *                 value = t + ay*(b - t), for U and for V.
 *   LEFT          nx = x + U, ny = y + V, and (nx, ny) is not inside.
 *   with d_bwd:
 *   NOBACK        the sample (bu, bv) of d_bwd at (nx, ny) meets a vector that is not good.
 *   INCONSISTENT  du = U + bu, dv = V + bv, e2 = du*du + dv*dv, m2 = (U*U + V*V) + (bu*bu + bv*bv); not e2 <= rel*m2 + abs
 *                 (Sundaram-Brox: rel 0.01, abs 0.5).
 *   LIVE          otherwise; the position becomes (nx, ny).  A track that ends keeps its last position.
 * d_err (NULL to skip) (cap) float32: e2 where it was formed, -1 elsewhere.  d_counts (NULL to skip) int32[6], zeroed by the call on
 * the stream = {live after, left, noflow, noback, inconsistent, not live before}; they add up to cap.  d_pos_out may be d_pos_in
 * and d_state_out may be d_state_in (a lane touches only its own slot).  One launch and at most one memset.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout_fwd, with d_bwd
 * an unknown layout_bwd; cap outside [1,2^26]; rel, then abs, not finite or < 0; any flag bit (there are none yet); a NULL d_fwd,
 * d_pos_in, d_state_in, d_pos_out or d_state_out; d_pos_in or d_pos_out not 8-byte aligned, another plane not 4-byte aligned; an
 * output equal to an input (but for the two pairs above) or to an output listed before it. */
#define DFLOW_TRACK_FREE 0
#define DFLOW_TRACK_LIVE 1
#define DFLOW_TRACK_LEFT 2
#define DFLOW_TRACK_NOFLOW 3
#define DFLOW_TRACK_NOBACK 4
#define DFLOW_TRACK_INCONSISTENT 5
int dflow_track_advance(int32_t h, int32_t w, const float *d_fwd, int32_t layout_fwd,
                        const float *d_bwd /* NULL: no check */, int32_t layout_bwd, int32_t cap,
                        const float *d_pos_in, const int32_t *d_state_in, float rel, float abs, uint32_t flags /* none yet */,
                        float *d_pos_out, int32_t *d_state_out, float *d_err /* NULL or (cap) */,
                        int32_t *d_counts /* NULL or int32[6] */, void *stream);

/* SEED: new tracks where no live one is.  1 <= step <= 256; the CELLS are the gh x gw grid, gh = ceil(h/step), gw = ceil(w/step).
 * n = clamp(*d_n, 0, cap), read on the device.  A LIVE track among the slots i < n whose position is inside covers the cell
 * ((int)rintf(y) / step, (int)rintf(x) / step); one that is not inside covers nothing.  The SEED PIXEL of cell (cy, cx) is sx =
 * min(cx*step + step/2, w-1), sy = min(cy*step + step/2, h-1).  A cell is SEEDABLE when no track covers it and d_mask is NULL or
 * d_mask[sy*w + sx] != 0 (d_mask: (h,w) uint8).  The r-th seedable cell in raster order, r from 0, gets slot n + r if that is below
 * cap: position ((float)sx, (float)sy), LIVE, d_birth = frame; otherwise it is dropped.  Afterwards *d_n = min(cap, n + seedable).
 * d_counts (NULL to skip) int32[4], zeroed by the call on the stream = {covered cells, seedable cells, seeded, dropped}.
 * d_scan is int32 scratch of gh*gw + ceil(gh*gw / 1024) + 1 elements: the cells, a sum per 1024 cells, the n the call began with.
 * Two memsets (one without d_counts) and four launches whatever the set holds: mark (every writer of a cell stores the same
 * value), count per block, one block that scans the block sums, emit.  No workgroup waits for another.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; cap outside [1,2^26]; step
 * outside [1,256]; a NULL d_pos, d_state, d_birth, d_n or d_scan; d_pos not 8-byte aligned, another int32 plane not 4-byte
 * aligned; a plane equal to d_mask or to one listed before it (d_pos, d_state, d_birth, d_n, d_scan, d_counts). */
int dflow_track_seed(int32_t h, int32_t w, int32_t cap, int32_t step, int32_t frame,
                     const uint8_t *d_mask /* NULL or (h,w) */, float *d_pos, int32_t *d_state, int32_t *d_birth, int32_t *d_n,
                     int32_t *d_scan /* int32 scratch, see above */, int32_t *d_counts /* NULL or int32[4] */, void *stream);

/* FLOW: the displacement of every track that is LIVE in snapshot a and in snapshot b of one set, as a sparse field a -> b in the
 * format dflow_epic_interpolate, dflow_segment_filter and dflow_flow_eval take.  Track i TAKES PART if d_state_a[i] and
 * d_state_b[i] are both LIVE and its position in a is inside.  It claims pixel ((int)rintf(y_a), (int)rintf(x_a)) by an integer
 * minimum of i on d_owner (h,w) int32, which the call sets to 0x7fffffff first and leaves holding the winners: the smallest index
 * wins a shared pixel.  d_out (h,w,3) float32: [x_b - x_a, y_b - y_a, 1] of the winner at a claimed pixel, [0,0,0] elsewhere.
 * d_counts (NULL to skip) int32[3], zeroed by the call on the stream = {pixels set, tracks that lost their pixel, tracks that took
 * no part}; they add up to cap.  Two memsets (one without d_counts) and two launches.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; cap outside [1,2^26]; a NULL
 * d_pos_a, d_state_a, d_pos_b, d_state_b, d_owner or d_out; d_pos_a or d_pos_b not 8-byte aligned, another plane not 4-byte
 * aligned; d_owner, d_out or d_counts equal to a snapshot plane or to one listed before it (the two snapshots may be one). */
int dflow_track_flow(int32_t h, int32_t w, int32_t cap, const float *d_pos_a, const int32_t *d_state_a, const float *d_pos_b,
                     const int32_t *d_state_b, int32_t *d_owner /* (h,w) int32 */, float *d_out /* (h,w,3) */,
                     int32_t *d_counts /* NULL or int32[3] */, void *stream);

/* Superpixels (DESIGN.md "Superpixels and per-segment flow models"): an over-segmentation of an image into compact regions of
 * similar colour, an integer variant of gSLIC (Achanta et al.; Ren and Reid) whose segments are 4-connected and numbered 0 ..
 * n_seg-1.  This build's definition; the reference has no counterpart.  1 <= h, w <= 8192, n = h*w; d_bgr is (h,w,3) uint8 [b,g,r];
 * S = step, 4 <= S <= 64; m = compactness, 0 <= m <= 255; 1 <= iters <= 32; 0 <= min_size <= 2^26.  All arithmetic is unsigned
 * integer: the result depends on no order of arrival, and two calls give the same bytes.
 *   GRID.  gw = ceil(w/S), gh = ceil(h/S), K = gw*gh <= 2^22.  Centre k = gy*gw + gx is five numbers at 1/16 resolution, (cx16,
 *     cy16, b16, g16, r16), and starts as 16 times the position and the colours of pixel (x, y) = (min(gx*S + S/2, w-1), min(gy*S +
 *     S/2, h-1)).
 *   ASSIGNMENT.  Pixel (x, y) with colours (b, g, r) lies in cell (gy, gx) = (y/S, x/S) and considers the centres k of the cells
 *     (gy+dy, gx+dx), |dy|, |dx| <= 1, that exist.  dc2 = (16b - b16)^2 + (16g - g16)^2 + (16r - r16)^2, ds2 = (16x - cx16)^2 + (16y -
 *     cy16)^2, D' = S*S*dc2 + m*m*ds2, key = D' << 22 | k; the pixel takes the k of its smallest key, so at equal distance the
 *     smaller k wins.  Bounds: a centre is the rounded mean of pixels of its own 3x3 cells, so every coordinate difference is
 *     below 4*S*16 <= 2^12 and every colour difference below 2^12: dc2 < 2^26 and ds2 < 2^25 fit 32 bits, D' < 2^12 * 2^26 + 2^16 *
 *     2^25 < 2^42, and the key fits 64 bits.
 *   UPDATE.  Per centre: n, the number of its pixels, and the sums of x, y, b, g, r over them (each below 2^32: at most 9*S*S
 *     pixels).  Each of the five numbers becomes (16*sum + (n >> 1)) / n, a 64-bit integer division; a centre with n == 0 keeps
 *     its numbers.
 *   An ITERATION is one assignment followed by one update.  The raw labels are the assignment of iteration `iters`, the centres
 *     those after its update.
 *   COMPONENTS.  The 4-connected components of equal raw label.  A component's ROOT is its smallest raster index y*w + x, its size
 *     its number of pixels; it is SMALL if size < min_size.  The TARGET of a small component with root pixel (y0, x0) is the
 *     component of pixel (y0, x0-1) if x0 > 0, else of (y0-1, x0) if y0 > 0, else there is none.  That pixel is not of the
 *     component and the target's root is smaller, so targets form a forest.  A small component joins the component at the end of
 *     its chain of targets: the first that is not small, or the one that holds pixel 0.  (The order-independent counterpart of
 *     SLIC's "merge into the label seen just before".)  So every final segment is 4-connected, every final segment but possibly
 *     the one that holds pixel 0 has at least min_size pixels, and min_size 0 or 1 merges nothing.
 *   NUMBERING.  The final segments are numbered 0 .. n_seg-1 in the order of their smallest raster index.
 * Outputs: d_label (h,w) int32, the final segment number.  d_centers (K,8) int32: [cx16, cy16, b16, g16, r16, n of the last
 * assignment, 0, 0].  d_slic (NULL to skip) (h,w) int32: the raw label k.  d_counts (NULL to skip) int32[8], zeroed by the call on
 * the stream = {K, centres with n == 0 in the last assignment, components, small components (the one that holds pixel 0
 * included if it is small), pixels of components that joined another, n_seg, the size of the largest final segment, 0}.
 * There is no d_ws: the scratch is the caller's typed planes, all int32 and 4-byte aligned: d_sums (K,8), d_comp (h,w), d_size
 * (h,w), d_final (h,w) and d_scan, ceil(h*w / 256) + 1 elements.  What they hold afterwards is unspecified.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; step outside [4,64];
 * compactness outside [0,255]; iters outside [1,32]; min_size outside [0,67108864]; any flag bit (there are none yet); a NULL
 * d_bgr, d_label, d_centers, d_sums, d_comp, d_size, d_final or d_scan; an int32 plane not 4-byte aligned; an output or scratch
 * plane equal to d_bgr or to one listed before it (d_label, d_centers, d_slic, d_counts, d_sums, d_comp, d_size, d_final, d_scan).
 * 8 + 2 iters launches (the centres; an assignment fused with the accumulation and a division per iteration; seven for the
 * components, the merge, the scan and the numbering) and at most one memset, whatever the image holds.  Asynchronous on `stream`,
 * allocates nothing, reads nothing back, can be captured into a graph. */
#define DFLOW_SEGMENTS_MAX 67108864 /* 2^26 */
int dflow_superpixels(int32_t h, int32_t w, const uint8_t *d_bgr, int32_t step /* 4..64 */, int32_t compactness /* 0..255 */,
        int32_t iters /* 1..32 */, int32_t min_size /* 0..2^26 */, uint32_t flags /* none yet */,
        int32_t *d_label   /* (h,w) */, int32_t *d_centers /* (K,8) */,
        int32_t *d_slic    /* NULL or (h,w) */, int32_t *d_counts /* NULL or int32[8] */,
        int32_t *d_sums    /* scratch (K,8) */, int32_t *d_comp /* scratch (h,w) */, int32_t *d_size /* scratch (h,w) */,
        int32_t *d_final   /* scratch (h,w) */, int32_t *d_scan /* scratch int32[ceil(h*w/256) + 1] */, void *stream);

/* A robust affine flow model per segment (DESIGN.md "Superpixels and per-segment flow models"): trimmed least squares over the
 * vectors of every segment of a label plane.  This build's definition; the reference has no counterpart.  1 <= h, w <= 8192; d_flow
 * is (h,w,.) float32 in DFLOW_EVAL_UVV or DFLOW_EVAL_DYDX layout; a vector is GOOD as in dflow_flow_consistency.  d_label is (h,w)
 * int32, any label plane; 1 <= n_seg <= 2^26; thresh (pixels) finite and > 0; R = rounds, 1 <= R <= 6.  Pixel (x, y) with vector
 * (U,V) and label l TAKES PART if the vector is good, 0 <= l < n_seg, and fabsf(U) <= 32768 && fabsf(V) <= 32768.  Its quantities:
 * xf = (float)x, yf = (float)y, a = 2x - (w-1), b = 2y - (h-1), p = llrintf(U*64), q = llrintf(V*64).  Float32 and float64 chains
 * are one IEEE operation per written operation; everything else is an integer.  The result depends on no order of arrival, and two
 * calls give the same bytes.
 *   A MODEL is float32[6]: Um = (m0*xf + m1*yf) + m2, Vm = (m3*xf + m4*yf) + m5 (float32).  A pixel AGREES with it at T iff, with
 *     eu = U - Um, ev = V - Vm: eu*eu + ev*ev <= T*T (float32; a NaN anywhere makes it false).
 *   ROUND 0.  Per segment, over the pixels of its label that take part, the int64 sums N, Sa, Sb, Saa, Sab, Sbb, Sp, Sap, Sbp, Sq,
 *     Saq, Sbq (|a|, |b| < 2^13, |p|, |q| <= 2^21, at most 2^26 pixels: every sum stays below 2^60).  SOLVE as step E of
 *     dflow_motion_fit does: each sum is converted to float64 (one rounding), then c00 = Sbb*N - Sb*Sb, c01 = Sb*Sa - Sab*N, c02 =
 *     Sab*Sb - Sbb*Sa, c11 = Saa*N - Sa*Sa, c12 = Sa*Sab - Saa*Sb, c22 = Saa*Sbb - Sab*Sab, det = (Saa*c00 + Sab*c01) + Sa*c02; for
 *     (r0,r1,r2) = (Sap, Sbp, Sp): x0 = ((c00*r0 + c01*r1) + c02*r2)/det, x1 = ((c01*r0 + c11*r1) + c12*r2)/det, x2 = ((c02*r0 +
 *     c12*r1) + c22*r2)/det, m0 = (float)(x0*0.03125), m1 = (float)(x1*0.03125), m2 = (float)(((x2 - x0*(w-1)) - x1*(h-1))*0.015625);
 *     m3..m5 likewise from (Saq, Sbq, Sq).  p and q are the flow, not the target: the model is the flow's.  The solve FAILS with N <
 *     3, det zero or not finite, or a coefficient not finite.  A failed solve with N >= 1 gives the translation [0, 0,
 *     (float)(((double)Sp/(double)N)*0.015625), 0, 0, (float)(((double)Sq/(double)N)*0.015625)]; with N == 0 the segment has no
 *     model.
 *   ROUND r = 1 .. R-1.  The same sums over the pixels that take part and agree with the model of round r-1 at T_r = thresh *
 *     2^(R-1-r) (one float32 multiplication); a segment without a model has none that agree.  The same solve and the same
 *     translation; with N == 0 the model of the round before, and its kind, stay.  The last round fits what lies within thresh.
 * Outputs: d_models (n_seg,6) float32, zeros without a model.  d_seg_counts (n_seg,4) int32 = {pixels with this label, pixels that
 * take part, those of them that agree with the final model at thresh, the kind of the final model: 0 none, 1 translation, 2 affine}.
 * d_out (NULL to skip) (h,w,3) float32: [Um, Vm, 1] at every pixel whose label is in range and whose segment has a model, good
 * vector or not (holes inside a segment are filled); [0,0,0] elsewhere.  d_class (NULL to skip) (h,w) uint8: 0 takes no part, 1
 * agrees with its segment's final model at thresh, 2 does not, 3 takes part but its segment has no model.  d_counts (NULL to skip)
 * int32[8], zeroed by the call on the stream = {pixels that take part, of class 1, segments with a model, affine segments,
 * translation segments, pixels whose label is out of range, good vectors outside the 32768 range (whatever their label), 0}.
 * There is no d_ws: the scratch is the caller's typed plane d_acc (n_seg,12) int64, 8-byte aligned, which the call zeroes on the
 * stream and every round leaves zeroed.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; an unknown layout; n_seg outside
 * [1,67108864]; thresh not finite or not > 0; rounds outside [1,6]; any flag bit (there are none yet); a NULL d_flow, d_label,
 * d_models, d_seg_counts or d_acc; d_acc not 8-byte aligned, a float or int32 plane not 4-byte aligned; an output or scratch plane
 * equal to d_flow, d_label or to one listed before it (d_models, d_seg_counts, d_out, d_class, d_counts, d_acc).
 * 2 rounds + 1 launches (per round the sums, a wave's adds aggregated per distinct label first, and a thread per segment that
 * solves; then one that applies) and two or three memsets, whatever the planes hold.  Asynchronous on `stream`, allocates nothing,
 * reads nothing back, can be captured into a graph. */
int dflow_segment_fit(int32_t h, int32_t w, const float *d_flow, int32_t layout,
        const int32_t *d_label /* (h,w): any label plane */, int32_t n_seg /* 1..2^26 */,
        float thresh, int32_t rounds /* 1..6 */, uint32_t flags /* none yet */,
        float *d_models       /* (n_seg,6) */, int32_t *d_seg_counts /* (n_seg,4) */,
        float *d_out          /* NULL or (h,w,3) [U,V,valid] */, uint8_t *d_class /* NULL or (h,w) */,
        int32_t *d_counts     /* NULL or int32[8] */,
        int64_t *d_acc        /* scratch int64 (n_seg,12), 8-byte aligned */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFLOW_H */
