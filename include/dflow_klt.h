/*
 * dflow_klt.h -- sparse feature tracking of libdflow.so: a grey image pyramid, Shi-Tomasi corners and pyramidal Lucas-Kanade
 * over a track set (DESIGN.md "Sparse feature tracking").  This build's definitions; the reference has no counterpart.
 *
 * The conventions of dflow.h hold: device pointers owned by the caller, `stream` a hipStream_t passed as void*, 0 or a negative
 * DFLOW_E* code, dflow_last_error() for the message.  There is no workspace: scratch is passed as typed planes.  Every call is
 * asynchronous on `stream`, allocates nothing, reads nothing back, can be captured into a graph, launches the same kernels whatever
 * the data hold, and makes every refusal before anything is launched.  Every result is an integer, or a fixed chain of IEEE
 * float32 / float64 operations on integers (one operation per written operation): it depends on no order of arrival, and two calls
 * give the same bytes.  Frame sizes: 1 <= h, w <= 8192.  A position (x, y) is INSIDE a (h, w) frame as in dflow_track_advance.
 *
 * Alignment of data planes: d_bgr, d_pyr of dflow_klt_pyramid 4 (four pixels move at a time); d_pos, d_pos_in, d_pos_out, d_back 8 (a
 * position moves as one float2); every float and int32 plane 4; the pyramids the other two calls read, d_mask and d_occ 1.
 */
#ifndef DFLOW_KLT_H
#define DFLOW_KLT_H

#include "dflow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PYRAMID.  1 <= levels <= 8.  Level 0 is the grey image of d_bgr ((h,w,3) uint8 [b,g,r]): Y = (29 b + 150 g + 77 r + 128) >> 8,
 * (h,w) uint8.  Level l+1 has the size (h', w') = ((h_l + 1) / 2, (w_l + 1) / 2) and is dflow_pyr_down's formula on the one channel
 * of level l: pixel (y, x) = (sum over i, j = -2..2 of k[i] k[j] L_l[cy(2y + i)][cx(2x + j)] + 128) >> 8, k = [1,4,6,4,1], cy and
 * cx clamping an index into level l.  d_pyr is one uint8 buffer of dflow_klt_pyramid_bytes(h, w, levels) bytes: level l starts at
 * the byte offset sum over k < l of h_k w_k, its rows w_l bytes apart.  `levels` launches, no memset.
 * dflow_klt_pyramid_bytes returns 0, and sets the message, for a frame size outside [1,8192] or levels outside [1,8].
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; levels outside [1,8]; a NULL
 * d_bgr or d_pyr; d_bgr or d_pyr not 4-byte aligned; d_pyr equal to d_bgr. */
size_t dflow_klt_pyramid_bytes(int32_t h, int32_t w, int32_t levels);
int dflow_klt_pyramid(int32_t h, int32_t w, int32_t levels, const uint8_t *d_bgr, uint8_t *d_pyr, void *stream);

/* CORNERS of level 0 of a pyramid, Y = the first h*w bytes of d_pyr.  rc: window radius, 1..7; min_dist 1..32; border 0..8192;
 * quality in [0,1]; min_response finite and >= 0.
 *   RESPONSE.  gx(y, x) = Y[y][cx(x+1)] - Y[y][cx(x-1)], gy(y, x) = Y[cy(y+1)][x] - Y[cy(y-1)][x].  Over the (2 rc + 1)^2 window
 *     of pixel (y, x), every window position (y', x') clamped into the frame: a = sum gx^2, b = sum gx gy, c = sum gy^2, exact
 *     integers below 2^24.  R = max(0, ((double)(a + c) - sqrt((double)((a - c)^2 + 4 b^2))) * 0.5), rounded once to float32: the
 *     smaller eigenvalue of the window's structure tensor (Shi-Tomasi).  The radicand is an int64 below 2^53; sqrt is IEEE.
 *   THRESHOLD.  Rmax = the maximum of R over the plane, an integer maximum on the bits of the non-negative floats, kept in d_rmax;
 *     thr = (float)quality * Rmax, one float32 multiplication.
 *   CANDIDATE.  border <= x <= w-1-border, border <= y <= h-1-border, R >= thr, R >= min_response and R > 0.
 *   MAXIMUM.  A candidate none of whose (2 min_dist + 1)^2 window's pixels, the window clipped to the frame, has a larger R, or an
 *     equal R and a smaller raster index y*w + x.
 *   OCCUPATION, with a track set (d_pos, d_state, d_n and d_occ all given; all NULL without one): cap, d_pos (cap,2) float32,
 *     d_state (cap) int32 and d_n int32[1] as in dflow_track_seed.  A slot i < clamp(*d_n, 0, cap), read on the device, that is
 *     LIVE and inside occupies pixel ((int)rintf(y), (int)rintf(x)) of d_occ, (h,w) uint8 scratch that the call zeroes first;
 *     every writer stores the same value.  A maximum with an occupied pixel in its clipped (2 min_dist + 1)^2 window is SUPPRESSED.
 *   A CORNER is a maximum that is not suppressed.
 * Outputs: d_response (h,w) float32, R.  d_mask (h,w) uint8: 255 at a corner, 0 elsewhere; the plane dflow_track_seed takes: with
 * step 1 the r-th corner in raster order becomes slot n + r.  d_rmax uint32[1] scratch: the bits of Rmax.  d_counts (NULL to skip)
 * int32[4], zeroed by the call on the stream = {candidates, maxima, suppressed, corners}.
 * Three launches (response, mark, select) and up to three memsets (d_rmax, d_occ, d_counts); without a set two and up to two.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; rc outside [1,7]; min_dist
 * outside [1,32]; border outside [0,8192]; quality not finite or < 0, then > 1; min_response not finite or < 0; with any of d_pos,
 * d_state, d_n, d_occ given: cap outside [1,2^26], then a NULL d_pos, d_state, d_n or d_occ; a NULL d_pyr, d_response, d_mask or
 * d_rmax; d_pos not 8-byte aligned, d_state, d_n, d_response, d_rmax or d_counts not 4-byte aligned; an output or scratch plane
 * equal to d_pyr, d_pos, d_state, d_n or to one listed before it (d_response, d_mask, d_occ, d_rmax, d_counts). */
int dflow_corners(int32_t h, int32_t w, const uint8_t *d_pyr, int32_t rc, int32_t min_dist, int32_t border, float quality,
                  float min_response, int32_t cap, const float *d_pos, const int32_t *d_state, const int32_t *d_n,
                  float *d_response, uint8_t *d_mask, uint8_t *d_occ /* NULL or (h,w) scratch */, uint32_t *d_rmax,
                  int32_t *d_counts /* NULL or int32[4] */, void *stream);

/* TRACK: pyramidal Lucas-Kanade over a track set, with the template's gradients (the 2x2 matrix is formed once per level).
 * d_pyr1, d_pyr2: the pyramids of the two frames, same h, w, levels (1..8).  cap 1..2^26, d_pos_in (cap,2) float32 [x,y],
 * d_state_in (cap) int32.  r: window radius 1..10, n = (2r+1)^2; iters 1..64; eps finite > 0 (pixels); min_eig finite >= 0
 * (grey^2/px^2); max_err finite >= 0 (grey levels), 0: no test; fb finite >= 0 (pixels), 0: no backward pass.
 *   A slot that is not LIVE is copied through, position bits included.  A LIVE slot whose position p is not inside the frame
 *   becomes LEFT before anything is sampled.  Every other slot runs PASS(pyramid 1, pyramid 2, p).
 *   SAMPLE(G, x, y), G a level of size (hl, wl), x and y float32: x0 = floorf(x), ax = x - x0, y0 = floorf(y), ay = y - y0;
 *     w00 = (int)rintf(((1-ax)*(1-ay))*16384.f), w01 = (int)rintf((ax*(1-ay))*16384.f), w10 = (int)rintf(((1-ax)*ay)*16384.f),
 *     w11 = 16384 - w00 - w01 - w10; value = (w00 G[cy(y0)][cx(x0)] + w01 G[cy(y0)][cx(x0+1)] + w10 G[cy(y0+1)][cx(x0)]
 *     + w11 G[cy(y0+1)][cx(x0+1)] + 256) >> 9, an integer in [0, 8160] = 32 * grey.  cx and cy clamp an index into the level: no
 *     position reads outside a plane.
 *   PASS(Ga, Gb, p) -> LIVE at q, or LEFT, FLAT or RESIDUAL.  d = (0, 0), float32.  For l = levels-1 down to 0, with s = 2^-l,
 *     pl = (p.x * s, p.y * s), and below the top level first d = (2 d.x, 2 d.y):
 *     1. T[i][j] = SAMPLE(Ga_l, pl.x + (float)j, pl.y + (float)i), i, j = -r-1 .. r+1.  On the inner window i, j = -r .. r:
 *        Ix = T[i][j+1] - T[i][j-1], Iy = T[i+1][j] - T[i-1][j]; A = sum Ix^2, B = sum Ix Iy, C = sum Iy^2, int64, each below 2^53 and
 *        converted to float64 exactly.  D = A*C - B*B; lam = ((A + C) - sqrt((A - C)*(A - C) + 4.0*(B*B))) * 0.5 / (4096.0 * n).  The
 *        level is FLAT when lam < min_eig or not D > 0.  A flat level above 0 is skipped (d goes down as it is); a flat level 0
 *        ends the pass FLAT.
 *     2. Up to iters times: q = pl + d.  Above level 0, q.x = min(max(q.x, 0), wl-1), q.y likewise, and d = q - pl (always, not
 *        only where the clamp acted).  At level 0 a q that is not inside ends the pass LEFT.  On the inner window e[i][j] =
 *        SAMPLE(Gb_l, q.x + (float)j, q.y + (float)i) - T[i][j]; bx = sum e Ix, by = sum e Iy, int64, converted to float64;
 *        dx = -2.0*((C*bx - B*by)/D), dy = -2.0*((A*by - B*bx)/D); d.x += (float)dx, d.y += (float)dy; the loop stops when
 *        dx*dx + dy*dy < eps*eps (float64, eps converted): the level has CONVERGED.
 *     3. After level 0: q = p + d; a q that is not inside ends the pass LEFT.  err = (float)((double)(sum |e|) / (32.0 * n)), e
 *        taken at this q.  With max_err > 0 and err > max_err the pass ends RESIDUAL.  Otherwise LIVE at q.
 *   With fb > 0 a forward pass that ended LIVE at q is followed by PASS(pyramid 2, pyramid 1, q) -> p'.  The slot is INCONSISTENT
 *   when that pass does not end LIVE, or when bx*bx + by*by > fb*fb with bx = p'.x - p.x, by = p'.y - p.y (float32).
 *   The slot's new state is LIVE with position q, or the terminal state with its old position: a track that ends keeps its last
 *   position.  LEFT and INCONSISTENT are dflow.h's; DFLOW_TRACK_FLAT and DFLOW_TRACK_RESIDUAL are new, and terminal like them.
 * Outputs: d_pos_out, d_state_out; d_pos_out may be d_pos_in and d_state_out may be d_state_in (a lane group touches only its own
 * slot).  d_err (NULL to skip) (cap) float32: the forward pass's err where it was formed, -1 elsewhere.  d_back (NULL to skip)
 * (cap,2) float32: p' where the backward pass ended LIVE, NaN elsewhere.  d_counts (NULL to skip) int32[8], zeroed by the call on the
 * stream = {live after, left, flat, residual, inconsistent, not live before, slots whose forward pass converged at level 0, 0};
 * the first six add up to cap.
 * One launch (a 16-lane group per slot carries it through every level and both passes) and at most one memset.
 * DFLOW_EINVAL before anything is launched, checked in this order: a frame size outside [1,8192]; levels outside [1,8]; cap
 * outside [1,2^26]; r outside [1,10]; iters outside [1,64]; eps not finite or not > 0; min_eig, then max_err, then fb not finite or
 * < 0; any flag bit (there are none yet); a NULL d_pyr1, d_pyr2, d_pos_in, d_state_in, d_pos_out or d_state_out; d_pos_in,
 * d_pos_out or d_back not 8-byte aligned, d_state_in, d_state_out, d_err or d_counts not 4-byte aligned; an output equal to d_pyr1,
 * d_pyr2, d_pos_in, d_state_in (but for the two pairs above) or to an output listed before it (d_pos_out, d_state_out, d_err,
 * d_back, d_counts). */
#define DFLOW_TRACK_FLAT 6
#define DFLOW_TRACK_RESIDUAL 7
int dflow_klt_track(int32_t h, int32_t w, int32_t levels, const uint8_t *d_pyr1, const uint8_t *d_pyr2, int32_t cap,
                    const float *d_pos_in, const int32_t *d_state_in, int32_t r, int32_t iters, float eps, float min_eig,
                    float max_err, float fb, uint32_t flags /* none yet */, float *d_pos_out, int32_t *d_state_out,
                    float *d_err /* NULL or (cap) */, float *d_back /* NULL or (cap,2) */, int32_t *d_counts /* NULL or int32[8] */,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFLOW_KLT_H */
