// Epipolar-geometry fit of a flow field (include/dflow.h: dflow_epipolar_fit; DESIGN.md "Epipolar-geometry fit"): the fundamental
// matrix most vectors of a flow field agree with, found by random 7-point samples, with the classes and the Sampson residual.
// This build's definition; the reference has no counterpart.  The model is kept in the centred, power-of-two scaled coordinates
// of motion_fit.hip's minimal solve: float32 scoring in pixel coordinates would cancel.
//
//   ep_hyp_kernel     one sample per lane: the Philox draws of its 7 points, the float64 elimination with complete pivoting of
//                     the 7 x 9 system (private memory: the pivots index it), the cubic det(alpha F1 + F2), its roots over the whole
//                     projective line by critical points and 60 bisections each, up to three float32 models into the slots
//                     3j .. 3j+2 of d_models; a slot without a model stores zeros and marks its count FIT_DEGENERATE
//   ep_score_kernel   the hot one.  A block stages a chunk of FIT_CHUNK scored pixels into LDS in normalised coordinates, two
//                     pixels per pair of 16-byte words, the pixels that take no part dropped; a lane owns a slot with its nine
//                     coefficients in registers and walks the chunk with broadcast 16-byte LDS reads, two pixels per packed
//                     float32 instruction; the count stays in the lane's register and ends in one integer atomic per lane.
//                     Grid = pixel chunks x groups of 256 slots; a wave whose slots are all degenerate leaves after the staging
//   ep_best_kernel    the 64-bit atomicMax of count << 32 | ~(round, slot); a degenerate count becomes 0
//   ep_select_kernel  one lane: the round's winner, if it beat the rounds before it, becomes the current model
//   ep_apply_kernel   one pixel per lane: class, residual, the scored pixels and the final model's scored inliers
//   ep_finish_kernel  one lane: d_counts is written from d_state
// 3 + 4 (lo_rounds + 1) launches and one or two memsets whatever the field holds.  Every count is an integer (exact in any order
// of arrival); every float32 and float64 chain is one IEEE operation per written operation (-ffp-contract=off).
// fit_common.h holds what this fit shares with motion_fit.hip: the arguments, the draw of a sample point, the chunk staging, the
// best key with its offer, its adoption and its counts, and the classes.  The coordinates a chunk holds, the slots of a sample,
// the solve, the score loop and the model a fit without a winner falls back to (all zeros) are this file's.
#include "fit_common.h"
#include "wave_ops.h"

#define EP_STRIDE 8                                   // counter slots per round and sample: a slot per point, one to spare
#define EP_BISECTIONS 60
// d_state: int64[32]
enum { EP_S_BEST = FIT_S_BEST, EP_S_SCORED, EP_S_DEGEN, EP_S_DEGEN0, EP_S_FINAL };

struct EpArgs {
    MfArgs f;                                         // n_hyp: samples; the slots are 3 n_hyp
    int slots;
    float cxf, cyf, sf, Pf, t2;                       // the normalisation in float32 (exact), (thresh*s)*(thresh*s)
};

// COORDINATES (include/dflow.h)
__device__ __forceinline__ static void ep_coords(const EpArgs &a, float xf, float yf, float U, float V, float &ca, float &cb,
                                                 float &cp, float &cq)
{
    ca = (xf - a.cxf) * a.sf; cb = (yf - a.cyf) * a.sf;
    cp = ((xf + U) - a.cxf) * a.sf; cq = ((yf + V) - a.cyf) * a.sf;
}

// 0 < den < +Inf: one v_cmp_class_f32 (positive normal or denormal)
__device__ __forceinline__ static bool ep_pos_finite(float den) { return __builtin_amdgcn_classf(den, 0x180); }

__device__ __forceinline__ static void ep_terms(const float (&m)[9], float ca, float cb, float cp, float cq, float &ee, float &den)
{
    const float l0 = (m[0] * ca + m[1] * cb) + m[2], l1 = (m[3] * ca + m[4] * cb) + m[5], l2 = (m[6] * ca + m[7] * cb) + m[8];
    const float e = (cp * l0 + cq * l1) + l2;
    const float m0 = (m[0] * cp + m[3] * cq) + m[6], m1 = (m[1] * cp + m[4] * cq) + m[7];
    den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    ee = e * e;
}

// INLIER (include/dflow.h)
__device__ __forceinline__ static bool ep_inlier(const float (&m)[9], float ca, float cb, float cp, float cq, float t2)
{
    float ee, den;
    ep_terms(m, ca, cb, cp, cq, ee, den);
    return ep_pos_finite(den) && ee <= t2 * den;
}

__device__ static inline double ep_det3(const double (&m)[9])
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// ROOTS of c3 x^3 + c2 x^2 + c1 x + c0 in [-1, 1] (closed) or (-1, 1), ascending: at most 4 (an exact zero at -1 and three pieces)
__device__ static int ep_cubic_roots(double c3, double c2, double c1, double c0, bool closed, double (&roots)[4])
{
    auto g = [&](double x) { return ((c3 * x + c2) * x + c1) * x + c0; };
    const double qa = 3.0 * c3, qb = 2.0 * c2;
    const double disc = qb * qb - (4.0 * qa) * c1;
    double pts[4];
    int np = 0, nr = 0;
    pts[np++] = -1.0;
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        const double qq = -0.5 * (qb + (qb < 0.0 ? -sq : sq));
        const double x1 = qq / qa, x2 = c1 / qq;
        const double xa = x1 < x2 ? x1 : x2, xb = x1 < x2 ? x2 : x1;
        if (-1.0 < xa && xa < 1.0) pts[np++] = xa;
        if (-1.0 < xb && xb < 1.0) pts[np++] = xb;
    }
    pts[np++] = 1.0;
    double gu = g(-1.0);
    if (closed && gu == 0.0) roots[nr++] = -1.0;
    for (int i = 1; i < np; i++) {
        const double u = pts[i - 1], v = pts[i], gv = g(v);
        if (gv == 0.0) {
            if (closed || v != 1.0) roots[nr++] = v;
        } else if ((gu < 0.0 && gv > 0.0) || (gu > 0.0 && gv < 0.0)) {
            double lo = u, hi = v;
            for (int t = 0; t < EP_BISECTIONS; t++) {
                const double mid = 0.5 * (lo + hi);
                if ((g(mid) < 0.0) == (gu < 0.0)) lo = mid; else hi = mid;
            }
            roots[nr++] = 0.5 * (lo + hi);
        }
        gu = gv;
    }
    return nr;
}

// CANONICAL SCALE, then the cast; false: an entry that is not finite
__device__ static bool ep_canonical(const double (&f)[9], float (&out)[9])
{
    int big = 0;
    for (int i = 1; i < 9; i++)
        if (fabs(f[i]) > fabs(f[big])) big = i;
    const double d = f[big];
    bool ok = true;
    for (int i = 0; i < 9; i++) { out[i] = (float)(f[i] / d); ok &= isfinite(out[i]); }
    return ok;
}

// ELIMINATION, CUBIC and ROOTS of one sample's 7 x 9 system -> the float32 models of its three slots; ok[m]: slot m holds one
__device__ static void ep_solve(double (&A)[7][9], float (&out)[3][9], bool (&ok)[3])
{
    ok[0] = ok[1] = ok[2] = false;
    int perm[9];
    for (int i = 0; i < 9; i++) perm[i] = i;
    for (int c = 0; c < 7; c++) {
        int pr = c, pk = c;
        double best = fabs(A[c][c]);
        for (int r = c; r < 7; r++)
            for (int k = c; k < 9; k++) {
                const double v = fabs(A[r][k]);
                if (v > best) { best = v; pr = r; pk = k; }
            }
        if (!(best >= FIT_PIVOT_MIN)) return;
        if (pr != c)
            for (int k = 0; k < 9; k++) { const double t = A[c][k]; A[c][k] = A[pr][k]; A[pr][k] = t; }
        if (pk != c) {
            for (int r = 0; r < 7; r++) { const double t = A[r][c]; A[r][c] = A[r][pk]; A[r][pk] = t; }
            const int t = perm[c]; perm[c] = perm[pk]; perm[pk] = t;
        }
        for (int r = c + 1; r < 7; r++) {
            const double f = A[r][c] / A[c][c];
            for (int k = c + 1; k < 9; k++) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
    double f1[9], f2[9];
    for (int q = 0; q < 2; q++) {
        double x[9];
        x[7] = q == 0 ? 1.0 : 0.0; x[8] = q == 0 ? 0.0 : 1.0;
        for (int r = 6; r >= 0; r--) {
            double t = -A[r][7 + q];
            for (int k = r + 1; k < 7; k++) t = t - A[r][k] * x[k];
            x[r] = t / A[r][r];
        }
        for (int i = 0; i < 9; i++) (q == 0 ? f1 : f2)[perm[i]] = x[i];
    }
    double sum[9], dif[9];
    for (int i = 0; i < 9; i++) { sum[i] = f1[i] + f2[i]; dif[i] = f2[i] - f1[i]; }
    const double k3 = ep_det3(f1), k0 = ep_det3(f2), dp = ep_det3(sum), dm = ep_det3(dif);
    const double k2 = (dp + dm) * 0.5 - k0, k1 = (dp - dm) * 0.5 - k3;
    if (!(isfinite(k0) && isfinite(k1) && isfinite(k2) && isfinite(k3))) return;
    double ra[4], rb[4];
    const int na = ep_cubic_roots(k3, k2, k1, k0, true, ra);          // F = alpha F1 + F2, alpha in [-1, 1]
    const int nb = ep_cubic_roots(k0, k1, k2, k3, false, rb);         // F = F1 + beta F2, beta in (-1, 1)
    for (int m = 0; m < 3 && m < na + nb; m++) {
        double f[9];
        if (m < na)
            for (int i = 0; i < 9; i++) f[i] = ra[m] * f1[i] + f2[i];
        else
            for (int i = 0; i < 9; i++) f[i] = f1[i] + rb[m - na] * f2[i];
        ok[m] = ep_canonical(f, out[m]);
    }
}

__global__ void __launch_bounds__(FIT_THREADS) ep_hyp_kernel(EpArgs a, int round)
{
    const int j = blockIdx.x * FIT_THREADS + threadIdx.x;
    if (j >= a.f.n_hyp) return;
    float cur[9];
    mf_load_model(a.f.cur, cur);
    uint32_t idx[7];
    double A[7][9];
    bool found_all = true;
    for (int k = 0; k < 7 && found_all; k++) {
        float xf, yf, U, V;
        found_all = fit_draw<EP_STRIDE>(a.f, j, round, k, idx, xf, yf, U, V, [&](float x, float y, float u, float v) {
            float ca, cb, cp, cq;
            ep_coords(a, x, y, u, v, ca, cb, cp, cq);
            return ep_inlier(cur, ca, cb, cp, cq, a.t2);
        });
        if (!found_all) break;
        const float tx = xf + U, ty = yf + V;
        const double da = ((double)xf - a.f.cx) * a.f.s, db = ((double)yf - a.f.cy) * a.f.s;
        const double dp = ((double)tx - a.f.cx) * a.f.s, dq = ((double)ty - a.f.cy) * a.f.s;
        double *row = A[k];
        row[0] = dp * da; row[1] = dp * db; row[2] = dp; row[3] = dq * da; row[4] = dq * db; row[5] = dq;
        row[6] = da; row[7] = db; row[8] = 1.0;
    }
    float out[3][9];
    bool ok[3] = {false, false, false};
    if (found_all) ep_solve(A, out, ok);
    for (int m = 0; m < 3; m++) {
        const size_t slot = (size_t)j * 3 + m;
        for (int k = 0; k < 9; k++) a.f.models[slot * 9 + k] = ok[m] ? out[m][k] : 0.0f;
        a.f.hyp_counts[slot] = ok[m] ? 0 : FIT_DEGENERATE;
    }
}

// Two pixels per instruction: the chunk lies in LDS as pairs, (a0, a1, b0, b1) and (p0, p1, q0, q1), so that the loads land in
// the register pairs v_pk_mul_f32 / v_pk_add_f32 take; each half is the IEEE operation of the scalar expression.
__global__ void __launch_bounds__(FIT_THREADS) ep_score_kernel(EpArgs a)
{
    __shared__ float4 s_px[FIT_CHUNK];
    __shared__ int s_n;
    const int np = fit_stage_chunk<FIT_CHUNK, FIT_THREADS>(a.f, s_px, s_n, [&](int x, int y, float U, float V, float (&v)[4]) {
        ep_coords(a, (float)x, (float)y, U, V, v[0], v[1], v[2], v[3]);
    });
    const int j = blockIdx.y * FIT_THREADS + threadIdx.x;
    const bool live = j < a.slots && a.f.hyp_counts[j] >= 0;      // the sign does not change while counts are added
    if (!__any(live)) return;                                     // the wave's slots are all degenerate; no barrier follows
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = 0.0f;                      // den = 0: a dead lane counts nothing
    if (live) mf_load_model(a.f.models + (size_t)j * 9, m);
    const float t2 = a.t2;
    int cnt = 0;
#pragma unroll 4
    for (int k = 0; k < (np + 1) >> 1; k++) {
        const float4 v0 = s_px[2 * k], v1 = s_px[2 * k + 1];      // every lane the same address: a broadcast
        const dflow_f2 ca = {v0.x, v0.y}, cb = {v0.z, v0.w}, cp = {v1.x, v1.y}, cq = {v1.z, v1.w};
        const dflow_f2 l0 = (m[0] * ca + m[1] * cb) + m[2], l1 = (m[3] * ca + m[4] * cb) + m[5], l2 = (m[6] * ca + m[7] * cb) + m[8];
        const dflow_f2 e = (cp * l0 + cq * l1) + l2;
        const dflow_f2 m0 = (m[0] * cp + m[3] * cq) + m[6], m1 = (m[1] * cp + m[4] * cq) + m[7];
        const dflow_f2 den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
        const dflow_f2 ee = e * e, rhs = t2 * den;
        cnt += (ep_pos_finite(den.x) && ee.x <= rhs.x ? 1 : 0) + (ep_pos_finite(den.y) && ee.y <= rhs.y ? 1 : 0);
    }
    if (live && cnt) atomicAdd(&a.f.hyp_counts[j], cnt);
}

__global__ void __launch_bounds__(FIT_THREADS) ep_best_kernel(EpArgs a, int round)
{
    const bool degenerate = fit_offer(a.f, blockIdx.x * FIT_THREADS + threadIdx.x, a.slots, round);
    fit_block_add({wave_count(degenerate)}, &a.f.state[EP_S_DEGEN]);
    fit_block_add({wave_count(degenerate && round == 0)}, &a.f.state[EP_S_DEGEN0]);
}

__global__ void ep_select_kernel(EpArgs a, int round)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long key = a.f.state[EP_S_BEST];
    if (key == 0ull) {
        for (int k = 0; k < 9; k++) a.f.cur[k] = 0.0f;
        return;
    }
    fit_adopt(a.f, key, round);
}

__global__ void __launch_bounds__(FIT_THREADS) ep_apply_kernel(EpArgs a, uint8_t *__restrict__ cls, float *__restrict__ residual)
{
    const uint32_t i = blockIdx.x * FIT_THREADS + threadIdx.x;
    bool scored = false, scored_in = false;
    if (i < a.f.n) {
        float m[9];
        mf_load_model(a.f.cur, m);
        const int y = (int)(i / (uint32_t)a.f.w), x = (int)(i % (uint32_t)a.f.w);
        float U = 0.0f, V = 0.0f;
        const bool good = flow_good(a.f.flow, a.f.layout, (size_t)i, U, V);
        const bool excluded = a.f.exclude && a.f.exclude[i];
        float ca, cb, cp, cq, ee, den;
        ep_coords(a, (float)x, (float)y, U, V, ca, cb, cp, cq);
        ep_terms(m, ca, cb, cp, cq, ee, den);
        const bool in = good && ep_pos_finite(den) && ee <= a.t2 * den;
        if (cls) cls[i] = fit_class(good, excluded, in);
        if (residual) residual[i] = !good ? -1.0f : ep_pos_finite(den) ? sqrtf(ee / den) * a.Pf : INFINITY;
        scored = fit_scored(a.f, good, excluded, x, y);
        scored_in = scored && in;
    }
    fit_block_add({wave_count(scored)}, &a.f.state[EP_S_SCORED]);
    fit_block_add({wave_count(scored_in)}, &a.f.state[EP_S_FINAL]);
}

__global__ void ep_finish_kernel(EpArgs a, int32_t *__restrict__ counts)
{
    if (blockIdx.x || threadIdx.x || !counts) return;
    fit_counts(a.f, counts, EP_S_SCORED, EP_S_FINAL, EP_S_DEGEN);
    counts[6] = (int32_t)((1000ll * ((long long)a.slots - (long long)a.f.state[EP_S_DEGEN0])) / (long long)a.f.n_hyp);
    counts[7] = 0;
}

int launch_epipolar_fit(int H, int W, const float *flow, int layout, const uint8_t *exclude, float thresh, int n_hyp, int lo_rounds,
                        int step, uint64_t seed, float *d_model, float *models, int32_t *hyp_counts, int64_t *state, uint8_t *cls,
                        float *residual, int32_t *counts, hipStream_t s)
{
    EpArgs a;
    a.f = fit_frame(H, W, layout, step, flow, state);
    a.f.n_hyp = n_hyp; a.f.k0 = (uint32_t)seed; a.f.k1 = (uint32_t)(seed >> 32); a.f.thresh = thresh;
    a.f.exclude = exclude; a.f.cur = d_model; a.f.models = models; a.f.hyp_counts = hyp_counts;
    a.slots = 3 * n_hyp;
    a.cxf = (float)a.f.cx; a.cyf = (float)a.f.cy; a.sf = (float)a.f.s; a.Pf = (float)a.f.inv;  // half-integers and powers of two: exact
    const float th = thresh * a.sf;
    a.t2 = th * th;
    if (int rc = fit_clear(state, counts, s)) return rc;
    const unsigned hyp_blocks = (unsigned)((n_hyp + FIT_THREADS - 1) / FIT_THREADS);
    const unsigned slot_blocks = (unsigned)((a.slots + FIT_THREADS - 1) / FIT_THREADS);
    const unsigned chunks = (a.f.ns + FIT_CHUNK - 1) / FIT_CHUNK;
    // no model until a round has a winner: round 0 does not look at it, the rounds after it sample its inliers
    hipLaunchKernelGGL(ep_select_kernel, dim3(1), dim3(64), 0, s, a, -1);
    for (int r = 0; r <= lo_rounds; r++) {
        hipLaunchKernelGGL(ep_hyp_kernel, dim3(hyp_blocks), dim3(FIT_THREADS), 0, s, a, r);
        hipLaunchKernelGGL(ep_score_kernel, dim3(chunks, slot_blocks), dim3(FIT_THREADS), 0, s, a);
        hipLaunchKernelGGL(ep_best_kernel, dim3(slot_blocks), dim3(FIT_THREADS), 0, s, a, r);
        hipLaunchKernelGGL(ep_select_kernel, dim3(1), dim3(64), 0, s, a, r);
    }
    hipLaunchKernelGGL(ep_apply_kernel, dim3((a.f.n + FIT_THREADS - 1) / FIT_THREADS), dim3(FIT_THREADS), 0, s, a, cls, residual);
    hipLaunchKernelGGL(ep_finish_kernel, dim3(1), dim3(64), 0, s, a, counts);
    return dflow_check_launch("epipolar fit kernels");
}
