// Robust global-motion fit of a flow field (include/dflow.h: dflow_motion_fit; DESIGN.md "Global-motion fit"): an affine map or a
// homography fitted to a flow field by random minimal samples, with the classes, the model's own flow and the residual.  This
// build's definition; the reference has no counterpart.
//
//   mf_hyp_kernel     one hypothesis per lane: the Philox draws of its 3 or 4 points, the float64 minimal solve (Gaussian
//                     elimination with partial pivoting in centred, power-of-two scaled coordinates), the float32 model into
//                     d_models; a degenerate one stores the identity and marks its count FIT_DEGENERATE
//   mf_score_kernel   the hot one.  A block stages a chunk of FIT_CHUNK scored pixels into LDS, two pixels per pair of 16-byte
//                     words, the pixels that take no part dropped; a lane owns a hypothesis with its coefficients in registers
//                     and walks the chunk with broadcast 16-byte LDS reads, two pixels per packed float32 instruction; the count
//                     stays in the lane's register and ends in one integer atomic per lane.  Grid = pixel chunks x groups of 256
//                     hypotheses.  Affine is the specialisation W = 1
//   mf_best_kernel    the 64-bit atomicMax of count << 32 | ~(round, index); a degenerate count becomes 0
//   mf_select_kernel  one lane: the round's winner, if it beat the rounds before it, becomes the current model
//   mf_sums_kernel, mf_solve_kernel, mf_count_kernel, mf_accept_kernel   one polish step: twelve int64 sums over the current
//                     model's scored inliers, the two 3x3 normal systems in float64, the candidate's inliers, the exchange
//   mf_apply_kernel   one pixel per lane: class, model flow, residual, the scored pixels and the final model's scored inliers
//   mf_finish_kernel  one lane: d_model stays, d_counts is written from d_state
// 3 + 4 (lo_rounds + 1) + 4 polish launches and one or two memsets whatever the field holds.  Every count and sum is an integer
// (exact in any order of arrival); every float32 and float64 chain is one IEEE operation per written operation
// (-ffp-contract=off).
#include "fit_common.h"      // what every fit shares: the arguments, the draw, the chunk, the best key, the classes, step E
#include "wave_ops.h"

#define MF_STRIDE 4                                   // counter slots per round and hypothesis: a slot per point
// d_state: int64[32]
enum { MF_S_BEST = FIT_S_BEST, MF_S_SCORED, MF_S_DEGEN, MF_S_CUR, MF_S_ACCEPTED, MF_S_SKIPPED, MF_S_CAND, MF_S_FINAL, MF_S_SUMS /* 8..19 */,
       MF_S_CAND_MODEL = 20 /* float32[9] in 20..24 */, MF_S_CAND_OK = 25 };

// INLIER (include/dflow.h, B and D)
__device__ __forceinline__ static bool mf_inlier(const float (&m)[9], float xf, float yf, float tx, float ty, float thresh)
{
    const float X = (m[0] * xf + m[1] * yf) + m[2], Y = (m[3] * xf + m[4] * yf) + m[5], W = (m[6] * xf + m[7] * yf) + m[8];
    const float ex = X - W * tx, ey = Y - W * ty, t = thresh * W;
    return W > 0.0f && ex * ex + ey * ey <= t * t;
}

__device__ static inline void mf_identity(float (&m)[9])
{
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = k % 4 == 0 ? 1.0f : 0.0f;
}

// Gaussian elimination with partial pivoting of the N x (N + R) system A, the first largest pivot winning, then the back
// substitutions: x[r] solves right-hand side r.  false: a pivot below FIT_PIVOT_MIN (or a NaN).
template <int N, int R> __device__ static bool mf_gauss(double (&A)[N][N + R], double (&x)[R][N])
{
    for (int c = 0; c < N; c++) {
        int piv = c;
        double best = fabs(A[c][c]);
        for (int r = c + 1; r < N; r++) {
            const double v = fabs(A[r][c]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best >= FIT_PIVOT_MIN)) return false;
        if (piv != c)
            for (int k = 0; k < N + R; k++) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
        for (int r = c + 1; r < N; r++) {
            const double f = A[r][c] / A[c][c];
            for (int k = c + 1; k < N + R; k++) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
    for (int q = 0; q < R; q++)
        for (int r = N - 1; r >= 0; r--) {
            double s = A[r][N + q];
            for (int k = r + 1; k < N; k++) s = s - A[r][k] * x[q][k];
            x[q][r] = s / A[r][r];
        }
    return true;
}

__global__ void __launch_bounds__(FIT_THREADS) mf_hyp_kernel(MfArgs a, int round)
{
    const int j = blockIdx.x * FIT_THREADS + threadIdx.x;
    if (j >= a.n_hyp) return;
    const int m = a.model == DFLOW_MOTION_HOMOGRAPHY ? 4 : 3;
    float cur[9];
    mf_load_model(a.cur, cur);
    uint32_t idx[4];
    float sx[4], sy[4], tx[4], ty[4];
    bool ok = true;
    for (int k = 0; k < m && ok; k++) {
        float U, V;
        ok = fit_draw<MF_STRIDE>(a, j, round, k, idx, sx[k], sy[k], U, V, [&](float xf, float yf, float u, float v) {
            return mf_inlier(cur, xf, yf, xf + u, yf + v, a.thresh);
        });
        if (ok) { tx[k] = sx[k] + U; ty[k] = sy[k] + V; }
    }
    double nm[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 1.0}};       // the model in normalised coordinates
    if (ok) {
        double ca[4], cb[4], cp[4], cq[4];
        for (int k = 0; k < m; k++) {
            ca[k] = ((double)sx[k] - a.cx) * a.s; cb[k] = ((double)sy[k] - a.cy) * a.s;
            cp[k] = ((double)tx[k] - a.cx) * a.s; cq[k] = ((double)ty[k] - a.cy) * a.s;
        }
        if (m == 3) {
            double A[3][5], x[2][3];
            for (int k = 0; k < 3; k++) { A[k][0] = ca[k]; A[k][1] = cb[k]; A[k][2] = 1.0; A[k][3] = cp[k]; A[k][4] = cq[k]; }
            ok = mf_gauss<3, 2>(A, x);
            if (ok)
                for (int c = 0; c < 3; c++) { nm[0][c] = x[0][c]; nm[1][c] = x[1][c]; }
        } else {
            double A[8][9], x[1][8];
            for (int k = 0; k < 4; k++) {
                double *r0 = A[2 * k], *r1 = A[2 * k + 1];
                r0[0] = ca[k]; r0[1] = cb[k]; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
                r0[6] = -(ca[k] * cp[k]); r0[7] = -(cb[k] * cp[k]); r0[8] = cp[k];
                r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = ca[k]; r1[4] = cb[k]; r1[5] = 1.0;
                r1[6] = -(ca[k] * cq[k]); r1[7] = -(cb[k] * cq[k]); r1[8] = cq[k];
            }
            ok = mf_gauss<8, 1>(A, x);
            if (ok)
                for (int c = 0; c < 8; c++) nm[c / 3][c % 3] = x[0][c];
        }
    }
    float mo[9];
    if (ok) {
        // to pixel coordinates: M = T^-1 N T, T: (x, y) -> ((x - cx) s, (y - cy) s)
        double R[3][3];
        for (int i = 0; i < 3; i++) {
            const double r0 = nm[i][0] * a.s, r1 = nm[i][1] * a.s;
            R[i][0] = r0; R[i][1] = r1; R[i][2] = (nm[i][2] - r0 * a.cx) - r1 * a.cy;
        }
        for (int c = 0; c < 3; c++) {
            mo[c] = (float)(a.inv * R[0][c] + a.cx * R[2][c]);
            mo[3 + c] = (float)(a.inv * R[1][c] + a.cy * R[2][c]);
            mo[6 + c] = (float)R[2][c];
        }
        for (int k = 0; k < 9; k++) ok &= isfinite(mo[k]);
        if (m == 4)
            for (int k = 0; k < 4; k++) ok &= (mo[6] * sx[k] + mo[7] * sy[k]) + mo[8] > 0.0f;
    }
    if (!ok) mf_identity(mo);
    for (int k = 0; k < 9; k++) a.models[(size_t)j * 9 + k] = mo[k];
    a.hyp_counts[j] = ok ? 0 : FIT_DEGENERATE;
}

// Two pixels per instruction: the chunk lies in LDS as pairs, (x0, x1, y0, y1) and (tx0, tx1, ty0, ty1), so that the loads land
// in the register pairs v_pk_mul_f32 / v_pk_add_f32 take; each half is the IEEE operation of the scalar expression.
template <bool HOMOG> __global__ void __launch_bounds__(FIT_THREADS) mf_score_kernel(MfArgs a)
{
    __shared__ float4 s_px[FIT_CHUNK];
    __shared__ int s_n;
    const int np = fit_stage_chunk<FIT_CHUNK, FIT_THREADS>(a, s_px, s_n, [](int x, int y, float U, float V, float (&v)[4]) {
        v[0] = (float)x; v[1] = (float)y; v[2] = v[0] + U; v[3] = v[1] + V;
    });
    const int j = blockIdx.y * FIT_THREADS + threadIdx.x;
    const bool live = j < a.n_hyp && a.hyp_counts[j] >= 0;        // the sign does not change while counts are added
    float m[9];
    mf_identity(m);
    if (live) mf_load_model(a.models + (size_t)j * 9, m);
    const float thresh = a.thresh, t2 = thresh * thresh;          // (thresh * 1) * (thresh * 1)
    int cnt = 0;
#pragma unroll 4
    for (int k = 0; k < (np + 1) >> 1; k++) {
        const float4 p = s_px[2 * k], q = s_px[2 * k + 1];        // every lane the same address: a broadcast
        const dflow_f2 xf = {p.x, p.y}, yf = {p.z, p.w}, tx = {q.x, q.y}, ty = {q.z, q.w};
        const dflow_f2 X = (m[0] * xf + m[1] * yf) + m[2], Y = (m[3] * xf + m[4] * yf) + m[5];
        if constexpr (HOMOG) {
            const dflow_f2 W = (m[6] * xf + m[7] * yf) + m[8];
            const dflow_f2 ex = X - W * tx, ey = Y - W * ty, t = thresh * W, e = ex * ex + ey * ey, tt = t * t;
            cnt += (W.x > 0.0f && e.x <= tt.x ? 1 : 0) + (W.y > 0.0f && e.y <= tt.y ? 1 : 0);
        } else {
            // W = (0 * xf + 0 * yf) + 1 = 1: W * tx = tx, thresh * W = thresh, bit for bit
            const dflow_f2 ex = X - tx, ey = Y - ty, e = ex * ex + ey * ey;
            cnt += (e.x <= t2 ? 1 : 0) + (e.y <= t2 ? 1 : 0);
        }
    }
    if (live && cnt) atomicAdd(&a.hyp_counts[j], cnt);
}

__global__ void __launch_bounds__(FIT_THREADS) mf_best_kernel(MfArgs a, int round)
{
    const bool degenerate = fit_offer(a, blockIdx.x * FIT_THREADS + threadIdx.x, a.n_hyp, round);
    fit_block_add({wave_count(degenerate)}, &a.state[MF_S_DEGEN]);
}

__global__ void mf_select_kernel(MfArgs a, int round)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long key = a.state[MF_S_BEST];
    if (key == 0ull) {
        float m[9];
        mf_identity(m);
        for (int k = 0; k < 9; k++) a.cur[k] = m[k];
        return;
    }
    if (fit_adopt(a, key, round)) a.state[MF_S_CUR] = fit_key_count(key);
}

struct MfSums { long long v[FIT_NSUMS]; long long skipped; };

__global__ void __launch_bounds__(FIT_THREADS) mf_sums_kernel(MfArgs a)
{
    MfSums s = {};
    if (a.state[MF_S_BEST] != 0ull) {
        float m[9];
        mf_load_model(a.cur, m);
        for (uint32_t c = blockIdx.x * FIT_THREADS + threadIdx.x; c < a.ns; c += gridDim.x * FIT_THREADS) {
            int x, y;
            const uint32_t i = mf_grid_pixel(a, c, x, y);
            float U, V;
            if (!mf_part(a, i, U, V)) continue;
            const float xf = (float)x, yf = (float)y, tx = xf + U, ty = yf + V;
            if (!mf_inlier(m, xf, yf, tx, ty, a.thresh)) continue;
            if (!(fabsf(tx) <= FIT_RANGE && fabsf(ty) <= FIT_RANGE)) { s.skipped++; continue; }
            const long long ca = 2 * x - (a.w - 1), cb = 2 * y - (a.h - 1), p = llrintf(tx * 64.0f), q = llrintf(ty * 64.0f);
            s.v[0] += 1; s.v[1] += ca; s.v[2] += cb; s.v[3] += ca * ca; s.v[4] += ca * cb; s.v[5] += cb * cb;
            s.v[6] += p; s.v[7] += ca * p; s.v[8] += cb * p; s.v[9] += q; s.v[10] += ca * q; s.v[11] += cb * q;
        }
    }
    s = block_reduce<FIT_THREADS / 64>(s, [](MfSums &x, const MfSums &y) {
#pragma unroll
        for (int k = 0; k < FIT_NSUMS; k++) x.v[k] += y.v[k];
        x.skipped += y.skipped;
    });
    if (threadIdx.x == 0) {
        for (int k = 0; k < FIT_NSUMS; k++)
            if (s.v[k]) atomicAdd(&a.state[MF_S_SUMS + k], (unsigned long long)s.v[k]);
        if (s.skipped) atomicAdd(&a.state[MF_S_SKIPPED], (unsigned long long)s.skipped);
    }
}

// the candidate of a polish step from the sums, which it clears for the next step
__global__ void mf_solve_kernel(MfArgs a)
{
    if (blockIdx.x || threadIdx.x) return;
    double S[FIT_NSUMS];
    for (int k = 0; k < FIT_NSUMS; k++) { S[k] = (double)(long long)a.state[MF_S_SUMS + k]; a.state[MF_S_SUMS + k] = 0ull; }
    const long long N = (long long)S[0];
    a.state[MF_S_CAND] = 0ull;
    a.state[MF_S_CAND_OK] = 0ull;
    if (a.state[MF_S_BEST] == 0ull || N < 3) return;
    float (&cand)[9] = *reinterpret_cast<float (*)[9]>(a.state + MF_S_CAND_MODEL);
    if (!fit_affine_from_sums(S, a.w, a.h, reinterpret_cast<float (&)[6]>(cand))) return;
    cand[6] = 0.0f; cand[7] = 0.0f; cand[8] = 1.0f;
    a.state[MF_S_CAND_OK] = 1ull;
}

// the scored inliers of the candidate
__global__ void __launch_bounds__(FIT_THREADS) mf_count_kernel(MfArgs a)
{
    int cnt = 0;
    if (a.state[MF_S_CAND_OK]) {
        float m[9];
        mf_load_model(reinterpret_cast<const float *>(a.state + MF_S_CAND_MODEL), m);
        for (uint32_t c = blockIdx.x * FIT_THREADS + threadIdx.x; c < a.ns; c += gridDim.x * FIT_THREADS) {
            int x, y;
            const uint32_t i = mf_grid_pixel(a, c, x, y);
            float U, V;
            if (!mf_part(a, i, U, V)) continue;
            const float xf = (float)x, yf = (float)y;
            cnt += mf_inlier(m, xf, yf, xf + U, yf + V, a.thresh) ? 1 : 0;
        }
    }
    cnt = block_reduce<FIT_THREADS / 64>(cnt, [](int &x, const int &y) { x += y; });
    if (threadIdx.x == 0 && cnt) atomicAdd(&a.state[MF_S_CAND], (unsigned long long)cnt);
}

__global__ void mf_accept_kernel(MfArgs a)
{
    if (blockIdx.x || threadIdx.x) return;
    if (!a.state[MF_S_CAND_OK] || a.state[MF_S_CAND] < a.state[MF_S_CUR]) return;
    const float *cand = reinterpret_cast<const float *>(a.state + MF_S_CAND_MODEL);
    for (int k = 0; k < 9; k++) a.cur[k] = cand[k];
    a.state[MF_S_CUR] = a.state[MF_S_CAND];
    a.state[MF_S_ACCEPTED] += 1ull;
}

__global__ void __launch_bounds__(FIT_THREADS) mf_apply_kernel(MfArgs a, uint8_t *__restrict__ cls, float *__restrict__ model_flow,
                                                              float *__restrict__ residual)
{
    const uint32_t i = blockIdx.x * FIT_THREADS + threadIdx.x;
    bool scored = false, scored_in = false;
    if (i < a.n) {
        float m[9];
        mf_load_model(a.cur, m);
        const int y = (int)(i / (uint32_t)a.w), x = (int)(i % (uint32_t)a.w);
        const float xf = (float)x, yf = (float)y;
        float U = 0.0f, V = 0.0f;
        const bool good = flow_good(a.flow, a.layout, (size_t)i, U, V);
        const bool excluded = a.exclude && a.exclude[i];
        const bool in = good && mf_inlier(m, xf, yf, xf + U, yf + V, a.thresh);
        const float X = (m[0] * xf + m[1] * yf) + m[2], Y = (m[3] * xf + m[4] * yf) + m[5], W = (m[6] * xf + m[7] * yf) + m[8];
        FlowOut mf = {0.0f, 0.0f, 0.0f}, res = {0.0f, 0.0f, 0.0f};
        if (W > 0.0f) {
            mf.u = X / W - xf; mf.v = Y / W - yf; mf.valid = 1.0f;
            if (good) { res.u = U - mf.u; res.v = V - mf.v; res.valid = 1.0f; }
        }
        if (cls) cls[i] = fit_class(good, excluded, in);
        if (model_flow) reinterpret_cast<FlowOut *>(model_flow)[i] = mf;
        if (residual) reinterpret_cast<FlowOut *>(residual)[i] = res;
        scored = fit_scored(a, good, excluded, x, y);
        scored_in = scored && in;
    }
    fit_block_add({wave_count(scored)}, &a.state[MF_S_SCORED]);
    fit_block_add({wave_count(scored_in)}, &a.state[MF_S_FINAL]);
}

__global__ void mf_finish_kernel(MfArgs a, int32_t *__restrict__ counts)
{
    if (blockIdx.x || threadIdx.x || !counts) return;
    fit_counts(a, counts, MF_S_SCORED, MF_S_FINAL, MF_S_DEGEN);
    counts[6] = (int32_t)a.state[MF_S_ACCEPTED];
    counts[7] = (int32_t)a.state[MF_S_SKIPPED];
}

int launch_motion_fit(int H, int W, const float *flow, int layout, const uint8_t *exclude, int model, float thresh, int n_hyp,
                      int lo_rounds, int polish, int step, uint64_t seed, float *d_model, float *models, int32_t *hyp_counts,
                      int64_t *state, uint8_t *cls, float *model_flow, float *residual, int32_t *counts, hipStream_t s)
{
    MfArgs a = fit_frame(H, W, layout, step, flow, state);
    a.model = model; a.n_hyp = n_hyp; a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.thresh = thresh;
    a.exclude = exclude; a.cur = d_model; a.models = models; a.hyp_counts = hyp_counts;
    if (int rc = fit_clear(state, counts, s)) return rc;
    const unsigned hyp_blocks = (unsigned)((n_hyp + FIT_THREADS - 1) / FIT_THREADS);
    const unsigned chunks = (a.ns + FIT_CHUNK - 1) / FIT_CHUNK;
    const unsigned grid_blocks = (a.ns + FIT_THREADS - 1) / FIT_THREADS;
    const unsigned walk_blocks = grid_blocks < PLANE_MAX_BLOCKS ? grid_blocks : PLANE_MAX_BLOCKS;
    // identity until a round has a winner: round 0 does not look at it, the rounds after it sample its inliers
    hipLaunchKernelGGL(mf_select_kernel, dim3(1), dim3(64), 0, s, a, -1);
    for (int r = 0; r <= lo_rounds; r++) {
        hipLaunchKernelGGL(mf_hyp_kernel, dim3(hyp_blocks), dim3(FIT_THREADS), 0, s, a, r);
        if (model == DFLOW_MOTION_HOMOGRAPHY) hipLaunchKernelGGL(mf_score_kernel<true>, dim3(chunks, hyp_blocks), dim3(FIT_THREADS), 0, s, a);
        else hipLaunchKernelGGL(mf_score_kernel<false>, dim3(chunks, hyp_blocks), dim3(FIT_THREADS), 0, s, a);
        hipLaunchKernelGGL(mf_best_kernel, dim3(hyp_blocks), dim3(FIT_THREADS), 0, s, a, r);
        hipLaunchKernelGGL(mf_select_kernel, dim3(1), dim3(64), 0, s, a, r);
    }
    for (int t = 0; t < (model == DFLOW_MOTION_AFFINE ? polish : 0); t++) {
        hipLaunchKernelGGL(mf_sums_kernel, dim3(walk_blocks), dim3(FIT_THREADS), 0, s, a);
        hipLaunchKernelGGL(mf_solve_kernel, dim3(1), dim3(64), 0, s, a);
        hipLaunchKernelGGL(mf_count_kernel, dim3(walk_blocks), dim3(FIT_THREADS), 0, s, a);
        hipLaunchKernelGGL(mf_accept_kernel, dim3(1), dim3(64), 0, s, a);
    }
    hipLaunchKernelGGL(mf_apply_kernel, dim3((a.n + FIT_THREADS - 1) / FIT_THREADS), dim3(FIT_THREADS), 0, s, a, cls, model_flow, residual);
    hipLaunchKernelGGL(mf_finish_kernel, dim3(1), dim3(64), 0, s, a, counts);
    return dflow_check_launch("motion fit kernels");
}
