// Two-view reconstruction from a flow field and its fundamental matrix (include/dflow.h: dflow_two_view; DESIGN.md "Two-view
// reconstruction"): the essential matrix of F^ under the camera's intrinsics, its four (R, t) candidates, the candidate most
// pixels lie in front of both cameras of, and that pose's depth, class and reprojection error per pixel.  This build's
// definition; the reference has no counterpart.  Every chain is float64, one IEEE operation per written operation.
//
//   tv_decompose_kernel  one lane: E = A^T F^ A, TV_SWEEPS cyclic Jacobi sweeps of E^T E with constant indices (registers, no
//                        private memory), the sorted eigenvectors, U by Gram-Schmidt on E v, R_a, R_b, t and the singular
//                        ratios into d_state[8..31]
//   tv_vote_kernel       the hot one.  TV_PER_LANE grid pixels per lane, a block's pixels contiguous: x1 and x2 once, r, c = r x
//                        x2, d, n1 and n2 for R_a and for R_b; the candidates with -t are the same numbers negated (IEEE
//                        rounding is symmetric), so the four are scored from two evaluations.  Votes are ballots, summed by
//                        the wave over its pixels -> LDS -> one 64-bit integer atomic per block and candidate (fit_common.h's
//                        fit_block_add, for five counts at once and a block of 2048 pixels: the atomics of all blocks land
//                        on the same five words, about 12 ns each on an MI355X, and at one block per 256 pixels they were
//                        the whole kernel's time)
//   tv_apply_kernel      every pixel, as many per lane: the winner is read from the four votes by every lane (ties to the
//                        smaller index), lane 0 of block 0 writes d_pose; depth, class, error, and the three class totals
//   tv_finish_kernel     one lane: d_counts is written from d_state
// 4 launches and one or two memsets whatever the planes hold.  Every count is an integer (exact in any order of arrival).
// fit_common.h holds the frame and the grid of scored pixels, the nine coefficients and the block's counts as the fits use them.
#include "fit_common.h"
#include "wave_ops.h"

#define TV_THREADS 256
#define TV_PER_LANE 8                                 // pixels a lane takes: a block covers 2048 contiguous ones
#define TV_SWEEPS 8
#define TV_SIGMA2_MIN 9.5367431640625e-07             // 2^-20: sigma2 must exceed this times sigma1
// d_state: int64[32].  [0..3] votes, [4] voters, [5..7] pixels of class 1, 2, 3, [8..30] float64 bits: R_a, R_b, t, sigma2/sigma1,
// sigma3/sigma1, [31] 1 when the decomposition gave candidates
enum { TV_S_VOTE = 0, TV_S_VOTERS = 4, TV_S_CLASS = 5, TV_S_RA = 8, TV_S_RB = 17, TV_S_T = 26, TV_S_SIGMA = 29, TV_S_VALID = 31 };

struct TvArgs {
    MfArgs f;                                         // the frame, the grid of voters, the field; cx, cy, s: the header's centre and scale
    const uint8_t *part;
    const float *model;
    double fx, fy, px, py;                            // the camera: focal lengths and principal point, pixels
    double *pose;
    long long *istate;                                // d_state read as integers, f.state for the atomics
    double *dstate;                                   // d_state read as float64
};

__device__ __forceinline__ static bool tv_pos_finite(double d) { return d > 0.0 && d < (double)INFINITY; }

__device__ __forceinline__ static double tv_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ static void tv_mat_vec(const double (&E)[3][3], const double (&v)[3], double (&out)[3])
{
#pragma unroll
    for (int i = 0; i < 3; i++) out[i] = (E[i][0] * v[0] + E[i][1] * v[1]) + E[i][2] * v[2];
}

// JACOBI ROTATION of the pair (P, Q): constant indices, so that M and V stay in registers
template <int P, int Q> __device__ __forceinline__ static void tv_rotate(double (&M)[3][3], double (&V)[3][3])
{
    constexpr int R = 3 - P - Q;
    const double apq = M[P][Q];
    if (apq == 0.0) return;
    const double theta = (M[Q][Q] - M[P][P]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));      // a quotient that overflowed: t = 0, the identity
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
    M[P][P] = M[P][P] - t * apq; M[Q][Q] = M[Q][Q] + t * apq;
    M[P][Q] = 0.0; M[Q][P] = 0.0;
    const double arp = M[R][P], arq = M[R][Q];
    M[R][P] = c * arp - sn * arq; M[P][R] = M[R][P];
    M[R][Q] = sn * arp + c * arq; M[Q][R] = M[R][Q];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - sn * vkq; V[k][Q] = sn * vkp + c * vkq;
    }
}

// eigenpair i <-> eigenpair j
__device__ __forceinline__ static void tv_swap(double (&lam)[3], double (&v)[3][3], int i, int j)
{
    double t = lam[i]; lam[i] = lam[j]; lam[j] = t;
#pragma unroll
    for (int k = 0; k < 3; k++) { t = v[i][k]; v[i][k] = v[j][k]; v[j][k] = t; }
}

// A and B (include/dflow.h)
__global__ void tv_decompose_kernel(TvArgs a)
{
    if (blockIdx.x || threadIdx.x) return;
    double *out = a.dstate + TV_S_RA;
    float m[9];
    mf_load_model(a.model, m);
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; k++) any |= !(m[k] == 0.0f);
    bool valid = any;
    double Ra[9], Rb[9], tt[3], sg[2];
#pragma unroll
    for (int k = 0; k < 9; k++) Ra[k] = Rb[k] = 0.0;
    tt[0] = tt[1] = tt[2] = sg[0] = sg[1] = 0.0;
    if (valid) {
        const double a00 = a.f.s * a.fx, a02 = a.f.s * (a.px - a.f.cx), a11 = a.f.s * a.fy, a12 = a.f.s * (a.py - a.f.cy);
        double G[3][3], E[3][3], M[3][3], V[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double f0 = (double)m[3 * i], f1 = (double)m[3 * i + 1], f2 = (double)m[3 * i + 2];
            G[i][0] = f0 * a00; G[i][1] = f1 * a11; G[i][2] = (f0 * a02 + f1 * a12) + f2;
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            E[0][j] = a00 * G[0][j]; E[1][j] = a11 * G[1][j]; E[2][j] = (a02 * G[0][j] + a12 * G[1][j]) + G[2][j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++) {
                M[i][j] = (E[0][i] * E[0][j] + E[1][i] * E[1][j]) + E[2][i] * E[2][j];
                M[j][i] = M[i][j];
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
        for (int sweep = 0; sweep < TV_SWEEPS; sweep++) {
            tv_rotate<0, 1>(M, V);
            tv_rotate<0, 2>(M, V);
            tv_rotate<1, 2>(M, V);
        }
        // descending eigenvalues, ties to the smaller index: an insertion sort written out
        double lam[3] = {M[0][0], M[1][1], M[2][2]}, v[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) v[i][k] = V[k][i];
        if (lam[1] > lam[0]) tv_swap(lam, v, 0, 1);
        if (lam[2] > lam[1]) {
            tv_swap(lam, v, 1, 2);
            if (lam[1] > lam[0]) tv_swap(lam, v, 0, 1);
        }
        const double det = (v[0][0] * (v[1][1] * v[2][2] - v[2][1] * v[1][2]) - v[1][0] * (v[0][1] * v[2][2] - v[2][1] * v[0][2]))
                           + v[2][0] * (v[0][1] * v[1][2] - v[1][1] * v[0][2]);
        if (det < 0.0) { v[2][0] = -v[2][0]; v[2][1] = -v[2][1]; v[2][2] = -v[2][2]; }
        double w1[3], w2[3], w3[3], u1[3], u2[3], u3[3];
        tv_mat_vec(E, v[0], w1);
        const double s1 = sqrt(tv_dot(w1, w1));
        valid = isfinite(s1) && s1 > 0.0;
        if (valid) {
#pragma unroll
            for (int i = 0; i < 3; i++) u1[i] = w1[i] / s1;
            tv_mat_vec(E, v[1], w2);
            const double g = tv_dot(w2, u1);
#pragma unroll
            for (int i = 0; i < 3; i++) w2[i] = w2[i] - g * u1[i];
            const double s2 = sqrt(tv_dot(w2, w2));
            valid = s2 > TV_SIGMA2_MIN * s1;
            if (valid) {
#pragma unroll
                for (int i = 0; i < 3; i++) u2[i] = w2[i] / s2;
                u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
                tv_mat_vec(E, v[2], w3);
                const double s3 = sqrt(tv_dot(w3, w3));
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        Ra[3 * i + j] = (u2[i] * v[0][j] - u1[i] * v[1][j]) + u3[i] * v[2][j];
                        Rb[3 * i + j] = (u1[i] * v[1][j] - u2[i] * v[0][j]) + u3[i] * v[2][j];
                    }
                tt[0] = u3[0]; tt[1] = u3[1]; tt[2] = u3[2];
                sg[0] = s2 / s1; sg[1] = s3 / s1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) { out[k] = valid ? Ra[k] : 0.0; out[9 + k] = valid ? Rb[k] : 0.0; }
#pragma unroll
    for (int k = 0; k < 3; k++) out[18 + k] = valid ? tt[k] : 0.0;
    out[21] = valid ? sg[0] : 0.0; out[22] = valid ? sg[1] : 0.0;
    a.istate[TV_S_VALID] = valid ? 1 : 0;
}

struct TvPixel { double x1, y1, x2, y2; };

// x1 and x2 of the pixel (x, y) with the good vector (U, V)
__device__ __forceinline__ static void tv_pixel(const TvArgs &a, int x, int y, float U, float V, TvPixel &p, float &tx, float &ty)
{
    const float xf = (float)x, yf = (float)y;
    tx = xf + U; ty = yf + V;
    p.x1 = ((double)xf - a.px) / a.fx; p.y1 = ((double)yf - a.py) / a.fy;
    p.x2 = ((double)tx - a.px) / a.fx; p.y2 = ((double)ty - a.py) / a.fy;
}

// C. r = R x1, c = r x x2, d = c.c, n1 = (x2 x t).c, n2 = (r x t).c
__device__ __forceinline__ static void tv_geometry(const double (&R)[9], const double (&t)[3], const TvPixel &p, double (&r)[3], double &d,
                                                   double &n1, double &n2)
{
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = (R[3 * i] * p.x1 + R[3 * i + 1] * p.y1) + R[3 * i + 2];
    const double c0 = r[1] - r[2] * p.y2, c1 = r[2] * p.x2 - r[0], c2 = r[0] * p.y2 - r[1] * p.x2;
    d = (c0 * c0 + c1 * c1) + c2 * c2;
    const double a0 = p.y2 * t[2] - t[1], a1 = t[0] - p.x2 * t[2], a2 = p.x2 * t[1] - p.y2 * t[0];
    n1 = (a0 * c0 + a1 * c1) + a2 * c2;
    const double b0 = r[1] * t[2] - r[2] * t[1], b1 = r[2] * t[0] - r[0] * t[2], b2 = r[0] * t[1] - r[1] * t[0];
    n2 = (b0 * c0 + b1 * c1) + b2 * c2;
}

// whether grid point c votes at all, and its vector
__device__ __forceinline__ static bool tv_voter(const TvArgs &a, uint32_t c, float &U, float &V)
{
    U = V = 0.0f;
    if (c >= a.f.ns) return false;
    int x, y;
    const uint32_t i = mf_grid_pixel(a.f, c, x, y);
    return flow_good(a.f.flow, a.f.layout, (size_t)i, U, V) && !(a.part && a.part[i] != 1);
}

// C. the votes of the voter at grid point c
__device__ __forceinline__ static void tv_vote_pixel(const TvArgs &a, uint32_t c, float U, float V, bool (&vote)[4])
{
    int x, y;
    mf_grid_pixel(a.f, c, x, y);
    TvPixel p;
    float tx, ty;
    tv_pixel(a, x, y, U, V, p, tx, ty);
    double t[3], R[9], r[3], d, n1, n2;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = a.dstate[TV_S_T + k];
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = a.dstate[(q ? TV_S_RB : TV_S_RA) + k];
        tv_geometry(R, t, p, r, d, n1, n2);
        const bool ok = tv_pos_finite(d);
        vote[2 * q] = ok && n1 > 0.0 && n2 > 0.0;
        vote[2 * q + 1] = ok && n1 < 0.0 && n2 < 0.0;                 // (R, -t): n1 and n2 negated exactly
    }
}

__global__ void __launch_bounds__(TV_THREADS) tv_vote_kernel(TvArgs a)
{
    static_assert(TV_S_VOTERS == TV_S_VOTE + 4, "fit_block_add: the four votes and the voters are neighbours in d_state");
    const bool valid = a.istate[TV_S_VALID] != 0;
    const uint32_t c0 = blockIdx.x * (TV_PER_LANE * TV_THREADS) + threadIdx.x;
    int total[5] = {0, 0, 0, 0, 0};
    float U[TV_PER_LANE], V[TV_PER_LANE];
    bool cover[TV_PER_LANE];
#pragma unroll
    for (int it = 0; it < TV_PER_LANE; it++) cover[it] = tv_voter(a, c0 + it * TV_THREADS, U[it], V[it]);    // every load in flight
#pragma unroll
    for (int it = 0; it < TV_PER_LANE; it++) total[4] += wave_count(cover[it]);
    if (valid) {
#pragma unroll 1
        for (int it = 0; it < TV_PER_LANE; it++) {
            bool vote[4] = {false, false, false, false};
            if (cover[it]) tv_vote_pixel(a, c0 + it * TV_THREADS, U[it], V[it], vote);
#pragma unroll
            for (int k = 0; k < 4; k++) total[k] += wave_count(vote[k]);
        }
    }
    fit_block_add(total, &a.f.state[TV_S_VOTE]);
}

// D. the candidate with the most votes, ties to the smaller index; -1: none
__device__ __forceinline__ static int tv_winner(const TvArgs &a)
{
    int best = -1;
    long long most = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long v = a.istate[TV_S_VOTE + k];
        if (v > most) { most = v; best = k; }
    }
    return best;
}

// E. pixel i < n with its vector under the winner (R, t), best < 0: none -> its class
__device__ __forceinline__ static int tv_apply_pixel(const TvArgs &a, uint32_t i, bool good, float U, float V, int best, const double (&R)[9],
                                                     const double (&t)[3], float *__restrict__ depth, uint8_t *__restrict__ cls,
                                                     float *__restrict__ err)
{
    const int y = (int)(i / (uint32_t)a.f.w), x = (int)(i % (uint32_t)a.f.w);
    float z = 0.0f, e = -1.0f;
    int k = 0;
    if (good) {
        k = 3; e = INFINITY;
        if (best >= 0) {
            TvPixel p;
            float tx, ty;
            tv_pixel(a, x, y, U, V, p, tx, ty);
            double r[3], d, n1, n2;
            tv_geometry(R, t, p, r, d, n1, n2);
            if (tv_pos_finite(d)) {
                const double Z = n1 / d;
                z = (float)Z;
                k = n1 > 0.0 && n2 > 0.0 ? 1 : 2;
                const double Y0 = Z * r[0] + t[0], Y1 = Z * r[1] + t[1], Y2 = Z * r[2] + t[2];
                if (Y2 > 0.0) {
                    const double ex = ((a.fx * Y0) / Y2 + a.px) - (double)tx, ey = ((a.fy * Y1) / Y2 + a.py) - (double)ty;
                    e = (float)sqrt(ex * ex + ey * ey);
                }
            }
        }
    }
    if (depth) depth[i] = z;
    if (cls) cls[i] = (uint8_t)k;
    if (err) err[i] = e;
    return k;
}

__global__ void __launch_bounds__(TV_THREADS) tv_apply_kernel(TvArgs a, float *__restrict__ depth, uint8_t *__restrict__ cls,
                                                              float *__restrict__ err)
{
    const int best = tv_winner(a);
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = best < 0 ? 0.0 : a.dstate[((best & 2) ? TV_S_RB : TV_S_RA) + k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double tk = a.dstate[TV_S_T + k];
        t[k] = best < 0 ? 0.0 : (best & 1) ? -tk : tk;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.pose[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) a.pose[9 + k] = t[k];
        a.pose[12] = best < 0 ? 0.0 : 1.0;
        a.pose[13] = best < 0 ? 0.0 : a.dstate[TV_S_SIGMA];
        a.pose[14] = best < 0 ? 0.0 : a.dstate[TV_S_SIGMA + 1];
        a.pose[15] = (double)best;
    }
    const uint32_t i0 = blockIdx.x * (TV_PER_LANE * TV_THREADS) + threadIdx.x;
    int total[3] = {0, 0, 0};
    float U[TV_PER_LANE], V[TV_PER_LANE];
    bool good[TV_PER_LANE];
#pragma unroll
    for (int it = 0; it < TV_PER_LANE; it++) {                                                                   // every load in flight
        const uint32_t i = i0 + it * TV_THREADS;
        U[it] = V[it] = 0.0f;
        good[it] = i < a.f.n && flow_good(a.f.flow, a.f.layout, (size_t)i, U[it], V[it]);
    }
#pragma unroll 1
    for (int it = 0; it < TV_PER_LANE; it++) {
        const uint32_t i = i0 + it * TV_THREADS;
        const int k = i < a.f.n ? tv_apply_pixel(a, i, good[it], U[it], V[it], best, R, t, depth, cls, err) : 0;
#pragma unroll
        for (int q = 1; q <= 3; q++) total[q - 1] += wave_count(k == q);
    }
    fit_block_add(total, &a.f.state[TV_S_CLASS]);
}

__global__ void tv_finish_kernel(TvArgs a, int32_t *__restrict__ counts)
{
    if (blockIdx.x || threadIdx.x || !counts) return;
    const int best = tv_winner(a);
    long long second = 0;
    for (int k = 0; k < 4; k++) {
        const long long v = a.istate[TV_S_VOTE + k];
        if (k != best && v > second) second = v;
    }
    counts[0] = (int32_t)a.istate[TV_S_VOTERS];
    counts[1] = best < 0 ? 0 : (int32_t)a.istate[TV_S_VOTE + best];
    counts[2] = best < 0 ? 0 : (int32_t)second;
    counts[3] = best;
    counts[4] = (int32_t)a.istate[TV_S_CLASS];
    counts[5] = (int32_t)a.istate[TV_S_CLASS + 1];
    counts[6] = (int32_t)a.istate[TV_S_CLASS + 2];
    counts[7] = 0;
}

int launch_two_view(int H, int W, const float *flow, int layout, const float *model, const uint8_t *part, double fx, double fy, double cx,
                    double cy, int step, double *pose, int64_t *state, float *depth, uint8_t *cls, float *err, int32_t *counts,
                    hipStream_t s)
{
    TvArgs a;
    a.f = fit_frame(H, W, layout, step, flow, state);             // no samples: nothing else of it is read
    a.part = part; a.model = model; a.fx = fx; a.fy = fy; a.px = cx; a.py = cy; a.pose = pose;
    a.istate = reinterpret_cast<long long *>(state); a.dstate = reinterpret_cast<double *>(state);
    if (int rc = fit_clear(state, counts, s)) return rc;
    hipLaunchKernelGGL(tv_decompose_kernel, dim3(1), dim3(64), 0, s, a);
    const uint32_t per_block = TV_THREADS * TV_PER_LANE;
    hipLaunchKernelGGL(tv_vote_kernel, dim3((a.f.ns + per_block - 1) / per_block), dim3(TV_THREADS), 0, s, a);
    hipLaunchKernelGGL(tv_apply_kernel, dim3((a.f.n + per_block - 1) / per_block), dim3(TV_THREADS), 0, s, a, depth, cls, err);
    hipLaunchKernelGGL(tv_finish_kernel, dim3(1), dim3(64), 0, s, a, counts);
    return dflow_check_launch("two-view kernels");
}
