// Variational refinement of a dense flow field (dflow_var_refine; DESIGN.md "Variational refinement"): one-level energy
// minimisation after Brox et al. 2004 and EpicFlow section 4, this build's own definition.  Preparation (Gaussian smoothing,
// the local smoothness weight), per outer iteration warp + derivatives, per inner iteration the lagged coefficients, then
// red-black SOR.  All arithmetic float32, one IEEE operation per written operation in a fixed order (-ffp-contract=off), so
// that two calls, and the fused and the unfused solver, agree bit for bit.  Nothing here synchronises or reads back.
#include <math.h>
#include "dflow_common.h"

#define VAR_EPS2 1e-6f
#define VAR_ZETA2 0.01f
#define VAR_BX 32
#define VAR_BY 8
#define VAR_THREADS (VAR_BX * VAR_BY)

// every plane is H*W float32
struct VarWs {
    float *I1[3], *I2[3], *omega, *u, *v, *Ibar[3], *Iz[3], *mask, *Ix[3], *Iy[3];
    float *Ixx[3], *Ixy[3], *Iyy[3], *Ixz[3], *Iyz[3], *p, *a11, *a12, *a22, *b1, *b2, *sx, *sy, *d[2][2];
    size_t bytes;
};

static VarWs var_ws(void *ws, int H, int W)
{
    WsCarver c(ws);
    const size_t n = (size_t)H * W;
    VarWs w;
    for (float **planes : {w.I1, w.I2, w.Ibar, w.Iz, w.Ix, w.Iy, w.Ixx, w.Ixy, w.Iyy, w.Ixz, w.Iyz})
        for (int k = 0; k < 3; k++) planes[k] = c.take<float>(n);
    for (float **plane : {&w.omega, &w.u, &w.v, &w.mask, &w.p, &w.a11, &w.a12, &w.a22, &w.b1, &w.b2, &w.sx, &w.sy,
                          &w.d[0][0], &w.d[0][1], &w.d[1][0], &w.d[1][1]})
        *plane = c.take<float>(n);
    w.bytes = c.bytes;
    return w;
}

size_t var_ws_bytes(int H, int W) { return var_ws(nullptr, H, W).bytes; }

// ---- preparation ----------------------------------------------------------------------------------------------------
// Separable Gaussian of one (H,W,3) uint8 image into three float planes: both passes in one launch.  A 32x32 tile with a
// halo of r pixels is staged in LDS (a halo cell holds the pixel at the clamped coordinate, so the row pass of a halo row is
// the row pass of the clamped row), filtered along x into a second LDS array, then along y.
#define VAR_ST 32
__global__ __launch_bounds__(VAR_THREADS) void var_smooth_kernel(const uint8_t *__restrict__ bgr, int H, int W, VarTaps taps,
                                                                  float *o0, float *o1, float *o2)
{
    constexpr int S = VAR_ST + 2 * VAR_MAX_RADIUS;
    __shared__ float in[S][S + 1];
    __shared__ float mid[S][VAR_ST + 1];
    const int r = taps.r, n = VAR_ST + 2 * r;
    const int x0 = blockIdx.x * VAR_ST, y0 = blockIdx.y * VAR_ST;
    float *const out[3] = {o0, o1, o2};
    for (int c = 0; c < 3; c++) {
        for (int i = threadIdx.x; i < n * n; i += VAR_THREADS) {
            const int ly = i / n, lx = i - ly * n;
            const int gy = clampi(y0 + ly - r, 0, H - 1), gx = clampi(x0 + lx - r, 0, W - 1);
            in[ly][lx] = (float)bgr[((size_t)gy * W + gx) * 3 + c];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n * VAR_ST; i += VAR_THREADS) {
            const int ly = i / VAR_ST, lx = i - ly * VAR_ST;
            float acc = 0.0f;
            for (int k = 0; k <= 2 * r; k++) acc = acc + taps.t[k] * in[ly][lx + k];
            mid[ly][lx] = acc;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < VAR_ST * VAR_ST; i += VAR_THREADS) {
            const int ly = i / VAR_ST, lx = i - ly * VAR_ST;
            float acc = 0.0f;
            for (int k = 0; k <= 2 * r; k++) acc = acc + taps.t[k] * mid[ly + k][lx];
            if (y0 + ly < H && x0 + lx < W) out[c][(size_t)(y0 + ly) * W + x0 + lx] = acc;
        }
        __syncthreads();
    }
}

// the 5-tap derivative (1, -8, 0, 8, -1) / 12 along x or y at (y, x), replicate border
template <typename F> __device__ __forceinline__ static float deriv5(F &&at)
{
    return (((at(-2) - 8.0f * at(-1)) + 8.0f * at(1)) - at(2)) / 12.0f;
}
__device__ __forceinline__ static float ddx(const float *__restrict__ f, int H, int W, int y, int x)
{
    const float *row = f + (size_t)y * W;
    return deriv5([&](int k) { return row[clampi(x + k, 0, W - 1)]; });
}
__device__ __forceinline__ static float ddy(const float *__restrict__ f, int H, int W, int y, int x)
{
    return deriv5([&](int k) { return f[(size_t)clampi(y + k, 0, H - 1) * W + x]; });
}

#define VAR_PIXEL() \
    const int x = blockIdx.x * VAR_BX + threadIdx.x, y = blockIdx.y * VAR_BY + threadIdx.y; \
    if (x >= W || y >= H) return; \
    const size_t i = (size_t)y * W + x

// omega = exp(-5 |grad L| / 255), L the luma of the smoothed first image
__global__ __launch_bounds__(VAR_THREADS) void var_omega_kernel(int H, int W, VarWs w)
{
    VAR_PIXEL();
    auto L = [&](int yy, int xx) {
        const size_t j = (size_t)yy * W + xx;
        return (0.114f * w.I1[0][j] + 0.587f * w.I1[1][j]) + 0.299f * w.I1[2][j];
    };
    const float lx = deriv5([&](int k) { return L(y, clampi(x + k, 0, W - 1)); });
    const float ly = deriv5([&](int k) { return L(clampi(y + k, 0, H - 1), x); });
    w.omega[i] = expf(-5.0f * sqrtf(lx * lx + ly * ly) / 255.0f);
}

__global__ __launch_bounds__(VAR_THREADS) void var_split_kernel(int H, int W, const float *__restrict__ flow, VarWs w)
{
    VAR_PIXEL();
    const float2 f = reinterpret_cast<const float2 *>(flow)[i];
    w.v[i] = f.x;
    w.u[i] = f.y;
}

__global__ __launch_bounds__(VAR_THREADS) void var_join_kernel(int H, int W, VarWs w, float *__restrict__ flow)
{
    VAR_PIXEL();
    reinterpret_cast<float2 *>(flow)[i] = make_float2(w.v[i], w.u[i]);
}

// ---- outer iteration ------------------------------------------------------------------------------------------------
// warp + mean image + temporal difference: I2w is never stored
__global__ __launch_bounds__(VAR_THREADS) void var_warp_kernel(int H, int W, VarWs w)
{
    VAR_PIXEL();
    const float u = w.u[i], v = w.v[i];
    const bool fin = isfinite(u) && isfinite(v);
    float xs = fin ? (float)x + u : (float)x, ys = fin ? (float)y + v : (float)y;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const bool inside = fin && xs >= 0.0f && xs <= xmax && ys >= 0.0f && ys <= ymax;
    xs = fminf(fmaxf(xs, 0.0f), xmax);
    ys = fminf(fmaxf(ys, 0.0f), ymax);
    const float xf = floorf(xs), yf = floorf(ys);
    const float fx = xs - xf, fy = ys - yf;
    const int xa = (int)xf, ya = (int)yf, xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);
    for (int c = 0; c < 3; c++) {
        const float *I2 = w.I2[c];
        const float top = (1.0f - fx) * I2[(size_t)ya * W + xa] + fx * I2[(size_t)ya * W + xb];
        const float bot = (1.0f - fx) * I2[(size_t)yb * W + xa] + fx * I2[(size_t)yb * W + xb];
        const float warped = (1.0f - fy) * top + fy * bot;
        const float i1 = w.I1[c][i];
        w.Ibar[c][i] = 0.5f * (i1 + warped);
        w.Iz[c][i] = warped - i1;
    }
    w.mask[i] = inside ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(VAR_THREADS) void var_deriv1_kernel(int H, int W, VarWs w)
{
    VAR_PIXEL();
    for (int c = 0; c < 3; c++) {
        w.Ix[c][i] = ddx(w.Ibar[c], H, W, y, x);
        w.Iy[c][i] = ddy(w.Ibar[c], H, W, y, x);
    }
}

__global__ __launch_bounds__(VAR_THREADS) void var_deriv2_kernel(int H, int W, VarWs w)
{
    VAR_PIXEL();
    for (int c = 0; c < 3; c++) {
        w.Ixx[c][i] = ddx(w.Ix[c], H, W, y, x);
        w.Ixy[c][i] = ddy(w.Ix[c], H, W, y, x);
        w.Iyy[c][i] = ddy(w.Iy[c], H, W, y, x);
        w.Ixz[c][i] = ddx(w.Iz[c], H, W, y, x);
        w.Iyz[c][i] = ddy(w.Iz[c], H, W, y, x);
    }
}

// ---- inner iteration ------------------------------------------------------------------------------------------------
__device__ __forceinline__ static float psi_prime(float s2) { return 1.0f / (2.0f * sqrtf(s2 + VAR_EPS2)); }

// p = omega Psi'(|grad U|^2 + |grad V|^2), U = u + du, V = v + dv, central differences
__global__ __launch_bounds__(VAR_THREADS) void var_smooth_weight_kernel(int H, int W, VarWs w, const float *__restrict__ du,
                                                                         const float *__restrict__ dv)
{
    VAR_PIXEL();
    const size_t l = (size_t)y * W + clampi(x - 1, 0, W - 1), r = (size_t)y * W + clampi(x + 1, 0, W - 1);
    const size_t t = (size_t)clampi(y - 1, 0, H - 1) * W + x, b = (size_t)clampi(y + 1, 0, H - 1) * W + x;
    const float ux = 0.5f * ((w.u[r] + du[r]) - (w.u[l] + du[l])), uy = 0.5f * ((w.u[b] + du[b]) - (w.u[t] + du[t]));
    const float vx = 0.5f * ((w.v[r] + dv[r]) - (w.v[l] + dv[l])), vy = 0.5f * ((w.v[b] + dv[b]) - (w.v[t] + dv[t]));
    w.p[i] = w.omega[i] * psi_prime(((ux * ux + uy * uy) + vx * vx) + vy * vy);
}

// data term at (du, dv), edge weights, divergence of the current flow -> a11 a12 a22 b1 b2 and the weights of the edges
// to the right (sx) and down (sy)
__global__ __launch_bounds__(VAR_THREADS) void var_coef_kernel(int H, int W, VarWs w, const float *__restrict__ du_,
                                                                const float *__restrict__ dv_, float alpha, float gamma,
                                                                float delta)
{
    VAR_PIXEL();
    const float du = du_[i], dv = dv_[i], m = w.mask[i];
    float e[3], s11[3], s12[3], s22[3], t1[3], t2[3];
    for (int c = 0; c < 3; c++) {
        const float Ixx = w.Ixx[c][i], Ixy = w.Ixy[c][i], Iyy = w.Iyy[c][i], Ixz = w.Ixz[c][i], Iyz = w.Iyz[c][i];
        const float nx = 1.0f / ((Ixx * Ixx + Ixy * Ixy) + VAR_ZETA2), ny = 1.0f / ((Ixy * Ixy + Iyy * Iyy) + VAR_ZETA2);
        const float rx = (Ixz + Ixx * du) + Ixy * dv, ry = (Iyz + Ixy * du) + Iyy * dv;
        e[c] = nx * (rx * rx) + ny * (ry * ry);
        s11[c] = nx * (Ixx * Ixx) + ny * (Ixy * Ixy);
        s12[c] = nx * (Ixx * Ixy) + ny * (Ixy * Iyy);
        s22[c] = nx * (Ixy * Ixy) + ny * (Iyy * Iyy);
        t1[c] = nx * (Ixx * Ixz) + ny * (Ixy * Iyz);
        t2[c] = nx * (Ixy * Ixz) + ny * (Iyy * Iyz);
    }
    auto sum3 = [](const float *a) { return (a[0] + a[1]) + a[2]; };
    const float g = (gamma * m) * psi_prime(sum3(e));
    float a11 = g * sum3(s11), a12 = g * sum3(s12), a22 = g * sum3(s22), b1 = -(g * sum3(t1)), b2 = -(g * sum3(t2));
    if (delta > 0.0f) {
        for (int c = 0; c < 3; c++) {
            const float Ix = w.Ix[c][i], Iy = w.Iy[c][i], Iz = w.Iz[c][i];
            const float n = 1.0f / ((Ix * Ix + Iy * Iy) + VAR_ZETA2);
            const float r = (Iz + Ix * du) + Iy * dv;
            e[c] = n * (r * r);
            s11[c] = n * (Ix * Ix);
            s12[c] = n * (Ix * Iy);
            s22[c] = n * (Iy * Iy);
            t1[c] = n * (Ix * Iz);
            t2[c] = n * (Iy * Iz);
        }
        const float k = (delta * m) * psi_prime(sum3(e));
        a11 = a11 + k * sum3(s11); a12 = a12 + k * sum3(s12); a22 = a22 + k * sum3(s22);
        b1 = b1 - k * sum3(t1); b2 = b2 - k * sum3(t2);
    }
    // an edge that leaves the image has weight 0, and the neighbour beyond it reads as 0
    const float p = w.p[i], u = w.u[i], v = w.v[i];
    const bool hl = x > 0, hr = x + 1 < W, hu = y > 0, hd = y + 1 < H;
    const float sl = hl ? alpha * (0.5f * (w.p[i - 1] + p)) : 0.0f, sr = hr ? alpha * (0.5f * (p + w.p[i + 1])) : 0.0f;
    const float su = hu ? alpha * (0.5f * (w.p[i - W] + p)) : 0.0f, sd = hd ? alpha * (0.5f * (p + w.p[i + W])) : 0.0f;
    const float ul = hl ? w.u[i - 1] : 0.0f, ur = hr ? w.u[i + 1] : 0.0f, uu = hu ? w.u[i - W] : 0.0f, ud = hd ? w.u[i + W] : 0.0f;
    const float vl = hl ? w.v[i - 1] : 0.0f, vr = hr ? w.v[i + 1] : 0.0f, vu = hu ? w.v[i - W] : 0.0f, vd = hd ? w.v[i + W] : 0.0f;
    float acc = sl * (ul - u); acc = acc + sr * (ur - u); acc = acc + su * (uu - u); acc = acc + sd * (ud - u);
    b1 = b1 + acc;
    acc = sl * (vl - v); acc = acc + sr * (vr - v); acc = acc + su * (vu - v); acc = acc + sd * (vd - v);
    b2 = b2 + acc;
    w.a11[i] = a11; w.a12[i] = a12; w.a22[i] = a22; w.b1[i] = b1; w.b2[i] = b2; w.sx[i] = sr; w.sy[i] = sd;
}

// ---- red-black SOR --------------------------------------------------------------------------------------------------
// the nine numbers a pixel's update needs besides du, dv: the data term and the weights of its four edges
struct SorCoef { float a11, a12, a22, b1, b2, sl, sr, su, sd; };

__device__ __forceinline__ static SorCoef sor_load(const VarWs &w, int H, int W, int y, int x)
{
    const size_t i = (size_t)y * W + x;
    SorCoef c;
    c.a11 = w.a11[i]; c.a12 = w.a12[i]; c.a22 = w.a22[i]; c.b1 = w.b1[i]; c.b2 = w.b2[i];
    c.sl = x > 0 ? w.sx[i - 1] : 0.0f; c.sr = w.sx[i];        // sx, sy are 0 on the last column / row
    c.su = y > 0 ? w.sy[i - W] : 0.0f; c.sd = w.sy[i];
    return c;
}

// One pixel's SOR step, the single statement of it that both solvers execute.  n*: the neighbours' (du, dv) in the order
// left, right, up, down (0 beyond the image, where the weight is 0 too).  Returns false when det is not > 0.
__device__ __forceinline__ static bool sor_update(const SorCoef &c, float2 nl, float2 nr, float2 nu, float2 nd, float omega,
                                                  float2 &d)
{
    const float ss = ((c.sl + c.sr) + c.su) + c.sd;
    const float A11 = c.a11 + ss, A22 = c.a22 + ss;
    const float det = A11 * A22 - c.a12 * c.a12;
    float acc = c.sl * nl.x; acc = acc + c.sr * nr.x; acc = acc + c.su * nu.x; acc = acc + c.sd * nd.x;
    const float B1 = c.b1 + acc;
    acc = c.sl * nl.y; acc = acc + c.sr * nr.y; acc = acc + c.su * nu.y; acc = acc + c.sd * nd.y;
    const float B2 = c.b2 + acc;
    if (!(det > 0.0f)) return false;
    d.x = (1.0f - omega) * d.x + omega * ((A22 * B1 - c.a12 * B2) / det);
    d.y = (1.0f - omega) * d.y + omega * ((A11 * B2 - c.a12 * B1) / det);
    return true;
}

// unfused: one launch per half-sweep, in place (a pixel of one colour reads only pixels of the other).  One thread per
// horizontal pair of pixels; it takes the one whose (x + y) parity is `colour`.
__global__ __launch_bounds__(VAR_THREADS) void var_sor_half_kernel(int H, int W, VarWs w, float *__restrict__ du,
                                                                    float *__restrict__ dv, float omega, int colour)
{
    const int y = blockIdx.y * VAR_BY + threadIdx.y;
    const int x = 2 * (blockIdx.x * VAR_BX + threadIdx.x) + ((y + colour) & 1);
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * W + x;
    auto at = [&](bool have, size_t j) { return have ? make_float2(du[j], dv[j]) : make_float2(0.0f, 0.0f); };
    float2 d = make_float2(du[i], dv[i]);
    if (sor_update(sor_load(w, H, W, y, x), at(x > 0, i - 1), at(x + 1 < W, i + 1), at(y > 0, i - W), at(y + 1 < H, i + W), omega, d)) {
        du[i] = d.x;
        dv[i] = d.y;
    }
}

// fused: a workgroup holds (du, dv) of a VAR_R x VAR_R region in LDS, each thread the coefficients of its 8 cells in
// registers, and runs up to VAR_T half-sweeps there.  The region's outermost ring is never updated, so it is right before
// the first half-sweep only; a cell at distance d from the ring reads, in half-sweep t <= d, neighbours at distance >= d - 1
// that are right after t - 1 half-sweeps, so it is right after t.  The interior, at distance >= VAR_T, is right after all
// of them and is what the workgroup writes (to the other buffer: its neighbours' halos read this one).  Cells beyond the
// image hold 0 and have no coefficients (det = 0: never updated), exactly what the global sweep reads there.
#define VAR_T 8
#define VAR_R 64
#define VAR_TILE (VAR_R - 2 * VAR_T)
#define VAR_FUSED_THREADS 512
#define VAR_ROWS_PER_THREAD (VAR_R / (VAR_FUSED_THREADS / (VAR_R / 2)))
static_assert(VAR_T % 2 == 0 && VAR_TILE % 2 == 0, "region origins must be even: a thread's colour choice is per row parity");
__global__ __launch_bounds__(VAR_FUSED_THREADS) void var_sor_fused_kernel(int H, int W, VarWs w, const float *__restrict__ du_in,
                                                                           const float *__restrict__ dv_in,
                                                                           float *__restrict__ du_out, float *__restrict__ dv_out,
                                                                           float omega, int first, int count)
{
    __shared__ float2 d[VAR_R][VAR_R];
    constexpr int STEP = VAR_FUSED_THREADS / (VAR_R / 2);       // rows between a thread's pairs
    static_assert(STEP % 2 == 0, "a thread's rows must share their parity");
    const int px = threadIdx.x % (VAR_R / 2), ry = threadIdx.x / (VAR_R / 2);
    const int x0 = blockIdx.x * VAR_TILE - VAR_T, y0 = blockIdx.y * VAR_TILE - VAR_T;
    SorCoef coef[VAR_ROWS_PER_THREAD][2];
#pragma unroll
    for (int k = 0; k < VAR_ROWS_PER_THREAD; k++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int lx = 2 * px + j, ly = ry + STEP * k, gx = x0 + lx, gy = y0 + ly;
            const bool in_image = gx >= 0 && gx < W && gy >= 0 && gy < H;
            const bool ring = lx == 0 || lx == VAR_R - 1 || ly == 0 || ly == VAR_R - 1;
            coef[k][j] = SorCoef{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (in_image && !ring) coef[k][j] = sor_load(w, H, W, gy, gx);
            d[ly][lx] = in_image ? make_float2(du_in[(size_t)gy * W + gx], dv_in[(size_t)gy * W + gx]) : make_float2(0.0f, 0.0f);
        }
    __syncthreads();
    for (int t = 0; t < count; t++) {
        const int j = (ry + first + t) & 1;                     // x0, y0 and STEP are even: (gx + gy) parity = (lx + ry) parity
        const int lx = 2 * px + j, lxl = max(lx - 1, 0), lxr = min(lx + 1, VAR_R - 1);
#pragma unroll
        for (int k = 0; k < VAR_ROWS_PER_THREAD; k++) {
            const int ly = ry + STEP * k;
            const SorCoef c = j ? coef[k][1] : coef[k][0];
            float2 v = d[ly][lx];
            if (sor_update(c, d[ly][lxl], d[ly][lxr], d[max(ly - 1, 0)][lx], d[min(ly + 1, VAR_R - 1)][lx], omega, v)) d[ly][lx] = v;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < VAR_ROWS_PER_THREAD; k++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int lx = 2 * px + j, ly = ry + STEP * k, gx = x0 + lx, gy = y0 + ly;
            if (lx >= VAR_T && lx < VAR_T + VAR_TILE && ly >= VAR_T && ly < VAR_T + VAR_TILE && gx < W && gy < H) {
                du_out[(size_t)gy * W + gx] = d[ly][lx].x;
                dv_out[(size_t)gy * W + gx] = d[ly][lx].y;
            }
        }
}

__global__ __launch_bounds__(VAR_THREADS) void var_add_kernel(int H, int W, VarWs w, const float *__restrict__ du,
                                                               const float *__restrict__ dv)
{
    VAR_PIXEL();
    w.u[i] = w.u[i] + du[i];
    w.v[i] = w.v[i] + dv[i];
}

VarTaps var_taps(float sigma)
{
    VarTaps t = {};
    if (sigma == 0.0f) { t.t[0] = 1.0f; return t; }
    const double s = (double)sigma;
    t.r = (int)ceil(3.0 * s);
    double e[2 * VAR_MAX_RADIUS + 1], sum = 0.0;
    for (int i = -t.r; i <= t.r; i++) sum += e[i + t.r] = exp(-(double)(i * i) / (2.0 * s * s));
    for (int i = 0; i <= 2 * t.r; i++) t.t[i] = (float)(e[i] / sum);
    return t;
}

int launch_var_smooth(int H, int W, const uint8_t *bgr, float sigma, float *o0, float *o1, float *o2, hipStream_t s)
{
    const dim3 stiles((W + VAR_ST - 1) / VAR_ST, (H + VAR_ST - 1) / VAR_ST);
    var_smooth_kernel<<<stiles, VAR_THREADS, 0, s>>>(bgr, H, W, var_taps(sigma), o0, o1, o2);
    return dflow_check_launch("var_smooth_kernel");
}

int launch_var(int H, int W, const uint8_t *bgr1, const uint8_t *bgr2, const float *flow_in, const dflow_var_params *p,
               float *flow_out, void *ws, hipStream_t s)
{
    const VarWs w = var_ws(ws, H, W);
    const dim3 block(VAR_BX, VAR_BY), grid((W + VAR_BX - 1) / VAR_BX, (H + VAR_BY - 1) / VAR_BY);
    const size_t plane = (size_t)H * W * sizeof(float);
    var_split_kernel<<<grid, block, 0, s>>>(H, W, flow_in, w);
    if (p->niter_outer > 0) {
        const VarTaps taps = var_taps(p->sigma);
        const dim3 stiles((W + VAR_ST - 1) / VAR_ST, (H + VAR_ST - 1) / VAR_ST);
        var_smooth_kernel<<<stiles, VAR_THREADS, 0, s>>>(bgr1, H, W, taps, w.I1[0], w.I1[1], w.I1[2]);
        var_smooth_kernel<<<stiles, VAR_THREADS, 0, s>>>(bgr2, H, W, taps, w.I2[0], w.I2[1], w.I2[2]);
        var_omega_kernel<<<grid, block, 0, s>>>(H, W, w);
    }
    const bool fused = !(p->flags & DFLOW_VAR_FLAG_SOR_UNFUSED);
    const dim3 half_grid(((W + 1) / 2 + VAR_BX - 1) / VAR_BX, grid.y);
    const dim3 fused_grid((W + VAR_TILE - 1) / VAR_TILE, (H + VAR_TILE - 1) / VAR_TILE);
    for (int outer = 0; outer < p->niter_outer; outer++) {
        var_warp_kernel<<<grid, block, 0, s>>>(H, W, w);
        var_deriv1_kernel<<<grid, block, 0, s>>>(H, W, w);
        var_deriv2_kernel<<<grid, block, 0, s>>>(H, W, w);
        int cur = 0;                                             // which of the two (du, dv) buffers is current
        DFLOW_HIP(hipMemsetAsync(w.d[0][0], 0, plane, s));
        DFLOW_HIP(hipMemsetAsync(w.d[0][1], 0, plane, s));
        for (int inner = 0; inner < p->niter_inner; inner++) {
            var_smooth_weight_kernel<<<grid, block, 0, s>>>(H, W, w, w.d[cur][0], w.d[cur][1]);
            var_coef_kernel<<<grid, block, 0, s>>>(H, W, w, w.d[cur][0], w.d[cur][1], p->alpha, p->gamma, p->delta);
            const int halves = 2 * p->niter_solver;
            if (fused) {
                for (int first = 0; first < halves; first += VAR_T, cur ^= 1)
                    var_sor_fused_kernel<<<fused_grid, VAR_FUSED_THREADS, 0, s>>>(H, W, w, w.d[cur][0], w.d[cur][1], w.d[cur ^ 1][0],
                                                                                   w.d[cur ^ 1][1], p->sor_omega, first,
                                                                                   min(VAR_T, halves - first));
            } else {
                for (int h = 0; h < halves; h++)
                    var_sor_half_kernel<<<half_grid, block, 0, s>>>(H, W, w, w.d[cur][0], w.d[cur][1], p->sor_omega, h & 1);
            }
        }
        var_add_kernel<<<grid, block, 0, s>>>(H, W, w, w.d[cur][0], w.d[cur][1]);
    }
    var_join_kernel<<<grid, block, 0, s>>>(H, W, w, flow_out);
    return dflow_check_launch("variational refinement kernels");
}
