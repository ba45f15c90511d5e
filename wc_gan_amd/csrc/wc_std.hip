// Batch standardisation + diagonal coloring (create_norm's norm 'b' with a CenterScale-family after-norm) as pure HBM streams:
// no matrix pipe anywhere.  Four streaming kernels (moments, apply, backward reduce, backward apply) and two small ones (factor,
// backward factor); DESIGN.md section 4.13.
//
// Thread layout of every streaming kernel: a block is (C/4, R) threads, R = 256 / (C/4) rows side by side.  Thread (cx, ry) owns the
// four channels 4 cx .. 4 cx + 3 for good (one 16-byte load per row) and walks rows ry, ry + R, ...; consecutive threads read
// consecutive addresses (C is the contiguous axis, so R rows of a block are one contiguous run), and no cross-lane exchange happens
// before a block's single LDS reduction.  Reductions leave float64 partials per slab and a second launch adds them in a fixed order:
// no float atomics, the same bits from run to run and from a replayed graph.
#include "wc_common.h"

namespace {

constexpr int STD_U = 4;            // rows a thread has in flight per step (independent 16-byte loads)
constexpr int STD_MAX_SLABS = 512;  // slabs per segment at most (two blocks per CU at the largest sites)
constexpr int64_t STD_SLAB_BYTES = 128 * 1024;

inline int std_rows(int C) { return 256 / (C / 4); }            // R: 1 (C = 1024) .. 32 (C = 32)

// y = relu?(fmaf(a, x, b)).  The decision is `!(t <= 0)`: a NaN stays a NaN (as K3's epilogue does).
__device__ __forceinline__ float std_act(float t, int relu) { return (!relu || !(t <= 0.f)) ? t : 0.f; }

__device__ __forceinline__ int std_slot(const int32_t* __restrict__ slot, uint32_t n, int Kt)
{
    const int k = slot[n];
    return k < 0 ? 0 : (k >= Kt ? Kt - 1 : k);       // an out-of-range class never reads outside the tables
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Reductions.  A SEGMENT is a run of HWs consecutive rows whose partials are kept apart from the other segments' (a statistic group in
// the forward, a sample in a conditional backward, everything otherwise); it is cut into nsplit slabs of rps rows.  The cut depends on
// (HWs, C) only, so a group of a grouped call is summed in exactly the order a call of its own would use.
//   MODE 0: P[slab][0] = sum x          P[slab][1] = sum x^2
//   MODE 1: P[slab][0] = sum g'         P[slab][1] = sum g' x        g' = gy, or gy where fmaf(a, x, b) > 0 (relu): the forward's own
//                                                                    fmaf on the forward's own tables, so its decision bit for bit
// Accumulation is float64 from the first add: at 16 bytes per lane and load the VALU has an order of magnitude of slack.
template <int MODE>
__global__ __launch_bounds__(256) void std_reduce_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                         const float* __restrict__ a, const float* __restrict__ b,
                                                         const int32_t* __restrict__ slot, int64_t HWs, int nsplit, int64_t rps,
                                                         int C, int Kt, int relu, double* __restrict__ P)
{
    __shared__ double red[256 * 8];
    const int C4 = blockDim.x, R = blockDim.y, cx = threadIdx.x, ry = threadIdx.y;
    const int64_t seg = blockIdx.x / nsplit, s = blockIdx.x % nsplit;
    const int64_t row0 = seg * HWs + s * rps;
    const int64_t row1 = min(row0 + rps, (seg + 1) * HWs);
    f32x4 av = {1.f, 1.f, 1.f, 1.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 1 && relu) {
        const int k = slot ? std_slot(slot, (uint32_t)seg, Kt) : 0;
        av = *reinterpret_cast<const f32x4*>(a + (size_t)k * C + 4 * cx);
        bv = *reinterpret_cast<const f32x4*>(b + (size_t)k * C + 4 * cx);
    }
    constexpr int U = MODE == 0 ? 2 * STD_U : STD_U;       // x alone: twice the rows for the same bytes in flight
    double s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
    const float* xp = x + 4 * cx;
    const float* gp = gy + 4 * cx;
    for (int64_t r = row0 + ry; r < row1; r += (int64_t)R * U) {
        f32x4 xv[U], gv[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int64_t ri = r + (int64_t)i * R;
            const bool ok = ri < row1;
            xv[i] = ok ? *reinterpret_cast<const f32x4*>(xp + ri * C) : f32x4{0.f, 0.f, 0.f, 0.f};
            if (MODE == 1) gv[i] = ok ? *reinterpret_cast<const f32x4*>(gp + ri * C) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool ok = r + (int64_t)i * R < row1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (MODE == 0) {
                    const double v = (double)xv[i][j];
                    s0[j] += v;
                    s1[j] = fma(v, v, s1[j]);
                } else {
                    float g = gv[i][j];
                    if (relu && (fmaf(av[j], xv[i][j], bv[j]) <= 0.f)) g = 0.f;
                    if (!ok) g = 0.f;                     // (a row behind the slab: its x is 0, but 0 * NaN must not enter)
                    const double gd = (double)g;
                    s0[j] += gd;
                    s1[j] = fma(gd, (double)xv[i][j], s1[j]);
                }
            }
        }
    }
    // the block's R row-lanes, added in the order ry = 0, 1, ...
    double* mine = red + ((size_t)ry * C4 + cx) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) { mine[j] = s0[j]; mine[4 + j] = s1[j]; }
    __syncthreads();
    if (ry == 0) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = mine[j];
        for (int q = 1; q < R; ++q) {
            const double* o = red + ((size_t)q * C4 + cx) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] += o[j];
        }
        double* out = P + (size_t)blockIdx.x * 2 * C + 4 * cx;
#pragma unroll
        for (int j = 0; j < 4; ++j) { out[j] = t[j]; out[C + j] = t[4 + j]; }
    }
}

// out0[k][c] = sum of P[slab][0][c] over the slabs of the segments that belong to k, out1 likewise, in ascending slab order per lane
// and ascending lane order after it.  by_segment: k IS the segment (statistic groups); else the segment's slot (NULL: everything is k = 0).
// Block (32 channels, 32 lanes) per (k, channel chunk).
__global__ __launch_bounds__(1024) void std_combine_kernel(const double* __restrict__ P, const int32_t* __restrict__ slot, int by_segment,
                                                           int64_t nseg, int nsplit, int C, int Kt,
                                                           double* __restrict__ out0, double* __restrict__ out1)
{
    __shared__ double red[2][32][33];
    const int c = blockIdx.x * 32 + threadIdx.x, lane = threadIdx.y, k = blockIdx.y;
    const int64_t p0 = by_segment ? (int64_t)k * nsplit : 0;
    const int64_t p1 = by_segment ? p0 + nsplit : nseg * nsplit;
    double t0 = 0., t1 = 0.;
    for (int64_t p = p0 + lane; p < p1; p += 32) {
        if (!by_segment && (slot ? std_slot(slot, (uint32_t)(p / nsplit), Kt) : 0) != k) continue;
        const double* q = P + (size_t)p * 2 * C + c;
        t0 += q[0];
        t1 += q[C];
    }
    red[0][lane][threadIdx.x] = t0;
    red[1][lane][threadIdx.x] = t1;
    __syncthreads();
    if (lane < 2) {
        double t = red[lane][0][threadIdx.x];
        for (int q = 1; q < 32; ++q) t += red[lane][q][threadIdx.x];
        (lane == 0 ? out0 : out1)[(size_t)k * C + c] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// factor: moments (training) or moving statistics -> mu, w = 1 / sqrt(var + eps), the moving-statistics update (groups one after the
// other, as separate calls would) and the tables a = gamma w, b = beta - a mu, row g * Kc + k.  One thread per channel; blockIdx.y
// strides the table rows, block row 0 also owns mu, w and the moving statistics (which no other block reads while training).
__device__ __forceinline__ void std_moments(const double* sum, const double* sqsum, const float* mm, const float* mv, int training,
                                            int g, int c, int C, double invM, double eps, double& mu, double& var, double& w)
{
    if (training) {
        mu = sum[(size_t)g * C + c] * invM;
        var = fmax(sqsum[(size_t)g * C + c] * invM - mu * mu, 0.);
    } else {
        mu = (double)mm[c];
        var = (double)mv[c];
    }
    w = 1. / sqrt(var + eps);
}

__global__ __launch_bounds__(64) void std_factor_kernel(const double* __restrict__ sum, const double* __restrict__ sqsum, int64_t M, int C,
                                                        int groups, double eps, double momentum, int ddof, int training,
                                                        float* moving_mean, float* moving_var,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, int Kc,
                                                        float* __restrict__ mu_out, float* __restrict__ w_out,
                                                        float* __restrict__ a, float* __restrict__ b)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double invM = 1. / (double)M;
    for (int t = blockIdx.y; t < groups * Kc; t += gridDim.y) {
        const int g = t / Kc, k = t % Kc;
        double mu, var, w;
        std_moments(sum, sqsum, moving_mean, moving_var, training, g, c, C, invM, eps, mu, var, w);
        const float af = (float)((gamma ? (double)gamma[(size_t)k * C + c] : 1.) * w);
        a[(size_t)t * C + c] = af;
        // b against the ROUNDED a: y = a (x - mu) + beta up to one rounding of b
        b[(size_t)t * C + c] = (float)((beta ? (double)beta[(size_t)k * C + c] : 0.) - (double)af * mu);
    }
    if (blockIdx.y != 0) return;
    double mmean = 0., mvar = 0.;
    const bool upd = training && moving_mean != nullptr;
    if (upd) { mmean = (double)moving_mean[c]; mvar = (double)moving_var[c]; }
    for (int g = 0; g < groups; ++g) {
        double mu, var, w;
        std_moments(sum, sqsum, moving_mean, moving_var, training, g, c, C, invM, eps, mu, var, w);
        mu_out[(size_t)g * C + c] = (float)mu;
        w_out[(size_t)g * C + c] = (float)w;
        if (upd) {
            // every group's update passes through fp32, as the stored statistics of separate calls do
            mmean = (double)(float)(momentum * mmean + (1. - momentum) * mu);
            mvar = (double)(float)(momentum * mvar + (1. - momentum) * var * ((double)M / (double)(M - ddof)));
        }
    }
    if (upd) { moving_mean[c] = (float)mmean; moving_var[c] = (float)mvar; }
}

// backward factor: per-slot sums -> dgamma, dbeta and the two per-channel coefficients of dx = a g' + q x + r
__global__ __launch_bounds__(64) void std_bwd_factor_kernel(const double* __restrict__ gsum, const double* __restrict__ gxsum,
                                                            const float* __restrict__ mu, const float* __restrict__ w,
                                                            const float* __restrict__ gamma, int64_t M, int C, int Kc, int training,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float* __restrict__ q, float* __restrict__ r)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double m = (double)mu[c], ww = (double)w[c];
    double m1 = 0., m2 = 0.;
    for (int k = 0; k < Kc; ++k) {
        const double gs = gsum[(size_t)k * C + c], gx = gxsum[(size_t)k * C + c];
        const double dg = ww * (gx - m * gs);
        const double gam = gamma ? (double)gamma[(size_t)k * C + c] : 1.;
        if (dgamma) dgamma[(size_t)k * C + c] = (float)dg;
        if (dbeta) dbeta[(size_t)k * C + c] = (float)gs;
        m1 += gam * gs;
        m2 += gam * dg;
    }
    m1 /= (double)M;
    m2 /= (double)M;
    // evaluation mode: mu and w are constants of the moving statistics, dx = a g'
    q[c] = training ? (float)(-ww * ww * m2) : 0.f;
    r[c] = training ? (float)(ww * (ww * m * m2 - m1)) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// apply (BWD = false):  y  = relu?(fmaf(a[slot], x, b[slot]))
// backward apply:       dx = fmaf(a[slot], g', fmaf(q, x, r)),  g' = gy where the forward's fmaf is > 0 (relu), recomputed
// Tiles of R * STD_U rows, grid-strided.  The two table rows of a sample stay in registers while the thread's rows stay inside it.
template <bool BWD>
__global__ __launch_bounds__(256) void std_apply_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                        const float* __restrict__ a, const float* __restrict__ b,
                                                        const float* __restrict__ q, const float* __restrict__ r,
                                                        const int32_t* __restrict__ slot, uint32_t M, uint32_t HW, int C, int Kt, int relu,
                                                        float* __restrict__ out)
{
    const int R = blockDim.y, cx = threadIdx.x, ry = threadIdx.y;
    const uint32_t tile_rows = (uint32_t)R * STD_U;
    const uint32_t ntiles = (M + tile_rows - 1) / tile_rows;
    const size_t col = 4 * (size_t)cx;
    int cur = 0;
    f32x4 av = *reinterpret_cast<const f32x4*>(a + col);
    f32x4 bv = *reinterpret_cast<const f32x4*>(b + col);
    f32x4 qv = {0.f, 0.f, 0.f, 0.f}, rv = {0.f, 0.f, 0.f, 0.f};
    if (BWD) {
        qv = *reinterpret_cast<const f32x4*>(q + col);
        rv = *reinterpret_cast<const f32x4*>(r + col);
    }
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t r0 = t * tile_rows + ry;
        f32x4 xv[STD_U], gv[STD_U];
#pragma unroll
        for (int i = 0; i < STD_U; ++i) {
            const uint32_t ri = r0 + (uint32_t)i * R;
            if (ri < M) {
                xv[i] = *reinterpret_cast<const f32x4*>(x + (size_t)ri * C + col);
                if (BWD) gv[i] = *reinterpret_cast<const f32x4*>(gy + (size_t)ri * C + col);
            }
        }
#pragma unroll
        for (int i = 0; i < STD_U; ++i) {
            const uint32_t ri = r0 + (uint32_t)i * R;
            if (ri >= M) break;
            if (slot) {
                const int k = std_slot(slot, ri / HW, Kt);
                if (k != cur) {
                    cur = k;
                    av = *reinterpret_cast<const f32x4*>(a + (size_t)k * C + col);
                    bv = *reinterpret_cast<const f32x4*>(b + (size_t)k * C + col);
                }
            }
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float f = fmaf(av[j], xv[i][j], bv[j]);
                if (!BWD) {
                    o[j] = std_act(f, relu);
                } else {
                    const float g = (relu && f <= 0.f) ? 0.f : gv[i][j];
                    o[j] = fmaf(av[j], g, fmaf(qv[j], xv[i][j], rv[j]));
                }
            }
            *reinterpret_cast<f32x4*>(out + (size_t)ri * C + col) = o;
        }
    }
}

}  // namespace

// the slab cut of a segment of HWs rows: a function of (HWs, C) alone
int wc_std_plan(int64_t HWs, int C, int64_t* rows_per_slab)
{
    int64_t n = (HWs * C * 4 + STD_SLAB_BYTES - 1) / STD_SLAB_BYTES;
    if (n < 1) n = 1;
    if (n > STD_MAX_SLABS) n = STD_MAX_SLABS;
    const int64_t rps = (HWs + n - 1) / n;
    *rows_per_slab = rps;
    return (int)((HWs + rps - 1) / rps);
}

hipError_t wc_launch_std_reduce(int mode, const float* x, const float* gy, const float* a, const float* b, const int32_t* slot,
                                int64_t nseg, int64_t HWs, int C, int Kt, int relu, double* P, hipStream_t st)
{
    int64_t rps;
    const int nsplit = wc_std_plan(HWs, C, &rps);
    const dim3 block(C / 4, std_rows(C)), grid((unsigned)(nseg * nsplit));
    if (mode == 0) hipLaunchKernelGGL(std_reduce_kernel<0>, grid, block, 0, st, x, gy, a, b, slot, HWs, nsplit, rps, C, Kt, relu, P);
    else hipLaunchKernelGGL(std_reduce_kernel<1>, grid, block, 0, st, x, gy, a, b, slot, HWs, nsplit, rps, C, Kt, relu, P);
    return hipGetLastError();
}

hipError_t wc_launch_std_combine(const double* P, const int32_t* slot, int by_segment, int64_t nseg, int64_t HWs, int C, int Kout,
                                 double* out0, double* out1, hipStream_t st)
{
    int64_t rps;
    const int nsplit = wc_std_plan(HWs, C, &rps);
    hipLaunchKernelGGL(std_combine_kernel, dim3(C / 32, Kout), dim3(32, 32), 0, st, P, slot, by_segment, nseg, nsplit, C, Kout, out0, out1);
    return hipGetLastError();
}

hipError_t wc_launch_std_factor(const double* sum, const double* sqsum, int64_t M, int C, int groups, double eps, double momentum,
                                int ddof, int training, float* moving_mean, float* moving_var, const float* gamma, const float* beta,
                                int Kc, float* mu, float* w, float* a, float* b, hipStream_t st)
{
    const int rows = groups * Kc;
    hipLaunchKernelGGL(std_factor_kernel, dim3((C + 63) / 64, rows < 64 ? rows : 64), dim3(64), 0, st, sum, sqsum, M, C, groups, eps,
                       momentum, ddof, training, moving_mean, moving_var, gamma, beta, Kc, mu, w, a, b);
    return hipGetLastError();
}

hipError_t wc_launch_std_bwd_factor(const double* gsum, const double* gxsum, const float* mu, const float* w, const float* gamma,
                                    int64_t M, int C, int Kc, int training, float* dgamma, float* dbeta, float* q, float* r,
                                    hipStream_t st)
{
    hipLaunchKernelGGL(std_bwd_factor_kernel, dim3((C + 63) / 64), dim3(64), 0, st, gsum, gxsum, mu, w, gamma, M, C, Kc, training,
                       dgamma, dbeta, q, r);
    return hipGetLastError();
}

hipError_t wc_launch_std_apply(int bwd, const float* x, const float* gy, const float* a, const float* b, const float* q, const float* r,
                               const int32_t* slot, int64_t N, int64_t HW, int C, int Kt, int relu, float* out, hipStream_t st)
{
    const int R = std_rows(C);
    const int64_t M = N * HW;
    const int64_t ntiles = (M + (int64_t)R * STD_U - 1) / ((int64_t)R * STD_U);
    const dim3 block(C / 4, R), grid((unsigned)(ntiles < 2048 ? ntiles : 2048));
    if (bwd) hipLaunchKernelGGL(std_apply_kernel<true>, grid, block, 0, st, x, gy, a, b, q, r, slot, (uint32_t)M, (uint32_t)HW, C, Kt, relu, out);
    else hipLaunchKernelGGL(std_apply_kernel<false>, grid, block, 0, st, x, gy, a, b, q, r, slot, (uint32_t)M, (uint32_t)HW, C, Kt, relu, out);
    return hipGetLastError();
}
