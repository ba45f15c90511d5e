// Renorm's C x C stage: the whitening matrix of the MOVING statistics and its product with the batch factor.
//
// norm 'dr' whitens with W_eff = W_m sg(L) W: the value is W_m = L_m^-1, L_m L_m^T = (1 - eps) moving_cov + eps I, the gradient flows
// through the batch's W = L^-1 alone and C0 = W_m L is a constant of the step.  The moving factor is K2's evaluation-mode launch
// sequence itself (wc_small.hip: prepare, Cholesky, triangular inverse -- the same kernels, the same bits as wc_factor_f64 with
// training == 0); what is new here is the triangular product.
//
// tri_gemm_kernel: float64 on v_mfma_f64_16x16x4_f64, one 16 x 16 output tile per wave (four waves = one 32 x 32 block per
// workgroup), operands straight from global memory (C x C doubles: they live in L2) with the next 16 k in flight under the
// current four MFMAs.  A tile runs k only where both operands can be non-zero:
//   TRI_LL  lower x lower  (C0 = W_m L):            tiles above the diagonal are written as zeros, tile (i, j) runs k over j..i
//   TRI_UG  upper x general (C0^T Wbar, K5 of 'dr'): tile (i, j) runs k over i..C/16-1
// An MFMA of this shape takes 64 cycles whatever feeds it (profiles/r6_mfma_f64_rate.txt), so the longest chain -- C / 4 MFMAs of tile
// (last, 0) -- bounds the launch: 7 us at C = 1024, 1.8 us at C = 256, where the dense product runs C / 4 in every tile.
// Elements on the far side of the operands' diagonals are masked to zero on load, not trusted to be zero.
#include "../../include/wc_hip.h"
#include "wc_common.h"

namespace {

inline bool renorm_width_ok(int C) { return C >= 32 && C <= 1024 && (C % 32) == 0; }
inline size_t renorm_slot(size_t n, size_t elem) { return wc_align_up(n * elem, 256); }
#define WC_RN_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

enum { TRI_LL = 0, TRI_UG = 1 };

// Operand maps of v_mfma_f64_16x16x4_f64 (as in gemm_f64_kernel): a = A[i = lane & 15][k = lane >> 4], b = B[k = lane >> 4][j = lane & 15],
// D register r of lane l = D[(l >> 4) + 4 r][l & 15].  Strides in elements; Cm row-major C x C.
template <int MODE>
__global__ __launch_bounds__(256) void tri_gemm_kernel(const double* __restrict__ A, int64_t a_rs, int64_t a_cs,
                                                       const double* __restrict__ B, int64_t b_rs, int64_t b_cs,
                                                       double* __restrict__ Cm, int C)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int ti = blockIdx.x * 2 + (wave >> 1), tj = blockIdx.y * 2 + (wave & 1);      // this wave's 16 x 16 tile
    const int gi = ti * 16 + li;            // the row of A this lane feeds
    const int gj = tj * 16 + li;            // the column of B this lane feeds
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    const bool live = MODE == TRI_UG || tj <= ti;
    if (live) {
        const int kbeg = (MODE == TRI_LL ? tj : ti) * 16;
        const int kend = MODE == TRI_LL ? (ti + 1) * 16 : C;
        const double* Ar = A + (int64_t)gi * a_rs;
        const double* Bc = B + (int64_t)gj * b_cs;
        // A[i][k] is zero for k > i (TRI_LL: lower) or k < i (TRI_UG: upper); TRI_LL's B[k][j] is zero for k < j
        auto load16 = [&](int k0, double (&x)[4], double (&y)[4]) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 4 * u + lq;
                const double a = Ar[(int64_t)k * a_cs], b = Bc[(int64_t)k * b_rs];
                x[u] = (MODE == TRI_LL ? k <= gi : k >= gi) ? a : 0.0;
                y[u] = (MODE == TRI_LL && k < gj) ? 0.0 : b;
            }
        };
        double a[4], b[4];
        load16(kbeg, a, b);
        for (int kk = kbeg; kk < kend; kk += 16) {
            double na[4], nb[4];
            load16(kk + 16 < kend ? kk + 16 : kk, na, nb);          // (the last group re-reads itself: no predicated loads)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = na[u]; b[u] = nb[u]; }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = ti * 16 + lq + 4 * r, col = tj * 16 + li;
        Cm[(int64_t)row * C + col] = (MODE == TRI_LL && col > row) ? 0.0 : acc[r];
    }
}

}  // namespace

// Cm = A B (row-major C x C doubles, C % 32 == 0) with A lower and B lower (upper == 0: Cm lower, its upper triangle exact zeros) or A upper
// and B general (upper != 0)
hipError_t wc_launch_tri_gemm(int upper, const double* A, int64_t a_rs, int64_t a_cs, const double* B, int64_t b_rs, int64_t b_cs,
                              double* Cm, int C, hipStream_t st)
{
    const dim3 grid(C / 32, C / 32);
    if (upper) hipLaunchKernelGGL(tri_gemm_kernel<TRI_UG>, grid, dim3(256), 0, st, A, a_rs, a_cs, B, b_rs, b_cs, Cm, C);
    else hipLaunchKernelGGL(tri_gemm_kernel<TRI_LL>, grid, dim3(256), 0, st, A, a_rs, a_cs, B, b_rs, b_cs, Cm, C);
    return hipGetLastError();
}

extern "C" {

int wc_renorm_supported(int C) { return renorm_width_ok(C) ? 1 : 0; }

// L_m [C][C] doubles | K2's scratch [C][C] doubles
size_t wc_renorm_workspace_bytes(int C)
{
    if (!renorm_width_ok(C)) return 0;
    return 2 * renorm_slot((size_t)C * C, 8);
}

int wc_renorm_f64(const float* moving_cov, const double* L, int C, double eps, double* Wm, double* C0,
                  void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!Wm || !ws || (!moving_cov && !L) || (L && !C0)) return WC_ERR_NULL;
    if (!renorm_width_ok(C)) return WC_ERR_CHANNELS;
    if (!(eps > 0.0) || eps >= 1.0) return WC_ERR_ARG;
    if (ws_bytes < wc_renorm_workspace_bytes(C)) return WC_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (moving_cov) {
        // K2 in evaluation mode, launch for launch (wc_factor_f64 with training == 0), without the mean and the channel scale
        double* Lm = static_cast<double*>(ws);
        double* tmp = reinterpret_cast<double*>(static_cast<char*>(ws) + renorm_slot((size_t)C * C, 8));
        WC_RN_TRY(wc_launch_factor_prepare(nullptr, nullptr, 1, C, eps, 0.0, 1, 0, 1, nullptr, const_cast<float*>(moving_cov), nullptr,
                                           nullptr, Lm, st, tmp));
        if (wc_factor_is_fused(C)) {
            WC_RN_TRY(wc_launch_factor_fused(Lm, Wm, tmp, C, 1, st));
        } else {
            WC_RN_TRY(wc_launch_cholesky(Lm, C, 1, st));
            WC_RN_TRY(wc_launch_tri_inverse(Lm, Wm, tmp, C, 1, st));
        }
    }
    if (L) WC_RN_TRY(wc_launch_tri_gemm(0, Wm, C, 1, L, C, 1, C0, C, st));      // C0 = W_m L
    return WC_OK;
}

}  // extern "C"
