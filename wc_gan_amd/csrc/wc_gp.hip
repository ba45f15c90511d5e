// Gradient penalty of the WGAN-GP recipes (scripts/cifar10_resnet_wgan_*.sh: --gradinet_penalty_weight 10) in closed form -- DESIGN.md
// section 4.17.  The penalty's weight gradient is the weight gradient of a TANGENT pass through the critic with the primal pass's ReLU
// decisions frozen, so it runs on the convolution kernels of wc_conv.hip; what those do not have is in this file:
//
//   * the operand split of a tangent: planes of t * (a > 0 ? 1 : slope), a = the primal pre-activation.  The scale rule, the history
//     record and the gated second pass are those of conv_split_kernel / conv_split_hist_kernel / conv_split_redo_kernel (wc_conv.hip),
//     restated here around a two-tensor load: the planes and the scale are the bits of the existing split on the premultiplied tensor
//     (tests/test_penalty_gpu.py, which also compares the records), and wc_conv.hip itself -- every existing path's code object -- stays
//     as it is.  A change to the record's protocol or constants in wc_conv.hip has to be made here as well;
//   * x_hat = eps real + (1 - eps) fake per sample;
//   * per sample: ||g||, v = (2 lambda / N)(1 - 1 / ||g||) g, and the penalty (lambda / N) sum (||g|| - 1)^2.
//
// Stream-ordered, no allocation, no atomics, plain vector stores.
#include "wc_common.h"
#include "wc_mask.h"
#include "../../include/wc_hip.h"

namespace {

constexpr int kAmaxBlocks = 512;                    // = wc_conv.hip: workgroups of a measuring pass = (maximum, tag) pairs of a record array
constexpr float kHistMargin = 64.0f;
constexpr int kHistArray = 2 * kAmaxBlocks;
constexpr int kHistRedoWord = 2 * kHistArray;

__device__ __forceinline__ f32x4 masked_load(const float* __restrict__ t, const float* __restrict__ a, int64_t i, float slope)
{
    const f32x4 v = *reinterpret_cast<const f32x4*>(t + 4 * i);
    const f32x4 p = *reinterpret_cast<const f32x4*>(a + 4 * i);
    return wc_mask_apply(v, p, slope);             // (wc_mask.h: shared with the critic's k-split finish, wc_conv.hip)
}

__device__ __forceinline__ float absmax4(float m, f32x4 v)
{
    return fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
}

__device__ __forceinline__ void store_split(f32x4 v, float s, _Float16* __restrict__ hi, _Float16* __restrict__ lo, int64_t i)
{
    v = v * s;
    f16x4 h, l;
    #pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = (_Float16)v[j]; l[j] = (_Float16)(v[j] - (float)h[j]); }
    *reinterpret_cast<f16x4*>(hi + 4 * i) = h;
    *reinterpret_cast<f16x4*>(lo + 4 * i) = l;
}

__device__ __forceinline__ float scale_for(float amax)
{
    if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(amax, &e);
    return ldexpf(1.0f, 14 - e);
}

__device__ __forceinline__ float wave_max(float m)
{
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

// colsum (nullable) / c4n = C / 4: the bias gradient's partial rows, of the MASKED values (the tensor the premultiplied route hands its
// split), in conv_absmax_kernel's / conv_split_hist_kernel's grid, stride and LDS fold (wc_conv.hip): the rows have their bits
__device__ __forceinline__ f32x4 colsum_add(f32x4 cs, f32x4 v)
{
    return wc_colsum_add(cs, v);                   // (wc_mask.h)
}

__device__ __forceinline__ void colsum_fold(f32x4* red4, float* __restrict__ colsum, int c4n)
{
    if (colsum && (int)threadIdx.x < c4n) {
        f32x4 s = red4[threadIdx.x];
        for (int p = threadIdx.x + c4n; p < 256; p += c4n) s += red4[p];
        *reinterpret_cast<f32x4*>(colsum + (int64_t)blockIdx.x * 4 * c4n + 4 * threadIdx.x) = s;
    }
}

__global__ __launch_bounds__(256) void gp_absmax_kernel(const float* __restrict__ t, const float* __restrict__ a, int64_t n4, float slope,
                                                        float* __restrict__ partial, float* __restrict__ colsum = nullptr, int c4n = 0)
{
    __shared__ float red[4];
    __shared__ f32x4 red4[256];
    float m = 0.f;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = masked_load(t, a, i, slope);
        m = absmax4(m, v);
        cs = colsum_add(cs, v);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    if (colsum) red4[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    colsum_fold(red4, colsum, c4n);
}

__global__ __launch_bounds__(256) void gp_split_kernel(const float* __restrict__ t, const float* __restrict__ a, int64_t n4, float slope,
                                                       const float* __restrict__ amax, _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                       float* __restrict__ scale_out)
{
    float m = 0.f;
    for (int i = threadIdx.x & 63; i < kAmaxBlocks; i += 64) m = fmaxf(m, amax[i]);
    const float s = scale_for(wave_max(m));
    if (blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = s;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) store_split(masked_load(t, a, i, slope), s, hi, lo, i);
}

typedef float f32x2h __attribute__((ext_vector_type(2)));
typedef int i32x2h __attribute__((ext_vector_type(2)));

// per-workgroup maxima (first kAmaxBlocks floats of the record) -> array 0 with tag 1, array 1 with tag 0, the carried maximum in both parities
__global__ __launch_bounds__(kAmaxBlocks) void gp_hist_seed_kernel(float* __restrict__ hist)
{
    const float m = hist[threadIdx.x];
    __syncthreads();
    const f32x2h a = {m, __builtin_bit_cast(float, 1u)}, b = {0.f, __builtin_bit_cast(float, 0u)};
    *reinterpret_cast<f32x2h*>(hist + 2 * threadIdx.x) = a;
    *reinterpret_cast<f32x2h*>(hist + kHistArray + 2 * threadIdx.x) = b;
    __shared__ float red[kAmaxBlocks / 64];
    const float mm = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mm;
    __syncthreads();
    if (threadIdx.x == 0) {
        float top = 0.f;
        for (int i = 0; i < kAmaxBlocks / 64; ++i) top = fmaxf(top, red[i]);
        hist[2 * kHistArray + 2] = top; hist[2 * kHistArray + 3] = top;
    }
}

// one launch, the scale from the record the call before left (conv_split_hist_kernel's protocol, word for word)
__global__ __launch_bounds__(256) void gp_split_hist_kernel(const float* __restrict__ t, const float* __restrict__ a, int64_t n4, float slope,
                                                            _Float16* __restrict__ hi, _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                            float* __restrict__ hist, float* __restrict__ colsum, int c4n)
{
    __shared__ float red[4];
    __shared__ f32x4 red4[256];
    float mx[2] = {0.f, 0.f};
    int tlo[2] = {0x7fffffff, 0x7fffffff}, thi[2] = {0, 0};
    #pragma unroll
    for (int arr = 0; arr < 2; ++arr)
        #pragma unroll
        for (int i = 0; i < kAmaxBlocks / 64; ++i) {
            const i32x2h p = *reinterpret_cast<const i32x2h*>(hist + arr * kHistArray + 2 * ((threadIdx.x & 63) + 64 * i));
            mx[arr] = fmaxf(mx[arr], __builtin_bit_cast(float, p[0]));
            tlo[arr] = min(tlo[arr], p[1]);
            thi[arr] = max(thi[arr], p[1]);
        }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        #pragma unroll
        for (int arr = 0; arr < 2; ++arr) {
            mx[arr] = fmaxf(mx[arr], __shfl_xor(mx[arr], o));
            tlo[arr] = min(tlo[arr], __shfl_xor(tlo[arr], o));
            thi[arr] = max(thi[arr], __shfl_xor(thi[arr], o));
        }
    const bool ok0 = tlo[0] == thi[0], ok1 = tlo[1] == thi[1];
    const int src = (ok1 && (!ok0 || thi[1] > thi[0])) ? 1 : 0;
    const int tag = (src ? thi[1] : thi[0]) + 1;
    const float prev = src ? mx[1] : mx[0];
    const float assumed = prev > 0.f ? prev : hist[2 * kHistArray + 2 + src];
    const float s = scale_for(assumed * kHistMargin);
    if (blockIdx.x == 0 && threadIdx.x == 0) { scale_out[0] = s; hist[2 * kHistArray + 2 + (1 - src)] = assumed; }
    float m = 0.f;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = masked_load(t, a, i, slope);
        cs = colsum_add(cs, v);
        m = absmax4(m, v);
        store_split(v, s, hi, lo, i);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    if (colsum) red4[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x == 0) {
        const f32x2h p = {fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), __builtin_bit_cast(float, tag)};
        *reinterpret_cast<f32x2h*>(hist + (1 - src) * kHistArray + 2 * blockIdx.x) = p;
    }
    colsum_fold(red4, colsum, c4n);
}

// the gated second pass (conv_split_redo_kernel's verdict and window)
__global__ __launch_bounds__(256) void gp_split_redo_kernel(const float* __restrict__ t, const float* __restrict__ a, int64_t n4, float slope,
                                                            _Float16* __restrict__ hi, _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                            float* __restrict__ hist)
{
    float mx[2] = {0.f, 0.f};
    int tg[2] = {0, 0};
    #pragma unroll
    for (int arr = 0; arr < 2; ++arr)
        #pragma unroll
        for (int i = 0; i < kAmaxBlocks / 64; ++i) {
            const i32x2h p = *reinterpret_cast<const i32x2h*>(hist + arr * kHistArray + 2 * ((threadIdx.x & 63) + 64 * i));
            mx[arr] = fmaxf(mx[arr], __builtin_bit_cast(float, p[0]));
            tg[arr] = max(tg[arr], p[1]);
        }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        #pragma unroll
        for (int arr = 0; arr < 2; ++arr) {
            mx[arr] = fmaxf(mx[arr], __shfl_xor(mx[arr], o));
            tg[arr] = max(tg[arr], __shfl_xor(tg[arr], o));
        }
    const int now = tg[1] > tg[0] ? 1 : 0;
    const float own = mx[now], assumed = hist[2 * kHistArray + 2 + now];
    const float top = own * scale_for(assumed * kHistMargin);
    const bool fine = !(own > 0.f) || !(own < 3.0e38f) || (top >= 0.03125f && top < 65504.0f);
    if (fine) return;
    const float s = scale_for(own);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scale_out[0] = s;
        reinterpret_cast<unsigned*>(hist)[kHistRedoWord] += 1u;
    }
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) store_split(masked_load(t, a, i, slope), s, hi, lo, i);
}

int grid_for(int64_t work_items)
{
    const int64_t g = (work_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

// x_hat[n][i] = eps[n] real[n][i] + (1 - eps[n]) fake[n][i], formed in float64 and rounded once
__global__ __launch_bounds__(256) void gp_interp_kernel(const float* __restrict__ real, const float* __restrict__ fake, const float* __restrict__ eps,
                                                        int64_t total, int64_t L, float* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const double e = (double)eps[i / L];
        out[i] = (float)(e * (double)real[i] + (1.0 - e) * (double)fake[i]);
    }
}

// one workgroup per sample: float64 sum of squares in a fixed order -> norm, (norm - 1)^2 (float64, for the finish) and v
__global__ __launch_bounds__(256) void gp_rows_kernel(const float* __restrict__ g, int64_t L, double two_lambda_over_n, float* __restrict__ norms,
                                                      float* __restrict__ v, double* __restrict__ terms)
{
    __shared__ double red[4];
    const float* row = g + (int64_t)blockIdx.x * L;
    float* out = v + (int64_t)blockIdx.x * L;
    double ss = 0.0;
    for (int64_t i = threadIdx.x; i < L; i += 256) { const double x = (double)row[i]; ss += x * x; }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const double norm = sqrt((red[0] + red[1]) + (red[2] + red[3]));
    const double coef = norm > 0.0 ? two_lambda_over_n * (1.0 - 1.0 / norm) : 0.0;       // a zero row: torch's subgradient of the norm
    if (threadIdx.x == 0) { norms[blockIdx.x] = (float)norm; terms[blockIdx.x] = (norm - 1.0) * (norm - 1.0); }
    for (int64_t i = threadIdx.x; i < L; i += 256) out[i] = (float)(coef * (double)row[i]);
}

// penalty = lambda / N * sum of the N terms: one wave, lane-strided partial sums folded in a fixed order
__global__ __launch_bounds__(64) void gp_finish_kernel(const double* __restrict__ terms, int64_t N, double lambda_over_n, float* __restrict__ penalty)
{
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += 64) s += terms[i];
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (threadIdx.x == 0) penalty[0] = (float)(lambda_over_n * s);
}

}  // namespace

extern "C" {

static bool colsum_args_ok(const float* colsum_partials, int C, int64_t n)
{
    return !colsum_partials || (C > 0 && !(C & 3) && 256 % (C >> 2) == 0 && n % C == 0);      // wc_conv.hip's split_measured / split_hist
}

int wc_conv_split_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale, void* amax_scratch,
                             float* colsum_partials, int C, wc_stream_t stream)
{
    if (!t || !a || !hi || !lo || !scale || !amax_scratch || n <= 0 || (n & 3)) return WC_ERR_ARG;
    if (!(slope >= 0.f && slope <= 1.f)) return WC_ERR_ARG;
    if (!colsum_args_ok(colsum_partials, C, n)) return WC_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gp_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, t, a, n / 4, slope, (float*)amax_scratch,
                       colsum_partials, colsum_partials ? C >> 2 : 0);
    hipLaunchKernelGGL(gp_split_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, t, a, n / 4, slope, (const float*)amax_scratch,
                       (_Float16*)hi, (_Float16*)lo, scale);
    return (int)hipGetLastError();
}

int wc_conv_split_hist_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale,
                                  float* colsum_partials, int C, float* hist, int bootstrap, wc_stream_t stream)
{
    if (!t || !a || !hi || !lo || !scale || !hist || n <= 0 || (n & 3)) return WC_ERR_ARG;
    if (!(slope >= 0.f && slope <= 1.f)) return WC_ERR_ARG;
    if (!colsum_args_ok(colsum_partials, C, n)) return WC_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int c4n = colsum_partials ? C >> 2 : 0;
    if (bootstrap & 1) {
        hipLaunchKernelGGL(gp_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, t, a, n / 4, slope, hist, colsum_partials, c4n);
        hipLaunchKernelGGL(gp_split_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, t, a, n / 4, slope, (const float*)hist, (_Float16*)hi,
                           (_Float16*)lo, scale);
        hipLaunchKernelGGL(gp_hist_seed_kernel, dim3(1), dim3(kAmaxBlocks), 0, st, hist);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(gp_split_hist_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, t, a, n / 4, slope, (_Float16*)hi, (_Float16*)lo, scale, hist,
                       colsum_partials, c4n);
    if (!(bootstrap & 2)) {
        const unsigned g2 = grid_for(n / 4) < 64 ? grid_for(n / 4) : 64u;
        hipLaunchKernelGGL(gp_split_redo_kernel, dim3(g2), dim3(256), 0, st, t, a, n / 4, slope, (_Float16*)hi, (_Float16*)lo, scale, hist);
    }
    return (int)hipGetLastError();
}

// the gated second pass alone, as wc_conv_split_hist_masked_f32 launches it behind its split: for a launch that wrote the masked planes and the
// record itself (the critic's k-split finish, wc_conv_tail_f16x3 / wc_conv_bwd_pair_tail_f16x3 in wc_conv.hip)
int wc_conv_split_redo_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale, float* hist,
                                  wc_stream_t stream)
{
    if (!t || !a || !hi || !lo || !scale || !hist || n <= 0 || (n & 3)) return WC_ERR_ARG;
    if (!(slope >= 0.f && slope <= 1.f)) return WC_ERR_ARG;
    const unsigned g2 = grid_for(n / 4) < 64 ? grid_for(n / 4) : 64u;
    hipLaunchKernelGGL(gp_split_redo_kernel, dim3(g2), dim3(256), 0, (hipStream_t)stream, t, a, n / 4, slope, (_Float16*)hi, (_Float16*)lo, scale, hist);
    return (int)hipGetLastError();
}

int wc_gp_interp_f32(const float* real, const float* fake, const float* eps, int64_t N, int64_t L, float* x_hat, wc_stream_t stream)
{
    if (!real || !fake || !eps || !x_hat) return WC_ERR_NULL;
    if (N <= 0 || L <= 0) return WC_ERR_SHAPE;
    hipLaunchKernelGGL(gp_interp_kernel, dim3(grid_for(N * L)), dim3(256), 0, (hipStream_t)stream, real, fake, eps, N * L, L, x_hat);
    return (int)hipGetLastError();
}

size_t wc_gp_rows_workspace_bytes(int64_t N) { return N > 0 ? (size_t)N * sizeof(double) : 0; }

int wc_gp_rows_f32(const float* g, int64_t N, int64_t L, double lambda, double inv_n, float* norms, float* v, float* penalty,
                   void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!g || !norms || !v || !penalty || !ws) return WC_ERR_NULL;
    if (N <= 0 || L <= 0 || N >= ((int64_t)1 << 31)) return WC_ERR_SHAPE;
    if (ws_bytes < wc_gp_rows_workspace_bytes(N)) return WC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gp_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, g, L, 2.0 * lambda * inv_n, norms, v, (double*)ws);
    hipLaunchKernelGGL(gp_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, N, lambda * inv_n, penalty);
    return (int)hipGetLastError();
}

}  // extern "C"
