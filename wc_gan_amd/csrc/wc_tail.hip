// The tail of a ResNet critic (discriminator.py:57-85 of the reference: ReLU -> global pooling -> Dense heads) and the AC-GAN class loss
// as three launches -- DESIGN.md section 4.19; the projection head's three further down (section 4.20).  For y [N, HW, C] fp32 NHWC:
//
//   f[n,c]     = s sum_hw relu(y[n,hw,c])                       s = 1 (sum pooling) or 1 / HW (mean pooling)
//   out[n]     = f[n] . w_out + b_out
//   logit[n,k] = f[n] . W_cls[k] + b_cls[k]                     K > 0: the class head
//   ce[n]      = lse[n] - logit[n, label[n]]                    with labels
//
//   dlogits[n,k] = g_logits[n,k] + g_ce[n] (softmax[n,k] - 1[k = label[n]])
//   dy[n,hw,c]   = y[n,hw,c] > 0 ? s (g_out[n] w_out[c] + sum_k dlogits[n,k] W_cls[k,c]) : 0
//
// One workgroup of 1024 threads per sample in the forward and the backward pass: the pooled row and the per-channel coefficient sit in LDS,
// the heads are wave reductions in a fixed order.  The weight gradients sum over n in a fixed order, one thread per weight.  Sums in float64, every value
// rounded once.  Stream-ordered, no allocation, no atomics, plain vector stores: the same bits on every call.
#include "wc_common.h"
#include "../../include/wc_hip.h"

namespace {

constexpr int kThreads = 1024;          // forward and backward: one workgroup of 16 waves per sample, so that one sample's loads hide each other's latency
constexpr int kWaves = kThreads / 64;
constexpr int kHeadRows = 4;            // rows of the heads' weights a wave has in flight
constexpr int kMaxC = 1024;
constexpr int kMaxK = 1024;
constexpr int kMaxParts = 64;           // partial rows folded per channel (pooling) / k-groups folded per channel (coefficient)
constexpr int kWgradThreads = 256;

__device__ __forceinline__ double wave_sum(double v)
{
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float wave_max(float m)
{
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

__device__ __forceinline__ double dot4(double a, f32x4 x, f32x4 w)
{
    #pragma unroll
    for (int j = 0; j < 4; ++j) a += (double)x[j] * (double)w[j];
    return a;
}

// Thread t < R * C4 (C4 = C / 4, R = min(1024 / C4, 64) rows of the grid at a time) owns the four channels 4 (t % C4) .. + 3 of the rows
// t / C4, t / C4 + R, ...: a wave reads whole rows of y, 16 bytes per lane.
__global__ __launch_bounds__(kThreads) void tail_fwd_kernel(const float* __restrict__ y, const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                            const float* __restrict__ w_cls, const float* __restrict__ b_cls,
                                                            const int32_t* __restrict__ labels, int64_t HW, int C, int K, double s,
                                                            float* __restrict__ feat, float* __restrict__ out, float* __restrict__ logits,
                                                            float* __restrict__ lse, float* __restrict__ ce)
{
    __shared__ double part[4 * kMaxC];      // [R][C]: R * C4 <= 1024
    __shared__ __attribute__((aligned(16))) float f[kMaxC];
    __shared__ float lg[kMaxK];
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, C4 = C >> 2, R = min(kThreads / C4, kMaxParts);
    if (tid < R * C4) {
        const int c4 = tid % C4, r = tid / C4;
        const float* col = y + n * HW * C + 4 * c4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t hw = r; hw < HW; hw += R) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(col + hw * C);
            #pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[j] > 0.f ? (double)v[j] : 0.0;
        }
        #pragma unroll
        for (int j = 0; j < 4; ++j) part[r * C + 4 * c4 + j] = acc[j];
    }
    __syncthreads();
    for (int c = tid; c < C; c += kThreads) {
        double t = 0.0;
        for (int r = 0; r < R; ++r) t += part[r * C + c];
        const float v = (float)(s * t);
        f[c] = v;
        feat[n * C + c] = v;
    }
    __syncthreads();
    // the K + 1 dot products, row K the adversarial head's: wave w takes the rows 4 w .. 4 w + 3, then 64 further on, four rows' loads in flight
    const int lane = tid & 63, wave = tid >> 6;
    for (int k0 = wave * kHeadRows; k0 <= K; k0 += kWaves * kHeadRows) {
        const float* row[kHeadRows];
        double a[kHeadRows];
        #pragma unroll
        for (int r = 0; r < kHeadRows; ++r) {
            const int k = min(k0 + r, K);
            row[r] = k < K ? w_cls + (int64_t)k * C : w_out;
            a[r] = 0.0;
        }
        for (int c = 4 * lane; c < C; c += 256) {
            const f32x4 fv = *reinterpret_cast<const f32x4*>(f + c);
            f32x4 w[kHeadRows];
            #pragma unroll
            for (int r = 0; r < kHeadRows; ++r) w[r] = *reinterpret_cast<const f32x4*>(row[r] + c);
            #pragma unroll
            for (int r = 0; r < kHeadRows; ++r) a[r] = dot4(a[r], fv, w[r]);
        }
        #pragma unroll
        for (int r = 0; r < kHeadRows; ++r) {
            const double t = wave_sum(a[r]);
            const int k = k0 + r;
            if (lane == 0 && k < K) {
                const float v = (float)(t + (b_cls ? (double)b_cls[k] : 0.0));
                lg[k] = v;
                logits[n * K + k] = v;
            } else if (lane == 0 && k == K) {
                out[n] = (float)(t + (b_out ? (double)b_out[0] : 0.0));
            }
        }
    }
    if (K == 0) return;
    __syncthreads();
    if (wave != 0) return;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, lg[k]);
    m = wave_max(m);
    double e = 0.0;
    for (int k = lane; k < K; k += 64) e += exp((double)lg[k] - (double)m);
    e = wave_sum(e);
    if (lane == 0) {
        const float l = (float)((double)m + log(e));
        lse[n] = l;
        if (ce) {
            const int32_t lab = labels[n];
            ce[n] = (lab >= 0 && lab < K) ? (float)((double)l - (double)lg[lab]) : __builtin_nanf("");
        }
    }
}

__global__ __launch_bounds__(kThreads) void tail_bwd_kernel(const float* __restrict__ y, const float* __restrict__ w_out, const float* __restrict__ w_cls,
                                                            const float* __restrict__ g_out, const float* __restrict__ g_logits,
                                                            const float* __restrict__ g_ce, const float* __restrict__ logits,
                                                            const float* __restrict__ lse, const int32_t* __restrict__ labels, int64_t HW, int C,
                                                            int K, double s, float* __restrict__ dlogits, float* __restrict__ dy)
{
    __shared__ double pc[4 * kMaxC];        // [G][C]: G * C4 <= 1024
    __shared__ float dl[kMaxK];
    __shared__ __attribute__((aligned(16))) float coef[kMaxC];
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, C4 = C >> 2;
    if (K > 0) {
        int32_t lab = -1;
        double gc = 0.0, l = 0.0;
        if (g_ce) {
            lab = labels[n];
            if (lab >= 0 && lab < K) { gc = (double)g_ce[n]; l = (double)lse[n]; }
            else lab = -1;                  // a label outside [0, K): no class gradient for this sample
        }
        for (int k = tid; k < K; k += kThreads) {
            double d = g_logits ? (double)g_logits[n * K + k] : 0.0;
            if (lab >= 0) d += gc * (exp((double)logits[n * K + k] - l) - (k == lab ? 1.0 : 0.0));
            const float v = (float)d;
            dl[k] = v;
            dlogits[n * K + k] = v;
        }
        __syncthreads();
    }
    // coef[c] = s (g_out w_out[c] + sum_k dl[k] W_cls[k][c]): group g of G takes the rows k = g, g + G, ... (four loads in flight), group 0 the
    // adversarial head's term as well; the groups' partial sums are folded in a fixed order
    const int G = min(kThreads / C4, kMaxParts);
    if (tid < G * C4) {
        const int c4 = tid % C4, grp = tid / C4;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        if (grp == 0) {
            const double go = (double)g_out[n];
            const f32x4 w = *reinterpret_cast<const f32x4*>(w_out + 4 * c4);
            #pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = go * (double)w[j];
        }
        for (int k0 = grp; k0 < K; k0 += 4 * G) {
            f32x4 w[4];
            double d[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + u * G;
                const int kk = k < K ? k : k0;          // (a row past the end: an in-range address, weight zero)
                w[u] = *reinterpret_cast<const f32x4*>(w_cls + (int64_t)kk * C + 4 * c4);
                d[u] = k < K ? (double)dl[kk] : 0.0;
            }
            #pragma unroll
            for (int u = 0; u < 4; ++u)
                #pragma unroll
                for (int j = 0; j < 4; ++j) a[j] += d[u] * (double)w[u][j];
        }
        #pragma unroll
        for (int j = 0; j < 4; ++j) pc[grp * C + 4 * c4 + j] = a[j];
    }
    __syncthreads();
    for (int c = tid; c < C; c += kThreads) {
        double t = 0.0;
        for (int g = 0; g < G; ++g) t += pc[g * C + c];
        coef[c] = (float)(s * t);
    }
    __syncthreads();
    const int R = kThreads / C4;
    if (tid < R * C4) {
        const int c4 = tid % C4, r = tid / C4;
        const f32x4 cf = *reinterpret_cast<const f32x4*>(coef + 4 * c4);
        const int64_t base = n * HW * C + 4 * c4;
        for (int64_t hw = r; hw < HW; hw += R) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(y + base + hw * C);
            f32x4 d;
            #pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = v[j] > 0.f ? cf[j] : 0.f;
            *reinterpret_cast<f32x4*>(dy + base + hw * C) = d;
        }
    }
}

// blockIdx.x = the row (k < K: the class head's, K: the adversarial head's), blockIdx.y = a block of 256 channels; one thread per weight,
// the samples in order, eight loads in flight
__global__ __launch_bounds__(kWgradThreads) void tail_wgrad_kernel(const float* __restrict__ feat, const float* __restrict__ g_out,
                                                                   const float* __restrict__ dlogits, int64_t N, int C, int K,
                                                                   float* __restrict__ dw_out, float* __restrict__ db_out,
                                                                   float* __restrict__ dW_cls, float* __restrict__ db_cls)
{
    const int k = blockIdx.x, c = blockIdx.y * kWgradThreads + threadIdx.x;
    const float* g = k < K ? dlogits + k : g_out;
    const int64_t gs = k < K ? K : 1;
    if (c < C) {
        double a = 0.0;
        int64_t n = 0;
        for (; n + 8 <= N; n += 8) {
            float fv[8], gv[8];
            #pragma unroll
            for (int u = 0; u < 8; ++u) { fv[u] = feat[(n + u) * C + c]; gv[u] = g[(n + u) * gs]; }
            #pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)gv[u] * (double)fv[u];
        }
        for (; n < N; ++n) a += (double)g[n * gs] * (double)feat[n * C + c];
        if (k < K) dW_cls[(int64_t)k * C + c] = (float)a;
        else dw_out[c] = (float)a;
    }
    if (blockIdx.y == 0 && threadIdx.x < 64) {      // the bias: lane-strided partial sums folded in a fixed order
        double b = 0.0;
        for (int64_t n = threadIdx.x; n < N; n += 64) b += (double)g[n * gs];
        b = wave_sum(b);
        if (threadIdx.x == 0) {
            if (k < K) db_cls[k] = (float)b;
            else db_out[0] = (float)b;
        }
    }
}

// ---- the projection head (discriminator.py:77-82 of the reference: out = psi(f) + <emb[cls], f>), DESIGN.md section 4.20 ----
//
//   out[n]     = f[n] . (w_out + E[cls[n]]) + b_out
//   dy[n,hw,c] = y[n,hw,c] > 0 ? s g_out[n] (w_out[c] + E[cls[n],c]) : 0
//   dE[k,c]    = sum_{n : cls[n] = k} g_out[n] f[n,c]            (ascending n; a class no sample carries: exactly 0)
//
// The pooling is tail_fwd_kernel's, sum for sum; a label outside [0, K) reads no row of E: its out is NaN, its dy the adversarial head's alone.
__global__ __launch_bounds__(kThreads) void proj_fwd_kernel(const float* __restrict__ y, const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                            const float* __restrict__ emb, const int32_t* __restrict__ cls, int64_t HW, int C, int K,
                                                            double s, float* __restrict__ feat, float* __restrict__ out)
{
    __shared__ double part[4 * kMaxC];      // [R][C]: R * C4 <= 1024
    __shared__ __attribute__((aligned(16))) float f[kMaxC];
    __shared__ double wp[kWaves];
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, C4 = C >> 2, R = min(kThreads / C4, kMaxParts);
    if (tid < R * C4) {
        const int c4 = tid % C4, r = tid / C4;
        const float* col = y + n * HW * C + 4 * c4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t hw = r; hw < HW; hw += R) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(col + hw * C);
            #pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += v[j] > 0.f ? (double)v[j] : 0.0;
        }
        #pragma unroll
        for (int j = 0; j < 4; ++j) part[r * C + 4 * c4 + j] = acc[j];
    }
    __syncthreads();
    for (int c = tid; c < C; c += kThreads) {
        double t = 0.0;
        for (int r = 0; r < R; ++r) t += part[r * C + c];
        const float v = (float)(s * t);
        f[c] = v;
        feat[n * C + c] = v;
    }
    __syncthreads();
    // thread t < C4 takes the channels 4 t .. 4 t + 3 of both rows; the (at most four) waves' sums are folded in order
    const int32_t k = cls[n];
    const bool valid = k >= 0 && k < K;
    const int lane = tid & 63, wave = tid >> 6, nw = (C4 + 63) >> 6;
    if (wave < nw) {
        double a = 0.0;
        if (tid < C4) {
            const f32x4 fv = *reinterpret_cast<const f32x4*>(f + 4 * tid);
            a = dot4(a, fv, *reinterpret_cast<const f32x4*>(w_out + 4 * tid));
            if (valid) a = dot4(a, fv, *reinterpret_cast<const f32x4*>(emb + (int64_t)k * C + 4 * tid));
        }
        a = wave_sum(a);
        if (lane == 0) wp[wave] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < nw; ++w) t += wp[w];
        out[n] = valid ? (float)(t + (b_out ? (double)b_out[0] : 0.0)) : __builtin_nanf("");
    }
}

// thread t < R * C4 (R = 1024 / C4) forms the coefficient of its four channels itself: no LDS
__global__ __launch_bounds__(kThreads) void proj_bwd_kernel(const float* __restrict__ y, const float* __restrict__ w_out, const float* __restrict__ emb,
                                                            const int32_t* __restrict__ cls, const float* __restrict__ g_out, int64_t HW, int C, int K,
                                                            double s, float* __restrict__ dy)
{
    const int64_t n = blockIdx.x;
    const int tid = threadIdx.x, C4 = C >> 2, R = kThreads / C4;
    if (tid >= R * C4) return;
    const int c4 = tid % C4, r = tid / C4;
    const int32_t k = cls[n];
    const double sg = s * (double)g_out[n];
    const f32x4 w = *reinterpret_cast<const f32x4*>(w_out + 4 * c4);
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
    if (k >= 0 && k < K) e = *reinterpret_cast<const f32x4*>(emb + (int64_t)k * C + 4 * c4);
    f32x4 cf;
    #pragma unroll
    for (int j = 0; j < 4; ++j) cf[j] = (float)(sg * ((double)w[j] + (double)e[j]));
    const int64_t base = n * HW * C + 4 * c4;
    for (int64_t hw = r; hw < HW; hw += R) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + base + hw * C);
        f32x4 d;
        #pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = v[j] > 0.f ? cf[j] : 0.f;
        *reinterpret_cast<f32x4*>(dy + base + hw * C) = d;
    }
}

// blockIdx.x = the row (k < K: the table's, K: the adversarial head's), blockIdx.y = a block of 256 channels; one thread per weight, the
// samples in order.  A table row takes the samples of its class -- the test is the same for every thread --, so every row is written in full.
__global__ __launch_bounds__(kWgradThreads) void proj_wgrad_kernel(const float* __restrict__ feat, const float* __restrict__ g_out,
                                                                   const int32_t* __restrict__ cls, int64_t N, int C, int K,
                                                                   float* __restrict__ dw_out, float* __restrict__ db_out, float* __restrict__ demb)
{
    const int k = blockIdx.x, c = blockIdx.y * kWgradThreads + threadIdx.x;
    if (k < K) {
        if (c >= C) return;
        double a = 0.0;
        for (int64_t n = 0; n < N; ++n)
            if (cls[n] == k) a += (double)g_out[n] * (double)feat[n * C + c];
        demb[(int64_t)k * C + c] = (float)a;
        return;
    }
    if (c < C) {
        double a = 0.0;
        int64_t n = 0;
        for (; n + 8 <= N; n += 8) {
            float fv[8], gv[8];
            #pragma unroll
            for (int u = 0; u < 8; ++u) { fv[u] = feat[(n + u) * C + c]; gv[u] = g_out[n + u]; }
            #pragma unroll
            for (int u = 0; u < 8; ++u) a += (double)gv[u] * (double)fv[u];
        }
        for (; n < N; ++n) a += (double)g_out[n] * (double)feat[n * C + c];
        dw_out[c] = (float)a;
    }
    if (blockIdx.y == 0 && threadIdx.x < 64) {      // the bias: lane-strided partial sums folded in a fixed order
        double b = 0.0;
        for (int64_t n = threadIdx.x; n < N; n += 64) b += (double)g_out[n];
        b = wave_sum(b);
        if (threadIdx.x == 0) db_out[0] = (float)b;
    }
}

}  // namespace

static bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }      // y, dy and the heads' weights are read 16 bytes at a time

extern "C" {

int wc_critic_tail_supported(int64_t N, int64_t HW, int C, int K)
{
    if (N < 1 || HW < 1 || C < 4 || C > kMaxC || (C & 3) || K < 0 || K > kMaxK) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if (N >= lim || HW >= lim || N * HW >= lim || N * HW * C >= lim) return 0;
    return 1;
}

int wc_critic_tail_fwd_f32(const float* y, const float* w_out, const float* b_out, const float* w_cls, const float* b_cls, const int32_t* labels,
                           int64_t N, int64_t HW, int C, int K, int sum_pool, float* feat, float* out, float* logits, float* lse, float* ce,
                           wc_stream_t stream)
{
    if (sum_pool != 0 && sum_pool != 1) return WC_ERR_ARG;
    if (!wc_critic_tail_supported(N, HW, C, K)) return WC_ERR_SHAPE;
    if (!y || !w_out || !feat || !out) return WC_ERR_NULL;
    if (K > 0 && (!w_cls || !logits || !lse)) return WC_ERR_NULL;
    if (misaligned(y) || misaligned(w_out) || misaligned(w_cls)) return WC_ERR_ARG;
    if ((labels != nullptr) != (ce != nullptr)) return WC_ERR_NULL;
    if (labels && K == 0) return WC_ERR_ARG;
    hipLaunchKernelGGL(tail_fwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, y, w_out, b_out, w_cls, b_cls, labels, HW, C, K,
                       sum_pool ? 1.0 : 1.0 / (double)HW, feat, out, logits, lse, ce);
    return (int)hipGetLastError();
}

int wc_critic_tail_bwd_f32(const float* y, const float* w_out, const float* w_cls, const float* g_out, const float* g_logits, const float* g_ce,
                           const float* logits, const float* lse, const int32_t* labels, int64_t N, int64_t HW, int C, int K, int sum_pool,
                           float* dlogits, float* dy, wc_stream_t stream)
{
    if (sum_pool != 0 && sum_pool != 1) return WC_ERR_ARG;
    if (!wc_critic_tail_supported(N, HW, C, K)) return WC_ERR_SHAPE;
    if (!y || !w_out || !g_out || !dy) return WC_ERR_NULL;
    if (K > 0 && (!w_cls || !dlogits)) return WC_ERR_NULL;
    if (misaligned(y) || misaligned(dy) || misaligned(w_out) || misaligned(w_cls)) return WC_ERR_ARG;
    if (K == 0 && (g_logits || g_ce)) return WC_ERR_ARG;
    if (g_ce && (!logits || !lse || !labels)) return WC_ERR_NULL;
    hipLaunchKernelGGL(tail_bwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, y, w_out, w_cls, g_out, g_logits, g_ce, logits, lse,
                       labels, HW, C, K, sum_pool ? 1.0 : 1.0 / (double)HW, dlogits, dy);
    return (int)hipGetLastError();
}

int wc_critic_tail_wgrad_f32(const float* feat, const float* g_out, const float* dlogits, int64_t N, int C, int K, float* dw_out, float* db_out,
                             float* dW_cls, float* db_cls, wc_stream_t stream)
{
    if (!wc_critic_tail_supported(N, 1, C, K)) return WC_ERR_SHAPE;
    if (!feat || !g_out || !dw_out || !db_out) return WC_ERR_NULL;
    if (K > 0 && (!dlogits || !dW_cls || !db_cls)) return WC_ERR_NULL;
    hipLaunchKernelGGL(tail_wgrad_kernel, dim3((unsigned)(K + 1), (unsigned)((C + kWgradThreads - 1) / kWgradThreads)), dim3(kWgradThreads), 0,
                       (hipStream_t)stream, feat, g_out, dlogits, N, C, K, dw_out, db_out, dW_cls, db_cls);
    return (int)hipGetLastError();
}

int wc_critic_proj_supported(int64_t N, int64_t HW, int C, int K) { return K >= 1 && wc_critic_tail_supported(N, HW, C, K); }

int wc_critic_proj_fwd_f32(const float* y, const float* w_out, const float* b_out, const float* emb, const int32_t* cls, int64_t N, int64_t HW, int C,
                           int K, int sum_pool, float* feat, float* out, wc_stream_t stream)
{
    if (sum_pool != 0 && sum_pool != 1) return WC_ERR_ARG;
    if (!wc_critic_proj_supported(N, HW, C, K)) return WC_ERR_SHAPE;
    if (!y || !w_out || !emb || !cls || !feat || !out) return WC_ERR_NULL;
    if (misaligned(y) || misaligned(w_out) || misaligned(emb)) return WC_ERR_ARG;
    hipLaunchKernelGGL(proj_fwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, y, w_out, b_out, emb, cls, HW, C, K,
                       sum_pool ? 1.0 : 1.0 / (double)HW, feat, out);
    return (int)hipGetLastError();
}

int wc_critic_proj_bwd_f32(const float* y, const float* w_out, const float* emb, const int32_t* cls, const float* g_out, int64_t N, int64_t HW, int C,
                           int K, int sum_pool, float* dy, wc_stream_t stream)
{
    if (sum_pool != 0 && sum_pool != 1) return WC_ERR_ARG;
    if (!wc_critic_proj_supported(N, HW, C, K)) return WC_ERR_SHAPE;
    if (!y || !w_out || !emb || !cls || !g_out || !dy) return WC_ERR_NULL;
    if (misaligned(y) || misaligned(dy) || misaligned(w_out) || misaligned(emb)) return WC_ERR_ARG;
    hipLaunchKernelGGL(proj_bwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, y, w_out, emb, cls, g_out, HW, C, K,
                       sum_pool ? 1.0 : 1.0 / (double)HW, dy);
    return (int)hipGetLastError();
}

int wc_critic_proj_wgrad_f32(const float* feat, const float* g_out, const int32_t* cls, int64_t N, int C, int K, float* dw_out, float* db_out,
                             float* demb, wc_stream_t stream)
{
    if (!wc_critic_proj_supported(N, 1, C, K)) return WC_ERR_SHAPE;
    if (!feat || !g_out || !cls || !dw_out || !db_out || !demb) return WC_ERR_NULL;
    hipLaunchKernelGGL(proj_wgrad_kernel, dim3((unsigned)(K + 1), (unsigned)((C + kWgradThreads - 1) / kWgradThreads)), dim3(kWgradThreads), 0,
                       (hipStream_t)stream, feat, g_out, cls, N, C, K, dw_out, db_out, demb);
    return (int)hipGetLastError();
}

}  // extern "C"
