// Adam with the recipes' learning-rate schedules (run.py:99-144, --lr_decay_schedule) in one pass over a network's parameters -- DESIGN.md
// section 4.18.  Two kernels:
//
//   * adam_tick_kernel: one thread.  Reads the int64 update counter (`it` = updates already applied), forms the schedule's multiplier,
//     lr * mult / (1 - beta1^(it+1)) and 1 / sqrt(1 - beta2^(it+1)) in float64, leaves them in a four-float record and increments the
//     counter.  The step is replayed from a hipGraph, so none of this can be a host value baked into a kernel argument.
//   * adam_update_kernel: a pure streaming pass, no LDS, no atomics.  The parameters (and in the single-process trainer the gradients) are
//     separate allocations, so the launch takes a by-value table of (parameter, gradient, offset into the flat moment buffers, numel) and
//     a prefix sum of chunks; a workgroup finds its (tensor, chunk) by bisection of the prefix sum -- blockIdx is wave-uniform, so the
//     table is read with scalar loads from the kernel-argument segment.  16-byte loads and stores (cdna_hip_programming.md Guideline 13:
//     16 B per lane, 1 KiB per wave instruction) where BOTH the parameter and the gradient pointer are 16-byte aligned; a gradient that
//     is a view into a flat bucket starts at an arbitrary element, and such a tensor takes the 4-byte path as a whole (chosen per tensor
//     from the pointers, never assumed).  The moment segments are padded to four elements and 16-byte aligned by construction.
//     45 / 52 VGPRs, no scratch: occupancy is the 8 waves per SIMD the chip allows (MI355X_MICROARCH.md), latency is hidden by resident
//     waves, and a chunk of 2048 elements gives a 1 M-parameter critic ~520 workgroups for 256 CUs (measured: DESIGN.md section 4.18).
//
// With beta1 == 0 (every recipe) exp_avg equals the gradient: it is neither stored nor read (HAS_M = false), 20 bytes per parameter
// instead of 28.  Stream-ordered, allocates nothing, plain vector stores.
#include "wc_common.h"
#include "../../include/wc_hip.h"

namespace {

enum { kNone = 0, kLinear = 1, kHalfLinear = 2, kLinearEnd = 3, kDropAt = 4 };

__device__ __forceinline__ double schedule_multiplier(int kind, double it, double total, double drop_at)
{
    if (kind == kNone) return 1.0;
    const double lin = fmax(0.0, 1.0 - it / total);
    if (kind == kLinear) return lin;
    if (kind == kHalfLinear) return it < 0.5 * total ? lin : 0.5;
    if (kind == kLinearEnd) return fmin(1.0, fmax(0.0, (total - it) / (total - 0.828 * total)));
    return (it < drop_at ? 1.0 : 0.1) * lin;
}

__global__ __launch_bounds__(64) void adam_tick_kernel(int64_t* __restrict__ counter, float* __restrict__ record, double lr, double beta1,
                                                       double beta2, int kind, double total, double drop_at)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t it = counter[0];
    const double mult = schedule_multiplier(kind, (double)it, total, drop_at);
    const double step = (double)(it + 1);
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    const f32x4 r = {(float)(lr * mult / bc1), (float)(1.0 / sqrt(bc2)), (float)(lr * mult), (float)mult};
    *reinterpret_cast<f32x4*>(record) = r;
    counter[0] = it + 1;
}

// The moments are formed in float64 and rounded once, as torch's fused kernel does (its betas are doubles): the stored exp_avg_sq carries
// one rounding per step and no more.  The parameter's own update is float32 arithmetic: its error is |update| x a few 2^-24, far below
// the rounding of the stored parameter.
template <bool HAS_M>
__device__ __forceinline__ float adam_one(float p, float g, float& m, float& v, double omb1, double beta2, double omb2, float eps, float a, float r)
{
    float mm = g;
    if (HAS_M) { m = (float)((double)m + omb1 * ((double)g - (double)m)); mm = m; }
    v = (float)(beta2 * (double)v + omb2 * ((double)g * (double)g));
    return p - a * (mm / (sqrtf(v) * r + eps));
}

template <bool HAS_M>
__global__ __launch_bounds__(256) void adam_update_kernel(const wc_adam_table t, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                          const float* __restrict__ record, double omb1, double beta2, double omb2, float eps)
{
    const int bid = blockIdx.x;
    int lo = 0, hi = t.count;                 // chunk_start[lo] <= bid < chunk_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.chunk_start[mid] <= bid) lo = mid; else hi = mid;
    }
    const int n = t.numel[lo];
    const int begin = (bid - t.chunk_start[lo]) * t.chunk;
    if (begin >= n) return;
    const int end = min(n, begin + t.chunk);
    float* __restrict__ p = t.param[lo];
    const float* __restrict__ g = t.grad[lo];
    float* __restrict__ v = exp_avg_sq + t.moment_off[lo];
    float* __restrict__ m = HAS_M ? exp_avg + t.moment_off[lo] : nullptr;
    const float a = record[0], r = record[1];
    const bool wide = (((uintptr_t)p | (uintptr_t)g) & 15) == 0;
    int done = begin;
    if (wide) {
        const int end4 = begin + ((end - begin) & ~3);
        for (int i = begin + 4 * (int)threadIdx.x; i < end4; i += 1024) {
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
            f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
            f32x4 mv = {0.f, 0.f, 0.f, 0.f};
            if (HAS_M) mv = *reinterpret_cast<const f32x4*>(m + i);
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mj = mv[j], vj = vv[j];
                pv[j] = adam_one<HAS_M>(pv[j], gv[j], mj, vj, omb1, beta2, omb2, eps, a, r);
                mv[j] = mj; vv[j] = vj;
            }
            *reinterpret_cast<f32x4*>(p + i) = pv;
            *reinterpret_cast<f32x4*>(v + i) = vv;
            if (HAS_M) *reinterpret_cast<f32x4*>(m + i) = mv;
        }
        done = end4;
    }
    // the 4-byte path: a whole tensor whose gradient (or parameter) is not 16-byte aligned, and the last numel % 4 elements otherwise
    for (int i = done + (int)threadIdx.x; i < end; i += 256) {
        float mj = HAS_M ? m[i] : 0.f, vj = v[i];
        p[i] = adam_one<HAS_M>(p[i], g[i], mj, vj, omb1, beta2, omb2, eps, a, r);
        v[i] = vj;
        if (HAS_M) m[i] = mj;
    }
}

}  // namespace

extern "C" {

int wc_adam_capacity(void) { return WC_ADAM_CAPACITY; }

int wc_adam_tick(int64_t* counter, float* record, double lr, double beta1, double beta2, int kind, double total, double drop_at,
                 wc_stream_t stream)
{
    if (!counter || !record) return WC_ERR_NULL;
    if (((uintptr_t)record & 15) || ((uintptr_t)counter & 7)) return WC_ERR_ARG;
    if (kind < kNone || kind > kDropAt || !(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return WC_ERR_ARG;
    if (kind != kNone && !(total > 0.0)) return WC_ERR_ARG;
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter, record, lr, beta1, beta2, kind, total, drop_at);
    return (int)hipGetLastError();
}

int wc_adam_update_f32(const wc_adam_table* table, float* exp_avg, float* exp_avg_sq, int64_t moment_elems, const float* record,
                       double beta1, double beta2, float eps, wc_stream_t stream)
{
    if (!table || !exp_avg_sq || !record) return WC_ERR_NULL;
    if (beta1 != 0.0 && !exp_avg) return WC_ERR_NULL;
    const wc_adam_table& t = *table;
    if (t.count < 1 || t.count > WC_ADAM_CAPACITY || t.chunk < 1024 || (t.chunk & 1023) || t.chunk_start[0] != 0) return WC_ERR_ARG;
    if (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return WC_ERR_ARG;
    for (int i = 0; i < t.count; ++i) {
        // every workgroup of the launch must land inside its tensor and its moment segment: checked here, not in the kernel
        if (!t.param[i] || !t.grad[i]) return WC_ERR_NULL;
        if (((uintptr_t)t.param[i] | (uintptr_t)t.grad[i]) & 3) return WC_ERR_ARG;
        if (t.numel[i] < 1 || t.numel[i] > INT32_MAX - t.chunk) return WC_ERR_SHAPE;
        if (t.chunk_start[i + 1] - t.chunk_start[i] != (t.numel[i] + t.chunk - 1) / t.chunk) return WC_ERR_SHAPE;
        if (t.moment_off[i] < 0 || (t.moment_off[i] & 3) || t.moment_off[i] + (int64_t)t.numel[i] > moment_elems) return WC_ERR_SHAPE;
    }
    const int grid = t.chunk_start[t.count];
    const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.f)) return WC_ERR_ARG;
    if (beta1 != 0.0)
        hipLaunchKernelGGL(adam_update_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, t, exp_avg, exp_avg_sq, record, omb1, beta2,
                           omb2, eps);
    else
        hipLaunchKernelGGL(adam_update_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, t, exp_avg, exp_avg_sq, record, omb1, beta2,
                           omb2, eps);
    return (int)hipGetLastError();
}

}  // extern "C"
