// The per-element work of a MASKED operand split -- planes of t * (a > 0 ? 1 : slope) and the bias gradient's column sums of the masked
// values -- in one place for its two users: the gradient penalty's tangent splits (wc_gp.hip) and the critic's k-split finish that writes
// conv1's masked output-gradient planes (wc_conv.hip: conv_finish_split_body).  One source per expression: the mask's multiply and the
// column sums' add keep the rounding they have in gp_split_hist_kernel wherever they are inlined.
#pragma once
#include "wc_common.h"

__device__ __forceinline__ f32x4 wc_mask_apply(f32x4 v, const f32x4 p, float slope)
{
    #pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * (p[j] > 0.f ? 1.0f : slope);      // (a NaN or -0 pre-activation takes the slope, as torch's a > 0)
    return v;
}

// The ReLU's backward on a gradient that feeds a SUM right away (the narrow weight gradient of the critic's first block, wc_conv.hip:
// conv_wrw_narrow_body): torch's threshold_backward(v, p, 0) predicate, p <= 0 -- a NaN pre-activation lets the gradient THROUGH, unlike
// wc_mask_apply's p > 0 -- as a multiply, so a masked-out element is (+-0) and leaves a sum that started as +0 as it would have been.
__device__ __forceinline__ f32x4 wc_relu_mask_apply(f32x4 v, const f32x4 p)
{
    #pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * (p[j] <= 0.f ? 0.f : 1.0f);
    return v;
}

__device__ __forceinline__ f32x4 wc_colsum_add(f32x4 cs, f32x4 v)
{
    #pragma unroll
    for (int j = 0; j < 4; ++j) cs[j] = __fadd_rn(cs[j], v[j]);      // (never contracted with the mask's multiply)
    return cs;
}
