/*
 * wc_hip.h -- C ABI of libwc_hip.so: the MI355X (gfx950) whitening-and-coloring hot path.
 *
 * The reference has no FFI boundary for this path: it sits behind the Keras 2.0.8 Layer
 * protocol.  Each entry point below names the reference call site /
 * op group it replaces:
 *
 *   wc_stats_f32        DecorelationNormalization.call, train mode, the transpose + mean +
 *                       centre + f f^T/(M-1) part            (class imported generator.py:9,
 *                       instantiated generator.py:24,26; body in the un-vendored gan/ submodule)
 *   wc_factor_f64       same call: (1-eps)Sigma+eps I, tf.cholesky, tf.matrix_triangular_solve
 *                       against I, and the moving_mean / moving_cov add_update ops; eval mode
 *                       (scorer.py:60,72) takes the moving statistics instead
 *   wc_color_f32        folds the coloring kernels into the whitening matrix:
 *                       Conv2D 1x1 (generator.py:50-51), ConditionalConv11 (generator.py:52-60),
 *                       FactorizedConv11 (generator.py:69-78), CenterScale variants
 *                       (generator.py:28-40)  ->  A_k = W^T Gamma_k
 *   wc_apply_f32        W f, the transpose back, and the 1x1-conv coloring + bias + Add
 *                       (generator.py:83-87 `stack`)            ->  y = (x - mu) A_k + beta_k
 *   wc_bwd_reduce_f32 / wc_bwd_factor_f64 / wc_bwd_apply_f32
 *                       the TF graph gradients of all of the above (training via
 *                       Trainer.train(), run.py:93-94); closed form in SURVEY.md row a10
 *
 * Contract (all entry points):
 *   - return 0 on success, a negative WC_ERR_* on a rejected argument, or a positive
 *     hipError_t from the launch; nothing throws, nothing aborts.
 *   - every pointer is DEVICE memory owned by the caller, including the workspace; the
 *     library allocates nothing and keeps no state between calls.
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and never synchronises
 *     with the host, so calls are graph-capturable and may run concurrently from several
 *     host threads on different streams/buffers.
 *   - x, y, gy, dx are row-major (M, C) float32 with C contiguous: an NHWC tensor viewed
 *     as M = N*H*W rows.  C must be a multiple of 32 with 32 <= C <= 1024 (callers pad
 *     other widths with zero channels, which leaves the real channels' result unchanged).
 *   - matrices are row-major, symmetric ones stored in full.  "slot" is an int32 (N,)
 *     array giving, per SAMPLE, the index into the leading axis of A / bias / gamma
 *     (NULL = every sample uses slot 0); a sample is HW consecutive rows.
 */
#ifndef WC_HIP_H
#define WC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WC_ABI_VERSION 8

#define WC_OK                 0
#define WC_ERR_NULL          -1   /* a required pointer is NULL                     */
#define WC_ERR_SHAPE         -2   /* M/N/HW/Kc not positive, or N*HW overflows       */
#define WC_ERR_CHANNELS      -3   /* C not a multiple of 32 in [32, 1024]            */
#define WC_ERR_WORKSPACE     -4   /* workspace smaller than wc_*_workspace_bytes()   */
#define WC_ERR_ARG           -5   /* eps/momentum/ddof out of range                  */

typedef void* wc_stream_t;        /* hipStream_t */

int         wc_abi_version(void);
const char* wc_error_string(int code);

/* ==== THE BOUNDARY (round 6) ==========================================================================================
 * SURVEY.md section 8b sketches the C ABI a replacement must export as `stats / factor / apply / bwd x 3 / workspace`.  That is this list:
 * ten functions (the seven stages + colouring glue) and their workspace sizers.  A binding that implements only these (INTEGRATION.md
 * section 3, the TF1/Keras-side stub) runs every layer of generator.py:13-90 -- forward, backward, train and eval mode, all colouring
 * variants -- to the parity bar; oracle/wc_cpu.cpp exports each of them with a `_cpu` suffix (the conformance twin SURVEY asks for),
 * and tests/test_abi.py checks both.
 *
 *   wc_stats_f32        K1   raw moments                         DecorelationNormalization.call (generator.py:24, 26)
 *   wc_factor_f64       K2   mu, L = chol((1-eps) Sigma + eps I), W = L^-1, moving statistics
 *   wc_color_f32             A_k = W^T Gamma_k                   Conv2D 1x1 / ConditionalConv11 / FactorizedConv11 (generator.py:49-78)
 *   wc_group_bias_f32        b_k = beta_k - mu A_k (grouped batches)
 *   wc_apply_f32        K3   y = (x - mu) A[slot] + b[slot]       (wc_apply_act_f32: the same with the block's ReLU in the epilogue)
 *   wc_bwd_reduce_f32   K4   R = f^T gy, column sums             autodiff of the above
 *   wc_bwd_factor_f64   K5   the C x C adjoint chain
 *   wc_bwd_apply_f32    K6   dx = [gy | f] [A^T ; S] - mean
 *   wc_*_workspace_bytes     the sizers of the eight above
 *
 * EVERYTHING ELSE in this header is an EXTENSION: a fusion or a data-format route of the same stages that the shipped torch layers take
 * where the shape allows (pre-split fp16 planes, the residual add as producer, bit masks, K1 + K2 in one call, the harness' convolutions
 * and spectral norm).  Each extension's comment names the core sequence it equals, each is parity-tested against that sequence or the
 * oracle, and none is needed for a drop-in: a caller that never heard of them loses speed, not results.  No new extension enters without
 * one leaving (ABI 8 retired nothing and added none).  The list below is what tests/test_abi.py parses. */
#define WC_CORE_API "wc_stats_f32 wc_factor_f64 wc_color_f32 wc_group_bias_f32 wc_apply_f32 wc_apply_act_f32 " \
                    "wc_bwd_reduce_f32 wc_bwd_factor_f64 wc_bwd_apply_f32 " \
                    "wc_stats_workspace_bytes wc_factor_workspace_bytes wc_color_workspace_bytes wc_apply_workspace_bytes " \
                    "wc_bwd_reduce_workspace_bytes wc_bwd_factor_workspace_bytes wc_bwd_apply_workspace_bytes"

/* K1 + K2 in one call (ABI 4): wc_stats_f32 followed by wc_factor_f64(training = 1) for the caller that does not need the moments
 * themselves -- per-replica statistics, the reference's behaviour (sync-WC all-reduces (sum, xtx) between the two and keeps the
 * separate entries).  Same arguments and results as that pair; the K1 tail's slab reduction and the K2 head's bookkeeping run as ONE
 * launch (bit-identical mu, L, W, chan_scale and moving statistics: the same float64 expressions in the same order), sum / xtx are
 * never stored.  M = all rows (groups * rows per group).  DecorelationNormalization.call, generator.py:24. */
size_t wc_whiten_workspace_bytes(int64_t M, int C, int groups);
/* Error words of K2's one-launch form (128 <= C <= 256: the inverse's workgroups wait, with a bounded spin, for the factorising
 * workgroup of the same launch): byte offset into the workspace given to wc_factor_f64 / wc_whiten_f32 of `groups` uint32 words, 64
 * bytes apart, that are 0 after a clean call and 1 when a wait ran out (W then also holds a NaN).  Read them back behind the
 * call (stream order) when the GPU is shared or time-sliced; WC_K2_TWO_LAUNCH=1 selects the form without such a wait.  0: no such
 * launch for this shape (wc_factor_route != 2: other widths, more than 8 groups, WC_K2_TWO_LAUNCH) -- the words are then not written. */
size_t wc_factor_error_offset(int C, int groups);
/* Which launch sequence K2 takes for (C, groups) -- the host's own decision, exported so that tests and tools can assert it instead of
 * restating the gates: 0 = Cholesky + level-doubling inverse (C > 256), 1 = factor with look-ahead + column inverse in two launches
 * (C < 128, more than 8 groups, or WC_K2_TWO_LAUNCH), 2 = factor and inverse in one launch (the only route with error words).
 * -1: the shape is refused (wc_factor_workspace_bytes returns 0). */
int    wc_factor_route(int C, int groups);
size_t wc_whiten_error_offset(int64_t M, int C, int groups);
int    wc_whiten_f32(const float* x, int64_t M, int C, int groups, double eps, double momentum, int ddof,
                     float* moving_mean /*[C] in/out, nullable*/, float* moving_cov /*[C,C] in/out, nullable*/,
                     float* mu /*[groups,C]*/, float* chan_scale /*[C], nullable*/, double* L /*[groups,C,C]*/, double* W /*[groups,C,C]*/,
                     void* ws, size_t ws_bytes, wc_stream_t stream);

/* Bytes of scratch each stage needs for the given problem (16-byte aligned carve inside). */
size_t wc_stats_workspace_bytes(int64_t M, int C, int groups);
size_t wc_factor_workspace_bytes(int C, int groups);
size_t wc_color_workspace_bytes(int C, int Kc);
size_t wc_bwd_reduce_workspace_bytes(int64_t N, int64_t HW, int C, int Kc, int has_slot);
size_t wc_bwd_factor_workspace_bytes(int C, int Kc);
size_t wc_apply_workspace_bytes(int64_t N, int64_t HW, int C, int Kc);
size_t wc_apply_plan_bytes(int C, int Kc);
size_t wc_bwd_apply_workspace_bytes(int64_t N, int64_t HW, int C, int Kc);

/* K1: raw additive moments of the rows of x:  sum[c] = sum_m x[m,c],  xtx = x^T x  (float64).
 * These are what a sync-WC data-parallel run all-reduces before wc_factor_f64.
 * groups > 1: the M rows are `groups` independent batches of M/groups consecutive rows, each with its own
 * statistics (sum [groups,C], xtx [groups,C,C]) -- several forward passes of the same layer in one call. */
int wc_stats_f32(const float* x, int64_t M, int C, int groups,
                 double* sum /*[groups,C]*/, double* xtx /*[groups,C,C]*/,
                 void* ws, size_t ws_bytes, wc_stream_t stream);

/* K2: moments -> mu, Sigma; T = (1-eps)Sigma + eps I; L = chol(T); W = L^-1 (float64).
 * training != 0: statistics come from (sum, xtx, M); if moving_mean/moving_cov are non-NULL they
 *                are updated in place, moving <- momentum*moving + (1-momentum)*batch (un-shrunk Sigma).
 * training == 0: mu = moving_mean, Sigma = moving_cov (sum/xtx ignored, may be NULL).
 * groups > 1: mu [groups,C], L/W [groups,C,C]; the moving statistics receive the groups' updates one after the
 * other (as separate calls would); chan_scale stays [C] (the largest variance over the groups decides). */
int wc_factor_f64(const double* sum, const double* xtx, int64_t M /*rows per group*/, int C, int groups,
                  double eps, double momentum, int ddof, int training,
                  float* moving_mean /*[C]*/, float* moving_cov /*[C*C]*/,
                  float* mu /*[C] out*/, float* chan_scale /*[C] out, nullable: power-of-two 1/sigma for the fp16 path*/,
                  double* L /*[C*C] out*/, double* W /*[C*C] out*/,
                  void* ws, size_t ws_bytes, wc_stream_t stream);

/* A_k = W^T Gamma_k for k < Kc (float32 out), and its transpose At_k = A_k^T (what the backward
 * apply multiplies by; At may be NULL).  gamma == NULL means Gamma = I (whitening only, Kc = 1).
 * With chan_scale (from wc_factor_f64) and a buffer of wc_apply_plan_bytes(C, Kc) it also prepares the
 * "plan" of A -- split-fp16 tables of the fast apply -- so that wc_apply_f32 is a single kernel launch. */
/* per_group != 0: gamma holds groups*Kc tables and group g takes its own run, A[g*Kc+k] = W_g^T Gamma[g*Kc+k]
 * (per-SAMPLE coloring tables of a grouped batch: ConditionalConv11 / FactorizedConv11 with more classes than
 * samples, generator.py:52-60,69-78 at run.py:172-173's 200 / 1000 classes); 0: every group takes the same Kc tables. */
int wc_color_f32(const double* W /*[groups,C,C]*/, const float* gamma /*[Kc,C,C] ([groups*Kc,C,C] if per_group) or NULL*/,
                 int Kc, int C, int groups, int per_group,
                 float* A /*[groups*Kc,C,C] out, index g*Kc+k*/, float* At /*same shape, nullable*/,
                 const float* chan_scale /*[C], nullable*/, void* plan /*out, nullable*/,
                 void* ws, size_t ws_bytes, wc_stream_t stream);

/* Grouped forward glue: center[c] = mean_g mu[g,c] and bias[g*Kc+k] = beta[k] - (mu[g] - center) A[g*Kc+k], so that
 * wc_apply_f32(x, center, A, bias, slot = g*Kc + k) equals (x - mu_g) A[g*Kc+k] + beta[k] for every group.
 * per_group != 0: beta is [groups*Kc,C] and slot g*Kc+k takes beta[g*Kc+k] (see wc_color_f32). */
int wc_group_bias_f32(const float* mu /*[groups,C]*/, const float* A /*[groups*Kc,C,C]*/,
                      const float* beta /*[Kc,C] ([groups*Kc,C] if per_group), nullable*/,
                      int groups, int Kc, int C, int per_group, float* center /*[C] out*/, float* bias /*[groups*Kc,C] out*/,
                      wc_stream_t stream);

/* K3: y[n] = (x[n] - mu) A[slot[n]] + bias[slot[n]]   (bias NULL = 0; mu NULL = 0).
 * With a workspace of wc_apply_workspace_bytes() the split-fp16 MFMA fast path runs when the shape allows
 * (C in {32,64,128,256}, N*HW >= 1024 and a multiple of 16384/C rows); ws == NULL (and no plan) always takes the
 * exact f32-MFMA kernel.  Both give fp32-GEMM accuracy; a row tile holding an element outside the fp16 range -- or,
 * with slot != NULL and HW not a multiple of the 8192/C-row tile, a tile that straddles samples of different slots --
 * is detected on the device and recomputed in fp32 by the same kernel. */
int wc_apply_f32(const float* x, const float* mu, const float* A, const float* bias,
                 const int32_t* slot, int64_t N, int64_t HW, int C, int Kc,
                 float* y, const void* plan /*from wc_color_f32, nullable*/,
                 void* ws, size_t ws_bytes, wc_stream_t stream);

/* K3 with the activation that follows every WC site of the generator folded into the epilogue (SURVEY.md section 8f
 * row N2; generator.py:144-151, 154: `Activation('relu')` after each norm stack): relu = 1 writes max(y, 0) (NaN stays
 * NaN), relu = 0 is wc_apply_f32.  The gradient of the pair is the caller's mask (gy where y > 0, else 0) in front of
 * the unchanged backward. */
int wc_apply_act_f32(const float* x, const float* mu, const float* A, const float* bias,
                     const int32_t* slot, int64_t N, int64_t HW, int C, int Kc, int relu,
                     float* y, const void* plan /*from wc_color_f32, nullable*/,
                     void* ws, size_t ws_bytes, wc_stream_t stream);

/* ---- Pre-split activations (ABI 4, additive) -------------------------------------------------------------------------
 * The fp16 MFMA paths of this library compute with x = hi + lo (two fp16 terms, three products).  A tensor that several
 * stages read (K1, K3, K4, K6 all read the site's input x: generator.py:83-87 `stack` and its gradient) is converted by
 * each of them; the PRODUCER can hand it over already split instead -- the same 4 bytes per element:
 *     x[m][c] ~= center[c] + (hi[m][c] + lo[m][c]) / scale[c],   hi = fp16(g), lo = fp16(g - hi), g = (x - center) scale
 * `xs` = 2*M*C halves: the hi plane [M][C], then the lo plane [M][C].  scale[c]: a power of two that puts the channel's
 * sampled maximum into [8, 16] (>= 3700 x of headroom below fp16's range); center[c]: any value near the channel mean
 * (NULL = 0).  wc_split_f32 (the stand-in producer of tests and benches: scales given by the caller) clamps an element beyond +-60000
 * after scaling and sets *flag (device int, nullable) to 1; the producer the layers use, wc_resadd_split_f32, never clamps (below). */
size_t wc_split_bytes(int64_t M, int C);
/* int32 words of the producer's `flag` area (ABI 7): [0] status, [64, 64 + C) per-channel maxima, [64 + C, 64 + 2C) the sampled scales */
#define WC_SPLIT_FLAG_WORDS (64 + 2 * 1024)
/* center, scale from <= 256 sampled rows of x (outlier-proof, as K1's own shift / scales); zeroes flag[0..63]. */
int wc_split_scales_f32(const float* x, int64_t M, int C, float* center /*[C] out*/, float* scale /*[C] out*/,
                        int* flag /*[64] out: zeroed*/, wc_stream_t stream);
/* x (M, C) fp32 -> xs; relu != 0 clamps at zero first (NaN stays NaN). */
int wc_split_f32(const float* x, const float* center /*nullable*/, const float* scale, int64_t M, int C, int relu,
                 void* xs /*out*/, int* flag /*nullable*/, wc_stream_t stream);
int wc_unsplit_f32(const void* xs, const float* center /*nullable*/, const float* scale, int64_t M, int C, float* x /*out*/,
                   wc_stream_t stream);

/* K1 on a pre-split input: the raw moments of wc_stats_f32 (same outputs, same meaning of `groups`) of the tensor the planes
 * stand for.  No conversion in the kernel: LDS-DMA staging, transposing LDS reads (ds_read_b64_tr_b16) for the [channel][row]
 * MFMA operands.  C in {128, 256}, rows per group a multiple of 64 and N*HW >= 16384 (wc_stats_split_supported; WC_ERR_SHAPE
 * otherwise: convert with wc_unsplit_f32 and call wc_stats_f32).  Replaces the same reference call site as wc_stats_f32. */
int    wc_stats_split_supported(int64_t M, int C, int groups);
size_t wc_stats_split_workspace_bytes(int64_t M, int C, int groups);
int wc_stats_split_f16x2(const void* xs, const float* xs_center, const float* xs_scale, int64_t M, int C, int groups,
                         double* sum /*[groups,C]*/, double* xtx /*[groups,C,C]*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* K3 on a pre-split input:  y[n] = (x[n] - mu) A[slot[n]] + bias[slot[n]]  with x given as (xs, xs_center, xs_scale).
 * The staging is pure LDS-DMA into the fp16 image the MFMAs read (no conversion in the kernel).  `plan` = the tables
 * wc_color_f32 builds when it is given chan_scale = xs_scale (NULL: built here, in ws).  C in {128, 256} and N*HW a multiple
 * of 8192/C rows (wc_apply_split_supported; WC_ERR_SHAPE otherwise: convert with wc_unsplit_f32 and call wc_apply_f32).
 * relu as in wc_apply_act_f32.  Replaces the same reference call site as wc_apply_f32 (generator.py:83-87). */
/* bias_eff[k] = bias[k] + (xs_center - mu) A[k]  ([Kc, C]; bias, xs_center, mu nullable = 0): the additive term of the split
 * apply.  A caller that passes bias = bias_eff with mu = xs_center = NULL to wc_apply_split_f16x2 gets a single launch. */
int    wc_split_bias_f32(const float* A /*[Kc,C,C]*/, const float* bias, const float* xs_center, const float* mu, int Kc, int C,
                         float* bias_eff /*[Kc,C] out*/, wc_stream_t stream);
int    wc_apply_split_supported(int64_t N, int64_t HW, int C);
size_t wc_apply_split_workspace_bytes(int C, int Kc);
int wc_apply_split_f16x2(const void* xs, const float* xs_center /*nullable*/, const float* xs_scale,
                         const float* mu /*nullable*/, const float* A, const float* bias /*nullable*/,
                         const int32_t* slot, int64_t N, int64_t HW, int C, int Kc, int relu,
                         float* y, const void* plan /*nullable*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* ---- The residual add as the producer of pre-split activations (ABI 5, additive; SURVEY.md section 8f row N2: "residual Add
 * feeding K1") ---------------------------------------------------------------------------------------------------------------
 * reference generator.py:142-146: every `resblock(...)` ends in the Add of its convolution path h and its shortcut s, and the sum
 * is what the next block's first norm stack and Generator.BN.Final (generator.py:154) read.  With up = 1 the shortcut is given
 * BEFORE the nearest-neighbour upsample (a 1x1 convolution commutes with it) and every 2x2 output patch adds its source pixel:
 *     out[n][y][x][c] = h[n][y][x][c] + s[n][y >> up][x >> up][c]      h (N, H, W, C), s (N, H >> up, W >> up, C) or NULL (= 0)
 * wc_resadd_f32 writes the fp32 sum.  wc_resadd_split_f32 writes the sum in the pre-split format above instead (xs, center,
 * scale, flag: exactly what wc_split_scales_f32 + wc_split_f32 make of the fp32 sum -- the same <= 256 sampled rows, the same
 * centre and scales) in ONE pass over h and s behind one small sampling launch, so that K1 / K3 of the next site
 * (wc_whiten_split_f16x2, wc_apply_split_ex_f16x2) and the next block's shortcut convolution (wc_fold_channel_scale_f32 +
 * wc_conv_f16x3 on the same planes) read it without a conversion; x32 (nullable) also receives the fp32 sum, for a reader without
 * a planes path.  C in {128, 256} (wc_resadd_split_supported), N*H*W < 2^31.
 * ABI 7: NOTHING SATURATES.  A sampled scale can be too tight (a channel nearly constant on the sampled rows that spikes elsewhere);
 * the pass then records the true maximum of every channel that met an element beyond +-60000 and a second, gated launch (it leaves
 * at once otherwise; no host synchronisation, graph-capturable) rewrites the planes with those channels' scales lowered to fit, and
 * scale[] with them -- every consumer reads scale[] from device memory behind this call, so K1, K3, the shortcut convolution and
 * the backward see a consistent, exact tensor.  flag[0] = 1 afterwards says that this happened (informational).  A non-finite
 * element stays non-finite in the planes.  `flag`: WC_SPLIT_FLAG_WORDS int32 words, all scratch but [0].
 * wc_patch_sum_f32: the gradient of the up = 1 form with respect to s: out[n][y][x] = the sum of g over the 2x2 patch. */
int wc_resadd_split_supported(int64_t N, int64_t H, int64_t W, int C);
int wc_resadd_f32(const float* h, const float* s /*nullable*/, int64_t N, int64_t H, int64_t W, int C, int up, float* out,
                  wc_stream_t stream);
int wc_resadd_split_f32(const float* h, const float* s /*nullable*/, int64_t N, int64_t H, int64_t W, int C, int up,
                        void* xs /*out: 2*N*H*W*C halves*/, float* center /*[C] out*/, float* scale /*[C] out*/,
                        int* flag /*[WC_SPLIT_FLAG_WORDS] out: [0] = 1 when the gated rescaling pass ran*/, float* x32 /*out, nullable*/,
                        wc_stream_t stream);
int wc_patch_sum_f32(const float* g /*(N, 2 Hs, 2 Ws, C)*/, int64_t N, int64_t Hs, int64_t Ws, int C, float* out /*(N, Hs, Ws, C)*/,
                     wc_stream_t stream);
/* The producer FEEDING K1 (ABI 7): wc_resadd_split_f32 whose pass also accumulates the next site's covariance
 * moments -- the rows are summed, centred, scaled and split once, the words go to the planes AND, transposed, through the LDS into the
 * block triangle of X^T X on the matrix pipe (the covariance kernel of wc_stats_f32's fast path with the add in front and the planes'
 * stores behind its conversion), so the next site's K1 pass over the tensor (wc_stats_split_f16x2's kernel: 134 MB re-read at
 * 128x32x32x256) does not exist.  xs / center / scale / flag / x32: exactly wc_resadd_split_f32's outputs (bit for bit, gated rescaling
 * pass included -- it then redoes the partials as well).  `groups`: the statistic groups of the CONSUMING site (runs of N/groups
 * samples; slabs never cross them).  ws (wc_resadd_stats_workspace_bytes) receives the per-slab partials; it is what
 * wc_whiten_presummed_f16x2 (K1 tail + K2: = wc_whiten_split_f16x2 without its pass) or wc_stats_presummed_f16x2 (the raw moments, for
 * sync-WC's all-reduce: = wc_stats_split_f16x2 without its pass) take -- same M, C, groups, the same buffer.
 * wc_resadd_stats_supported: C in {128, 256}, up = 1 (every block of the shipped generators), W % 8 == 0, N*H*W/groups >= 20480 rows
 * in whole stages (64 rows at C = 256, 128 at C = 128); elsewhere WC_ERR_SHAPE: wc_resadd_split_f32 + wc_whiten_split_f16x2.
 * Replaces: the Add that ends `resblock` (generator.py:142-146) + the moments part of DecorelationNormalization.call (generator.py:24). */
int    wc_resadd_stats_supported(int64_t N, int64_t H, int64_t W, int C, int up, int groups);
size_t wc_resadd_stats_workspace_bytes(int64_t N, int64_t H, int64_t W, int C, int groups);
int    wc_resadd_stats_split_f32(const float* h, const float* s /*required*/, int64_t N, int64_t H, int64_t W, int C, int up, int groups,
                                 void* xs /*out*/, float* center /*[C] out*/, float* scale /*[C] out*/, int* flag /*[WC_SPLIT_FLAG_WORDS]*/,
                                 float* x32 /*out, nullable*/, void* ws /*out: the partials*/, size_t ws_bytes, wc_stream_t stream);
size_t wc_whiten_presummed_error_offset(int64_t M, int C, int groups);
int    wc_whiten_presummed_f16x2(const float* xs_center, int64_t M, int C, int groups, double eps, double momentum, int ddof,
                                 float* moving_mean /*nullable*/, float* moving_cov /*nullable*/, float* mu /*[groups,C]*/,
                                 double* L /*[groups,C,C]*/, double* W /*[groups,C,C]*/, void* ws /*from wc_resadd_stats_split_f32*/,
                                 size_t ws_bytes, wc_stream_t stream);
int    wc_stats_presummed_f16x2(const float* xs_center, int64_t M, int C, int groups, double* sum /*[groups,C]*/,
                                double* xtx /*[groups,C,C]*/, void* ws /*from wc_resadd_stats_split_f32*/, size_t ws_bytes, wc_stream_t stream);
/* A 1x1 convolution (the block's shortcut, generator.py:142-146) on a pre-split input: with x[c] = center[c] + g[c] / scale[c],
 *     sum_c x[c] w[o][c] + b[o] = sum_c g[c] wf[o][c] + bf[o],   wf[o][c] = w[o][c] / scale[c],  bf[o] = b[o] + <center, w[o]>
 * so wc_conv_f16x3 runs on the planes themselves (x scale 1) with the folded weight and bias; its weight gradient D (of wf, from
 * wc_conv_wrw_bias_f16x3 on the same planes) and bias gradient db unfold to dW[o][c] = D[o][c] / scale[c] + center[c] db[o].
 * w / wf / D / dW: element (o, c) at o * stride_o + c * stride_c. */
int wc_fold_channel_scale_f32(const float* w, int64_t stride_o, int64_t stride_c, int Cout, int Cin, const float* bias /*nullable*/,
                              const float* scale, const float* center, float* wf /*out*/, float* bf /*[Cout] out*/, wc_stream_t stream);
int wc_unfold_channel_scale_f32(const float* D, const float* db, int64_t stride_o, int64_t stride_c, int Cout, int Cin,
                                const float* scale, const float* center, float* dW /*out*/, wc_stream_t stream);

/* K1 + K2 on a pre-split input in one call (ABI 5): wc_stats_split_f16x2 + wc_factor_f64(training = 1) as wc_whiten_f32 is for the
 * fp32 input -- same results as that pair, the K1 tail and the K2 head as one launch, the moments never stored.  No chan_scale
 * output: the apply's input scales are the planes' own (pass xs_scale to wc_color_f32).  DecorelationNormalization.call,
 * generator.py:24. */
size_t wc_whiten_split_workspace_bytes(int64_t M, int C, int groups);
size_t wc_whiten_split_error_offset(int64_t M, int C, int groups);
int    wc_whiten_split_f16x2(const void* xs, const float* xs_center, const float* xs_scale, int64_t M, int C, int groups,
                             double eps, double momentum, int ddof, float* moving_mean /*nullable*/, float* moving_cov /*nullable*/,
                             float* mu /*[groups,C]*/, double* L /*[groups,C,C]*/, double* W /*[groups,C,C]*/,
                             void* ws, size_t ws_bytes, wc_stream_t stream);

/* The planes route's glue (ABI 5).  wc_color_split_f32: wc_color_f32 (one statistic group) for a site whose input is pre-split -- A, At,
 * the apply's tables for the PLANES' scales, and in the same launch bias_eff[k] = beta[k] + (xs_center - mu) A[k], the additive term
 * wc_apply_split_ex_f16x2 takes as `bias` with mu = xs_center = NULL (wc_split_bias_f32 as a launch of its own cost the forward site
 * 5 us).  C in {32, 64, 128, 256}.  wc_group_bias_centered_f32: wc_group_bias_f32 with the common centre GIVEN (the planes' centre):
 * bias[g*Kc+k] = beta[k] - (mu[g] - center) A[g*Kc+k] is then the grouped planes route's additive term directly.
 * Replace the same reference call sites as wc_color_f32 / wc_group_bias_f32 (generator.py:28-80 coloring layers folded into W). */
int wc_color_split_f32(const double* W /*[C,C]*/, const float* gamma /*[Kc,C,C] or NULL*/, int Kc, int C, float* A /*[Kc,C,C] out*/,
                       float* At /*nullable*/, const float* xs_scale, const float* xs_center, const float* mu /*[C]*/,
                       const float* beta /*[Kc,C], nullable*/, void* plan /*out: wc_apply_plan_bytes(C, Kc)*/, float* bias_eff /*[Kc,C] out*/,
                       void* ws, size_t ws_bytes, wc_stream_t stream);
int wc_group_bias_centered_f32(const float* mu /*[groups,C]*/, const float* A /*[groups*Kc,C,C]*/, const float* beta /*nullable*/,
                               const float* center /*[C] in*/, int groups, int Kc, int C, int per_group, float* bias /*[groups*Kc,C] out*/,
                               wc_stream_t stream);

/* The dictionary mix of the soft-assignment coloring "cWC_sa" (ABI 6):
 *     out[t] = base + sum_{e < E} alpha[idx[t], e] * dict[e],   t = 0 .. Kc-1   (C x C each)
 * dict (E, C, C): the filter dictionary, alpha (K, E): the per-class coefficients, idx (Kc) int32: the class of table t (NULL: t itself,
 * then Kc must equal K), base (C, C): the unconditional 1x1 kernel the reference adds (NULL: none).  Only the Kc tables the batch uses
 * are formed (K = 200 / 1000 classes at batch 64: run.py:172-173).  E <= 32, C a multiple of 4 (wc_factor_mix_supported).
 * wc_factor_mix_bwd_f32: from dout (Kc, C, C) -> ddict (E, C, C), dalpha (K, E; written whole, zero for absent classes), dbase (C, C); each
 * nullable; dalpha needs wc_factor_mix_bwd_workspace_bytes(E, Kc) of workspace.  Deterministic (fixed summation order).
 * Replace: generator.py:69-78 -- FactorizedConv11(number_of_classes, filters, filters_emb, use_bias=False)([x, cls]) + Conv2D 1x1 -> Add,
 * i.e. the (N, E) x (E, C^2) mix + gather of the (missing) gan.conditional_layers.FactorizedConv11 and TF's gradients of it. */
int    wc_factor_mix_supported(int E, int C);
int    wc_factor_mix_f32(const float* dict, const float* alpha, const int32_t* idx /*nullable*/, const float* base /*nullable*/,
                         int E, int C, int K, int Kc, float* out /*[Kc,C,C]*/, wc_stream_t stream);
size_t wc_factor_mix_bwd_workspace_bytes(int E, int Kc);
int    wc_factor_mix_bwd_f32(const float* dict, const float* alpha, const int32_t* idx /*nullable*/, const float* dout /*[Kc,C,C]*/,
                             int E, int C, int K, int Kc, float* ddict /*nullable*/, float* dalpha /*nullable*/, float* dbase /*nullable*/,
                             void* ws, size_t ws_bytes, wc_stream_t stream);

/* K3 on a pre-split input with the epilogues the generator's sites use (ABI 5): as wc_apply_split_f16x2, and
 *   relu_mask (nullable; relu = 1, N*HW a multiple of 32): the ReLU's one-bit gradient mask, as wc_apply_mask_f32 leaves it;
 *   planes + oscale instead of y (exactly one of y / planes is given): the output as the next convolution's fp16 planes,
 *   oscale the record wc_out_scale_f32 filled -- the protocol of wc_apply_planes_f32 (two launches: the pass and its gate).
 * Replaces the same reference call site as wc_apply_f32 (generator.py:83-87) + Activation('relu') (generator.py:144-151, 154). */
int wc_apply_split_ex_f16x2(const void* xs, const float* xs_center /*nullable*/, const float* xs_scale,
                            const float* mu /*nullable*/, const float* A, const float* bias /*nullable*/,
                            const int32_t* slot, int64_t N, int64_t HW, int C, int Kc, int relu,
                            float* y /*nullable*/, void* relu_mask /*out, nullable*/, void* planes /*out, nullable*/, float* oscale,
                            const void* plan /*nullable*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* K3 + ReLU + the ReLU's gradient mask as ONE BIT per element (ABI 4).  As wc_apply_act_f32 with relu = 1, and
 * relu_mask (wc_relu_mask_bytes(N*HW, C) bytes; N*HW a multiple of 32) receives, for every 32-row block t and channel c, the word
 * mask[t * C + c] whose bit b says "y[32 t + b][c] passed the ReLU" (y > 0, or NaN).  The planned fast kernel writes the words
 * from its epilogue (32 vector instructions and one 128-byte store per 32 x 32 outputs); every other path takes one pass over
 * y.  The backward then needs neither y nor a masked copy of the gradient to know the mask: wc_bwd_reduce_mask_f32.
 * (generator.py:144-151, 154: `Activation('relu')` behind every norm stack.) */
size_t wc_relu_mask_bytes(int64_t M, int C);
/* out = gy where the mask's bit is set, else 0 (the elementwise form of the ReLU gradient; wc_bwd_reduce_mask_f32 does the same
 * while it stages gy).  M a multiple of 32, C a multiple of 32 in [32, 1024]. */
int wc_relu_mask_apply_f32(const float* gy, const void* relu_mask, int64_t M, int C, float* out, wc_stream_t stream);
int wc_apply_mask_f32(const float* x, const float* mu, const float* A, const float* bias,
                      const int32_t* slot, int64_t N, int64_t HW, int C, int Kc,
                      float* y, void* relu_mask /*out*/, const void* plan /*from wc_color_f32, nullable*/,
                      void* ws, size_t ws_bytes, wc_stream_t stream);

/* K3 -> convolution hand-off (ABI 4).  Every WC site of the generator is followed by
 * ReLU and a convolution (generator.py:144-151), and this build's convolution (wc_conv_f16x3) reads its input as two fp16 planes
 * hi | lo of s * y with ONE power-of-two scale s: wc_apply_planes_f32 is wc_apply_act_f32 whose output leaves in that form -- no
 * fp32 y, and no wc_conv_split_f32 (one pass for max |y|, one to split) in front of the convolution.
 *   planes  (out) 2 * N*HW*C fp16: hi plane, then lo plane;  y ~= (hi + lo) / oscale[0]
 *   oscale  float[wc_apply_planes_scale_floats()], the scale record: wc_out_scale_f32 fills its input part from the coloring
 *           parameters alone, no pass over data (a whitened activation has unit covariance, so channel c of table k has standard
 *           deviation |Gamma_k[:, c]|: [1] = K as an int, [2 + k] = max_c (|beta_k[c]| + 16 |Gamma_k[:, c]|), K <= 1024; the
 *           kernel puts the largest bound into [2^13, 2^14), the convolution's own target for max |y|).  A caller with a better
 *           bound writes [1] = 1 (int) and [2] = the bound.  [0] (out) = the scale the planes were written with -- the device
 *           scalar wc_conv_f16x3 takes.  The rest is scratch (per-workgroup maxima).
 *   Two launches of the same kernel: the pass, and a gated one that leaves at once unless an element of s * y left fp16's range
 *   (beyond ~64 sigma), in which case it redoes the pass with the scale the measured maximum asks for.  No host synchronisation.
 *   relu_mask (nullable, relu = 1): as in wc_apply_mask_f32.  plan: required (wc_color_f32).
 * wc_apply_planes_supported: C in {128, 256}, N*HW a multiple of 8192/C rows and of 32; otherwise WC_ERR_SHAPE -- call
 * wc_apply_act_f32 and let the convolution split its input. */
int    wc_apply_planes_supported(int64_t N, int64_t HW, int C);
size_t wc_apply_planes_scale_floats(void);
int    wc_out_scale_f32(const float* gamma /*[K,C,C], nullable = identity*/, const float* beta /*[K,C], nullable*/, int K, int C,
                        float* oscale, wc_stream_t stream);
int    wc_apply_planes_f32(const float* x, const float* mu, const float* A, const float* bias, const int32_t* slot,
                           int64_t N, int64_t HW, int C, int Kc, int relu, void* planes /*out*/, float* oscale,
                           void* relu_mask /*out, nullable*/, const void* plan, wc_stream_t stream);

/* K4: R[k] = sum_{n: slot[n]=k} (x[n]-mu)^T gy[n]  (Kc,C,C),  gsum[k] = sum_{n in k} rows of gy[n]  (Kc,C). */
int wc_bwd_reduce_f32(const float* x, const float* mu, const float* gy, const int32_t* slot,
                      int64_t N, int64_t HW, int C, int Kc,
                      double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/,
                      void* ws, size_t ws_bytes, wc_stream_t stream);

/* K4 / K6 sharing the fp16 paths' per-channel input scales (ABI 3).  Both stages scale (x - mu) and gy by per-channel powers
 * of two sampled from <= 256 rows; K4 samples them anyway.  `scales` = float[2*C]: the scales of (x - mu), then those of gy.
 * wc_bwd_reduce_scaled_f32 writes them (also when its own reduction takes the exact path); wc_bwd_apply_scaled_f32 takes them
 * instead of sampling the same two tensors again and builds the tables of both its passes in one launch: three launches
 * instead of six.  scales == NULL: exactly wc_bwd_reduce_f32 / wc_bwd_apply_f32.  Results are identical either way (the same
 * samples give the same scales). */
int wc_bwd_reduce_scaled_f32(const float* x, const float* mu, const float* gy, const int32_t* slot,
                             int64_t N, int64_t HW, int C, int Kc,
                             double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/, float* scales_out /*[2C], nullable*/,
                             void* ws, size_t ws_bytes, wc_stream_t stream);
/* K4 behind a site whose ReLU rode in K3's epilogue (wc_apply_act_f32, relu = 1): the activation's gradient mask
 * gy := gy unless y <= 0 (a NaN in y lets the gradient through, as aten::threshold_backward does; generator.py:144-154
 * `Activation('relu')` after each norm stack) applied while K4 stages gy,
 * instead of an elementwise pass over three tensors in front of it.  relu_y = the site's output y; gy_masked (out, same
 * shape as gy, must not alias it) receives the masked gradient -- what K6 then takes as its gy.  R, gsum, scales_out as in
 * wc_bwd_reduce_scaled_f32, computed from the masked gradient.  relu_y == NULL (then gy_masked must be NULL too) is that
 * function.  Shapes whose reduction kernel does not mask in its staging take one elementwise pass inside the call. */
int wc_bwd_reduce_relu_f32(const float* x, const float* mu, const float* gy, const float* relu_y /*nullable*/, const int32_t* slot,
                           int64_t N, int64_t HW, int C, int Kc,
                           double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/, float* gy_masked /*[N*HW*C] out, nullable*/,
                           float* scales_out /*[2C], nullable*/, void* ws, size_t ws_bytes, wc_stream_t stream);
/* The same with the mask in wc_apply_mask_f32's one-bit form: K4 reads x, gy and 1/32 of a tensor where wc_bwd_reduce_relu_f32
 * reads three tensors (the quadrant kernel at C = 256 masks while it stages: one 16-byte load of mask words per thread and
 * 64-row stage; other shapes take one elementwise pass inside the call).  gy_masked as above (required). */
int wc_bwd_reduce_mask_f32(const float* x, const float* mu, const float* gy, const void* relu_mask, const int32_t* slot,
                           int64_t N, int64_t HW, int C, int Kc,
                           double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/, float* gy_masked /*[N*HW*C] out*/,
                           float* scales_out /*[2C], nullable*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* The ReLU'd backward with NO masked copy of the gradient in between (ABI 4): K4 applies the one-bit mask while it stages gy and
 * writes nothing back (wc_bwd_reduce_bits_f32: x, gy and M*C/8 bytes of mask in, R / gsum / scales out), K6 applies the same bits
 * while it converts gy (wc_bwd_apply_bits_f32: gy here is the gradient BEFORE the ReLU, as K4 received it).  The backward site then
 * moves 5.03 M*C*4 bytes instead of 7 (fp32 y, masked copy) -- VERDICT r2 item 3.  Only where both kernels carry the mask in their
 * staging (wc_bwd_bits_supported: C = 256, the fast reduction and the one-pass K6, N*HW a multiple of 32; `scales` required);
 * elsewhere WC_ERR_SHAPE: use wc_bwd_reduce_mask_f32 (which writes the masked gradient) + wc_bwd_apply_scaled_f32.
 * Arguments otherwise as in wc_bwd_reduce_scaled_f32 / wc_bwd_apply_scaled_f32.  generator.py:144-151, 154. */
int wc_bwd_bits_supported(int64_t N, int64_t HW, int C, int has_slot);
int wc_bwd_reduce_bits_f32(const float* x, const float* mu, const float* gy, const void* relu_mask, const int32_t* slot,
                           int64_t N, int64_t HW, int C, int Kc, double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/,
                           float* scales_out /*[2C]*/, void* ws, size_t ws_bytes, wc_stream_t stream);
int wc_bwd_apply_bits_f32(const float* gy, const void* relu_mask, const float* x, const float* mu, const float* At, const float* S,
                          const float* gmean, const int32_t* slot, int64_t N, int64_t HW, int C, int Kc,
                          const float* scales /*[2C] from wc_bwd_reduce_bits_f32*/, float* dx, void* ws, size_t ws_bytes, wc_stream_t stream);
int wc_bwd_apply_scaled_f32(const float* gy, const float* x, const float* mu, const float* At,
                            const float* S, const float* gmean, const int32_t* slot,
                            int64_t N, int64_t HW, int C, int Kc, const float* scales /*[2C], nullable*/, float* dx,
                            void* ws, size_t ws_bytes, wc_stream_t stream);

/* K4 / K6 of a site whose input exists as pre-split planes (ABI 5): the backward reads x from the planes the residual add wrote for the
 * forward (wc_resadd_split_f32) -- no fp32 copy of x has to exist.  K4: the X threads take 8 bytes per plane and row and build the
 * transposed fp16 image with one byte-permute per word (no centre / scale / split instructions); K6: a chunk of x is [hi row | lo row]
 * and its conversion a copy.  (x - mu) = g / scale + (center - mu): K4 adds the rank-one term (center - mu) (sum gy)^T to R, K6 folds
 * (center - mu) S into gmean.  relu_mask (nullable): the site's one-bit ReLU mask, applied by both as in wc_bwd_reduce_bits_f32 /
 * wc_bwd_apply_bits_f32 (gy is then the gradient BEFORE the ReLU).  scales: float[2C]; K4 writes gy's scales to [C, 2C) and K6 reads
 * them there ([0, C) is unused: x's scales are xs_scale).  wc_bwd_xsplit_supported: C = 256 (the fast reduction and the one-pass K6) or, since ABI 7, C = 128 (the plain two-operand
 * reduction staging x from the planes; K6 as the planes kernel for (x - mu) S - sub followed by the accumulating fp32 kernel for + gy At; relu_mask must be
 * NULL there: mask gy in front; with a slot table HW must be a multiple of 128 -- the accumulating kernel takes one table per 128-row tile),
 * N*HW a multiple of 32; elsewhere WC_ERR_SHAPE (keep an fp32 x: wc_resadd_split_f32's x32).  Replace the same TF graph gradients as
 * wc_bwd_reduce_f32 / wc_bwd_apply_f32 (run.py:93-94). */
int    wc_bwd_xsplit_supported(int64_t N, int64_t HW, int C, int has_slot);
int    wc_bwd_reduce_xsplit_f32(const void* xs, const float* xs_center, const float* xs_scale, const float* mu, const float* gy,
                                const void* relu_mask /*nullable*/, const int32_t* slot, int64_t N, int64_t HW, int C, int Kc,
                                double* R /*[Kc,C,C]*/, double* gsum /*[Kc,C]*/, float* scales_out /*[2C]*/,
                                void* ws /*wc_bwd_reduce_workspace_bytes*/, size_t ws_bytes, wc_stream_t stream);
size_t wc_bwd_apply_xsplit_workspace_bytes(int C, int Kc);
int    wc_bwd_apply_xsplit_f32(const float* gy, const void* relu_mask /*nullable*/, const void* xs, const float* xs_center,
                               const float* xs_scale, const float* mu, const float* At, const float* S, const float* gmean,
                               const int32_t* slot, int64_t N, int64_t HW, int C, int Kc, const float* scales /*[2C] from the K4 above*/,
                               float* dx, void* ws, size_t ws_bytes, wc_stream_t stream);

/* K5: dgamma[k] = W R[k];  and, when training != 0, the statistics path
 *     Wbar = sum_k Gamma_k R_k^T;  Lbar = -tril(W^T Wbar W^T);  P = Phi(L^T Lbar)  [computed as -Phi(Wbar W^T): L^T W^T = I and
 *     the strictly upper part of W^T Wbar W^T never reaches Phi's triangle -- one product instead of three; L itself is not read];
 *     S = 2(1-eps)/(M-ddof) sym(W^T P W)  (float32, C x C);   gmean = (1/M) sum_k gsum_k A_k^T  (C).
 * gamma == NULL means Gamma = I.  dgamma / dbeta may be NULL (that output is skipped).  S and gmean are
 * untouched when training == 0. */
int wc_bwd_factor_f64(const double* R, const double* gsum, const double* W, const double* L,
                      const float* gamma, const float* A, int Kc, int C, int64_t M,
                      double eps, int ddof, int training,
                      float* dgamma /*[Kc,C,C]*/, float* dbeta /*[Kc,C]*/,
                      float* S /*[C,C]*/, float* gmean /*[C]*/,
                      void* ws, size_t ws_bytes, wc_stream_t stream);

/* K6: dx[n] = gy[n] At[slot[n]] + (x[n]-mu) S - gmean     (S, gmean NULL in eval mode: dx = gy A^T).
 * At[k] = A[k]^T as written by wc_color_f32. */
int wc_bwd_apply_f32(const float* gy, const float* x, const float* mu, const float* At,
                     const float* S, const float* gmean, const int32_t* slot,
                     int64_t N, int64_t HW, int C, int Kc, float* dx,
                     void* ws, size_t ws_bytes, wc_stream_t stream);

/* N3: spectral normalisation of a weight matrix W (rows, cols) row-major -- SNConv2D / SNDense /
 * SNEmbeding at discriminator.py:26-33, generator.py:104-113 (a convolution kernel is passed in its memory order with
 * rows = output channels; singular values do not depend on the order of the columns).
 *   `iterations` steps of  v <- W^T u / max(|W^T u|, eps),  u <- W v / max(|W v|, eps)   (--spectral_iterations,
 *   run.py:269; 0 = inference: u, v are used as they are);  sigma = u^T W v;  w_sn = W / sigma.
 * u (rows) and v (cols) are updated in place when iterations > 0.  One launch of up to 32 co-resident workgroups that
 * meet through the last 16 bytes of `ws`: a buffer of wc_spectral_norm_workspace_bytes() that belongs to this weight,
 * ZEROED ONCE by the caller before its first use (a zeroing allocation, never an uninitialised one: the meeting words are counters every
 * workgroup increments, and the per-workgroup maxima beyond the launch's own keep the caller's zeros; every launch leaves the meeting
 * words zero) and used by one launch at
 * a time.  rows + cols floats must fit the LDS (WC_ERR_SHAPE otherwise). */
size_t wc_spectral_norm_workspace_bytes(int rows, int cols);
/* After a forward call the 32 floats at this byte offset of `ws` hold per-workgroup maxima of |w_sn| (unused entries keep
 * the caller's zeros): wc_conv_weights_f32 takes them as `known_amax` and skips its own sweep over the weight. */
size_t wc_spectral_norm_amax_offset(int rows, int cols);
/* The unsigned word at this byte offset of `ws` is the weight's sticky error word: a workgroup whose wait for its peers ran out
 * (> 0.1 s: the device could not hold the launch's workgroups at once -- CUs held by another process or stream) sets it to 1 and
 * goes on; that call's outputs are then invalid.  0 after every normal call; never cleared by the library. */
size_t wc_spectral_norm_error_offset(int rows, int cols);
int wc_spectral_norm_f32(const float* W, int rows, int cols, float* u, float* v, int iterations, float eps,
                         float* w_sn /*[rows*cols] out*/, float* sigma /*[1] out*/,
                         float* u_used /*[rows] out, nullable*/, float* v_used /*[cols] out, nullable: u, v as used for sigma,
                                                                    for the backward of THIS call (u, v move on)*/,
                         void* ws, size_t ws_bytes, wc_stream_t stream);

/* Gradient of the above w.r.t. W for constant u, v:  dW = (g - fully_diff * <g, w_sn> u v^T) / sigma.
 * fully_diff == 0 treats sigma as a constant of the step (--fully_diff_spectral 0, run.py:268: dW = g / sigma).
 * Same workspace rules (the same buffer as the forward may be passed: different words are used). */
int wc_spectral_norm_bwd_f32(const float* g, const float* w_sn, const float* u, const float* v, const float* sigma,
                             int rows, int cols, int fully_diff, float* dW,
                             void* ws, size_t ws_bytes, wc_stream_t stream);

/* The same two operations for EVERY spectrally normalised layer of a network in one launch each: the layers depend on
 * the weights only, not on each other or on the activations, and one launch keeps up to 16 x 32 workgroups busy where
 * per-layer launches run back to back on a mostly idle chip.  `items` is a HOST array (its contents travel in the
 * kernel arguments); every field as in the per-layer calls, one workspace per item. */
typedef struct {
    const float* W; float* u; float* v; float* w_sn; float* sigma; float* u_used; float* v_used; void* ws;
    int rows, cols;
} wc_sn_item;
typedef struct {
    const float* g; const float* w_sn; const float* u; const float* v; const float* sigma; float* dW; void* ws;
    int rows, cols;
} wc_sn_bwd_item;
int wc_spectral_norm_batched_f32(const wc_sn_item* items, int count, int iterations, float eps, wc_stream_t stream);
int wc_spectral_norm_bwd_batched_f32(const wc_sn_bwd_item* items, int count, int fully_diff, wc_stream_t stream);

/* ---- Convolutions around the WC sites (the callers either side of the path) ------------------
 * Replaces, for the generator/critic residual blocks, Keras `Conv2D(3x3, padding='same')` (generator.py:142-158,
 * discriminator.py:41-54), its `UpSampling2D -> Conv2D` and `Conv2D -> AveragePooling2D` pairs (as ONE 4x4 stride-2
 * transposed / strided convolution: exact rewrites) and the data gradient of each, fp32-accurate
 * on the fp16 MFMA pipe with split operands (3 products, the scheme of wc_apply_f32's fast path).
 *
 * One geometry describes all of them as an implicit GEMM over a "virtual grid" (N, H, W): point (y, x) of phase p
 * reads input pixel (y*in_stride + dy[p][t], x*in_stride + dx[p][t]) for tap t (zero outside the Hin x Win plane) and
 * writes output pixel (y*out_stride + off_y[p], x*out_stride + off_x[p]) of the Hout x Wout plane; tap t of phase p
 * multiplies by a weight slice built from the source slices (wr, ws) below.  Tensors are NHWC fp32, dense.
 *   3x3 same:              H=Hin=Hout, strides 1, 9 taps dy=r-1;  1 phase
 *   4x4 stride-2 conv:     H=Hout=Hin/2, in_stride 2, 16 taps dy=r-1; 1 phase
 *   4x4 stride-2 transposed conv: H=Hin, out_stride 2, 4 phases (py,px) of 2x2 taps, r = py+1-2*dy
 * Data gradients are the same three with the channel roles swapped in the weight image (stride_k <-> stride_n). */
typedef struct {
    int N, H, W;                    /* virtual grid */
    int Hin, Win, Cin;              /* input plane, reduction channels (multiple of 32) */
    int Hout, Wout, Cout;           /* output plane, output channels (multiple of 128) */
    int in_stride, out_stride;
    int ntaps, nphase;              /* <= 16 taps, <= 4 phases */
    signed char dy[4][16], dx[4][16];
    signed char off_y[4], off_x[4];
    /* the weight slice of tap t of phase p = wcoef * the sum of nsrc[p][t] (1..4) source slices (wr[p][t][m], ws[p][t][m]):
     * one slice for a plain convolution; the 4x4 kernels of the pooled / upsampled 3x3 convolutions are sums of 3x3 taps
     *  and are formed here, from the 3x3 weight -- and the weight gradient is folded back the same way */
    signed char nsrc[4][16];
    signed char wr[4][16][4], ws[4][16][4];
    float wcoef;
} wc_conv_geom;

#define WC_CONV_SCRATCH_BYTES 2048

/* 1 when wc_conv_f16x3 takes the geometry (N*H*W a multiple of 128, Cin a multiple of 32, Cout a multiple of 64: a width that is 64
 * beyond a multiple of 128 -- the DC critic's 64-filter layers, discriminator.py:41-60 with arch 'dcgan' -- runs 64-output tiles). */
int wc_conv_supported(const wc_conv_geom* g);

/* 1 for every geometry wc_conv_supported takes, and for the same geometries with N*H*W a multiple of 32 instead of 128 (below 2^31 - 128):
 * the launch runs ceil(N*H*W / 128) of the 128-point tiles, and the 32, 64 or 96 rows the last one has past the grid read zeros and
 * write nothing -- never the 256-point tile.  This is the set the launch entries (wc_conv_f16x3, _res_, _tail_, wc_conv_wrw_*_f16x3,
 * wc_conv_bwd_pair_*) accept, and wc_conv_res_supported / _tail_supported / _bwd_pair_supported answer for such a geometry under their
 * own rules, with tiles counted as ceil(N*H*W / 128); wc_conv_supported keeps its value (whole tiles only), which is what a caller that
 * has not opted in asks (wc_gan_amd/conv.py: a layer built with ragged_conv=True asks this one). */
int wc_conv_ragged_supported(const wc_conv_geom* g);

/* 1 when the geometry is one wc_conv_supported takes, or differs from one only in its output width: Cout any multiple of 32 (Cin as ever).
 * N*H*W is a multiple of 128 -- whole tiles; a width that is 32 beyond a multiple of 64 on a partial last tile is in no set.  The launch
 * entries wc_conv_f16x3 and wc_conv_wrw_[bias_]f16x3 (and the two *_workspace_bytes) accept the union of this set and
 * wc_conv_ragged_supported's: Cout % 64 == 32 runs on 128-point x 32-output tiles, a weight gradient with Cin % 64 == 32 or
 * Cout % 64 == 32 on 32 x 32 tiles, in either weight memory format.  wc_conv_res_supported / _tail_supported / _bwd_pair_supported answer
 * 0 for a 32-wide side, and wc_conv_supported / wc_conv_ragged_supported keep their values: a caller that has not opted in asks those
 * (wc_gan_amd/conv.py: a layer built with slim_conv=True asks this one). */
int wc_conv_slim_supported(const wc_conv_geom* g);

/* hi = fp16(s*x), lo = fp16(s*x - hi) over n floats (n % 4 == 0), s = the power of two that puts max|x| into
 * [2^13, 2^14) (written to *scale on the device); relu != 0 clamps at zero first.  `amax_scratch`: WC_CONV_SCRATCH_BYTES
 * device bytes (per-workgroup maxima; no atomics, nothing to clear). */
int wc_conv_split_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, void* amax_scratch,
                      wc_stream_t stream);

/* The same, and -- when `colsum_partials` (WC_CONV_COLSUM_ROWS x C floats) is given -- partial column sums of x seen as
 * rows of C channels (C a multiple of 4 with 256 % (C/4) == 0), collected while the maximum is taken: the bias gradient of
 * a layer whose output gradient is being split; wc_conv_wrw_bias_f16x3 adds the rows up. */
#define WC_CONV_COLSUM_ROWS 512
int wc_conv_split_colsum_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, void* amax_scratch,
                             float* colsum_partials, int C, wc_stream_t stream);

/* The same split in ONE launch, its scale taken from the call before at the same call site (ABI 7).  `hist`: WC_CONV_HIST_FLOATS floats
 * that belong to the call site (one convolution's input, or its output gradient), zero-filled once by the caller before the site's first call
 * (a zeroing allocation, never an uninitialised one: word WC_CONV_HIST_REDO is only ever incremented) and kept across calls: two arrays of
 * 512 (maximum, tag) pairs.  A call reads both, takes the array whose tags are all equal with the larger tag -- what the previous call
 * left -- and the power of two that puts THAT maximum into [2^7, 2^8): room for a 255-fold growth before fp16 overflows, precision to
 * 2^-20 of the tensor's maximum down to a 4000-fold shrink (hi + lo carry 22 bits wherever the scaled maximum lies in [2^-5, 65504]);
 * each workgroup leaves (its maximum, tag + 1) in the other array.  No atomics, no host-side parity: the record is a function of the
 * sequence of tensors alone, so an eager run and a replayed hipGraph of the same calls give the same bits.  NOTHING clamps.
 * ABI 8: a gated second launch follows on the same stream; it reads the record (the tensor's own maximum is in it by then) and, when the
 * scaled maximum fell outside [2^-5, 65504) -- the previous tensor was all zero (a saturated hinge critic), a growth beyond 255-fold, a
 * shrink beyond 4096-fold -- splits the tensor again with the MEASURED scale (the bits of wc_conv_split_f32) and counts the event in word
 * WC_CONV_HIST_REDO of `hist`; inside the window it returns at once.  Capturable, no host synchronisation, never quietly wrong.
 * The second launch costs ~2.3 us per call (0.56 ms of the 18-ms CIFAR-10 step when every split of the step takes it: as much as the
 * history saves), so the caller chooses per call: bit 1 of `bootstrap` set = no second launch.  The shipped layers take it for the OUTPUT
 * GRADIENTS (the tensors that do go to zero and swing by orders of magnitude) and not for the layer inputs.  Without it a call is still
 * exact after all-zero tensors (the record carries the maximum a call assumed: zeros leave the site's scale where it was), loud above a
 * 255-fold growth (inf), and short of bits for ONE call after a shrink beyond 4096-fold.
 * bit 0 of `bootstrap` (the site's first call): the two-launch form with the measured maximum, which seeds the record.  Calls of one
 * site must be ordered (one stream, or events).
 * colsum_partials / C as in wc_conv_split_colsum_f32 (nullable).  Replaces the absmax pass of wc_conv_split_f32 (~130 launches of
 * 3-30 us per G+D step; reference call sites: every Conv2D of discriminator.py:41-54 / generator.py:142-158 as in wc_conv_f16x3). */
#define WC_CONV_HIST_FLOATS (4 * 512 + 16)
#define WC_CONV_HIST_REDO (4 * 512)      /* index of the uint32 count of second passes taken */
int wc_conv_split_hist_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, float* colsum_partials /*nullable*/, int C,
                           float* hist, int bootstrap, wc_stream_t stream);

/* LeakyReLU in front of the split (the DC critic's LeakyReLU -> Conv2D pairs, discriminator.py:41-60: Keras's default slope 0.3):
 * v = x > 0 ? x : negative_slope * x (one fp32 multiply), then the scaling and hi / lo rounding of the entries above.  0 <= slope <= 1
 * (the measured scale is that of the activated tensor, max|LeakyReLU(x)|); slope 0 takes the ReLU form and gives the bits of relu = 1.
 * wc_conv_split_leaky_f32 = wc_conv_split_colsum_f32 (colsum_partials nullable), wc_conv_split_hist_leaky_f32 = wc_conv_split_hist_f32
 * with the same record rules (the record holds the maximum AFTER the activation, as with the ReLU).
 * wc_conv_leaky_bwd_f32: the activation's backward on the data gradient, in place and in one launch: dx[i] *= x[i] > 0 ? 1 : slope
 * (torch's convention at 0); n % 4 == 0. */
int wc_conv_split_leaky_f32(const float* x, int64_t n, float negative_slope, void* hi, void* lo, float* scale, void* amax_scratch,
                            float* colsum_partials /*nullable*/, int C, wc_stream_t stream);
int wc_conv_split_hist_leaky_f32(const float* x, int64_t n, float negative_slope, void* hi, void* lo, float* scale,
                                 float* colsum_partials /*nullable*/, int C, float* hist, int bootstrap, wc_stream_t stream);
int wc_conv_leaky_bwd_f32(float* dx, const float* x, int64_t n, float negative_slope, wc_stream_t stream);

/* Weight fragment images for a geometry: element (k, n, r, s) of the source is w[k*stride_k + n*stride_n + r*stride_r +
 * s*stride_s] (k = reduction channel, n = output channel of the product), `n_elems` = extent of the source storage (for
 * the tensor scale).  `image`: wc_conv_weights_bytes(g) device bytes.  `known_amax` (nullable): `known_count` device
 * floats whose maximum is max|w| (e.g. the ones wc_spectral_norm_f32 leaves) -- then the weight is not swept again. */
size_t wc_conv_weights_bytes(const wc_conv_geom* g);
int wc_conv_weights_f32(const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                        int64_t n_elems, const wc_conv_geom* g, void* image, float* scale, void* amax_scratch,
                        const float* known_amax, int known_count, wc_stream_t stream);

/* The images of one weight for two geometries (the layer's forward and its data gradient) in one launch: as two calls of
 * wc_conv_weights_f32 with the same source; `scale`: TWO floats (one per image, equal). */
int wc_conv_weights_pair_f32(const float* w, int64_t stride_r, int64_t stride_s, int64_t n_elems,
                             int64_t a_stride_k, int64_t a_stride_n, const wc_conv_geom* ga, void* image_a,
                             int64_t b_stride_k, int64_t b_stride_n, const wc_conv_geom* gb, void* image_b,
                             float* scale, void* amax_scratch, const float* known_amax, int known_count,
                             wc_stream_t stream);

/* The images of MANY weights in one launch: a pass's images depend on its weights only, so a network builds them all at the top of
 * the pass instead of one launch per layer between the layer's split and its convolution.  `jobs` is a HOST array (its contents travel
 * in the kernel arguments: no copy to the device, no allocation; capturable like the per-layer entries).  Every field as in
 * wc_conv_weights_f32, and the image and the scale have its bits; `scale` is ONE float per job.  `amax`: `amax_count` (1..4096) device
 * floats whose maximum is max|w| -- the spectral-norm op's, or the WC_CONV_ABSMAX_FLOATS partials wc_conv_absmax_batch_f32 left --; NULL:
 * the maximum is taken inside the job (n_elems <= 32768, n_elems % 4 == 0, w 16-byte aligned: wc_conv_weights_f32's rule; WC_ERR_ARG
 * otherwise).  `pair_of`: -1, or the index (smaller than the job's own) of the other image of the SAME weight -- a layer's forward and
 * data-gradient image stay two jobs; the entry checks that both read the same source and maximum and come to the same scale
 * (WC_ERR_ARG otherwise, as wc_conv_weights_pair_f32).  Any count > 0: a list that does not fit one launch's arguments (16 jobs, 6
 * distinct tap-source tables) takes several, filled greedily; wc_conv_weights_batch_launches says how many (or a negative error).
 * Errors (nothing is launched): WC_ERR_NULL a null list or field, WC_ERR_SHAPE count <= 0, WC_ERR_ARG a job the per-layer entry refuses. */
typedef struct {
    const float* w; int64_t stride_k, stride_n, stride_r, stride_s, n_elems;
    const wc_conv_geom* g; void* image; float* scale;
    const float* amax; int amax_count; int pair_of;
} wc_conv_weights_job;
int wc_conv_weights_batch_f32(const wc_conv_weights_job* jobs, int count, wc_stream_t stream);
int wc_conv_weights_batch_launches(const wc_conv_weights_job* jobs, int count);

/* max|x| of many tensors in one launch (the weights no spectral norm has measured): per job WC_CONV_ABSMAX_FLOATS per-workgroup maxima
 * of the n floats at x (16-byte aligned) in `partial`, the ones wc_conv_weights_f32's own sweep leaves in its scratch, bit for bit.
 * Same error rules. */
#define WC_CONV_ABSMAX_FLOATS 512
typedef struct { const float* x; int64_t n; float* partial; } wc_conv_absmax_job;
int wc_conv_absmax_batch_f32(const wc_conv_absmax_job* jobs, int count, wc_stream_t stream);

/* y = conv(x, w) (+ bias[Cout]) (then max(., 0) when relu != 0) for the geometry; x as split planes, `zero_line` = 64
 * device bytes of zeros (the padding). */
size_t wc_conv_workspace_bytes(const wc_conv_geom* g);     /* 0 unless the grid is small (the tap loop is then shared) */
int wc_conv_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                  const float* bias, const void* zero_line, const wc_conv_geom* g, int relu, float* y,
                  void* ws, size_t ws_bytes, wc_stream_t stream);

/* The passes between the critic's convolutions (discriminator.py:41-54: relu -> conv -> relu -> conv (-> pool), + shortcut), in the
 * launches that are there anyway.  These three entries are new; WC_CORE_API keeps its list and WC_ABI_VERSION, which covers that core,
 * its value.  (The same change is NOT additive for two extension entries further down: wc_conv_split_masked_f32 and
 * wc_conv_split_hist_masked_f32 took `colsum_partials, C` in front of their trailing arguments.  A caller built against their old
 * signatures has to be rebuilt; the binding table of _lib.py refuses a library without the new symbols below, old or new.)
 * wc_conv_res_f16x3: y = (conv(x, w) + bias) + res, res of y's shape -- the block's `h + s` in the finish of the convolution whose tap
 *   loop is shared over workgroups (wc_conv_res_supported: wc_conv_workspace_bytes(g) > 0 and Cout a multiple of 128); the bits of
 *   wc_conv_f16x3 followed by an elementwise fp32 add.  Other geometries: WC_ERR_SHAPE, the caller adds.  ws as in wc_conv_f16x3.
 * wc_conv_block_dx_f32: the gradient of a block's input from the first convolution's data gradient dx1, the block input x (the ReLU's
 *   mask: x <= 0 gives +0, a NaN lets the gradient through, as aten::threshold_backward) and the other branch, NHWC, C % 4 == 0:
 *     down == 0:  out = mask(dx1) + other,                          other [N,H,W,C]: the block's output gradient (identity shortcut)
 *     down != 0:  out = mask(dx1) + 0.25 * other[n][y/2][x/2][c],   other [N,H/2,W/2,C]: the gradient in front of the 2x2 average pooling
 *   (0.25 * other rounded on its own, then one add: the bits of the three elementwise passes it replaces).  out must not alias an input. */
int wc_conv_res_supported(const wc_conv_geom* g);
int wc_conv_res_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                      const float* bias, const float* res, const void* zero_line, const wc_conv_geom* g, float* y,
                      void* ws, size_t ws_bytes, wc_stream_t stream);
int wc_conv_block_dx_f32(const float* dx1, const float* x, const float* other, int64_t N, int64_t H, int64_t W, int C, int down,
                         float* out, wc_stream_t stream);

/* Weight gradient of the same convolution: dW(k, n, r, s) = sum over the grid of x[input pixel][k] * gy[output pixel][n]
 * for the FORWARD geometry `g` (x and gy as split planes; Cin and Cout multiples of 64 -- 64 x 64 tiles when either is no multiple
 * of 128), written to
 * dw[k*stride_k + n*stride_n + r*stride_r + s*stride_s] (every element of the taps the geometry names; fixed summation
 * order).  `ws`: wc_conv_wrw_workspace_bytes(g) device bytes. */
size_t wc_conv_wrw_workspace_bytes(const wc_conv_geom* g);
int wc_conv_wrw_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* ghi, const void* glo,
                      const float* gscale, const void* zero_line, const wc_conv_geom* g, float* dw, int64_t stride_k,
                      int64_t stride_n, int64_t stride_r, int64_t stride_s, void* ws, size_t ws_bytes,
                      wc_stream_t stream);

/* Weight and bias gradient of a 'same' convolution (1x1 or 3x3, stride 1) with a handful of INPUT channels, ksize^2 * Cin < 32 -- the
 * critic's first block on images: Conv2D 3 -> 128 and the 1x1 shortcut 3 -> 128 (discriminator.py:41-54; ABI 7).  x [N,H,W,Cin] and
 * gy [N,H,W,Cout] in fp32 NHWC, Cout a multiple of 128; one pass over gy on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, no split, no scales):
 *     dw[c*stride_k + o*stride_n + r*stride_r + s*stride_s] = sum_p x[p + (r, s) - pad][c] gy[p][o],   db[o] = sum_p gy[p][o]  (nullable)
 * in a fixed summation order.  `ws`: wc_conv_wrw_narrow_workspace_bytes(...) device bytes.  Replaces MIOpen's fp32 weight-gradient kernels
 * for these layers (138 / 54 us per critic update at 128x32x32, 0.5 TB/s of gy) and the bias gradient's reduction. */
int    wc_conv_wrw_narrow_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
size_t wc_conv_wrw_narrow_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int    wc_conv_wrw_narrow_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                              float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db /*nullable*/,
                              void* ws, size_t ws_bytes, wc_stream_t stream);

/* The same three for Cout a multiple of 64 (the DC critic's first layer, 3 -> 64 at 3x3): a superset -- the entries above keep refusing
 * what they refused (callers size and gate by them).  A last group of 64 channels runs the 128-channel group with half its lanes idle;
 * the workspace holds one partial per STARTED 128 channels.  Every narrow predicate and workspace function declines W < 2 (as the block
 * convolutions do: the kernels' multiply-shift division of the pixel index wants divisors >= 2) -- such a layer is the caller's. */
int    wc_conv_narrow64_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
size_t wc_conv_wrw_narrow64_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int    wc_conv_wrw_narrow64_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                                float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db /*nullable*/,
                                void* ws, size_t ws_bytes, wc_stream_t stream);

/* Forward of the same kind of layer (ksize^2 * Cin < 32, Cout a multiple of 64; wc_conv_narrow64_supported):
 *     y[p][o] = bias[o] + sum_{r,s,c} x[p + (r, s) - pad][c] w[c*stride_k + o*stride_n + r*stride_r + s*stride_s]      (relu != 0: max(., 0))
 * in one launch on the fp32 matrix pipe, the bias as a row of the product (bias nullable).  The strides may be negative: with x := gy of a layer
 * with a handful of OUTPUT channels, stride_k / stride_n exchanged and the tap strides negated (w pointing at its last tap) this is that
 * layer's data gradient (the generator's last layer, generator.py:155-157).  Replaces MIOpen's forward + two bias launches for the critic's
 * first block (discriminator.py:41-54 on images). */
int    wc_conv_fwd_narrow_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                              const float* bias /*nullable*/, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu,
                              float* y, wc_stream_t stream);

/* ==== the critic's first block: conv1 writes conv2's planes, conv1's weight gradient applies the ReLU mask ==============================
 * Additive: WC_CORE_API keeps its list and WC_ABI_VERSION its value; the entries above keep their signatures and their kernels.
 * The first block (discriminator.py:41-54 with is_first) holds the critic's largest tensor, conv1's output h (64 MiB at 128x32x32x128).
 *
 * wc_conv_fwd_narrow_split_f32 = wc_conv_fwd_narrow_f32(..., relu = 0, y) followed by wc_conv_split_hist_f32(y, relu, slope, ...) on an
 * already seeded record `hist` (WC_CONV_HIST_FLOATS floats) of the convolution that reads act(y), in ONE launch: the kernel splits the
 * 16 bytes a lane is about to store.  y, hi, lo and scale[0] have the bits of the two launches; so has what the record shows to its
 * readers -- the fold of the newer complete array, its tag, the two assumed words, the redo counter (single pairs may differ: a workgroup
 * here writes the pairs b, b + G, ... of a grid of G workgroups with its own maximum).  relu / slope: the activation in front of the split
 * (0 none, 1 ReLU, 2 LeakyReLU); y itself stays unactivated.  flags: WC_NARROW_SPLIT_NO_REDO leaves out the gated second pass (a launch
 * of its own on y, as behind wc_conv_split_hist_f32), WC_NARROW_SPLIT_NT stores y with the non-temporal hint.
 * wc_conv_fwd_narrow_split_supported: the narrow forward's shapes whose grid has at most 512 workgroups (one pair of the record each at
 * least); WC_ERR_SHAPE otherwise -- the caller then runs the two launches. */
#define WC_NARROW_SPLIT_NO_REDO 2
#define WC_NARROW_SPLIT_NT 4
int    wc_conv_fwd_narrow_split_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int    wc_conv_fwd_narrow_split_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                    const float* bias /*nullable*/, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                                    int relu, float slope, float* y, void* hi, void* lo, float* scale, float* hist, int flags,
                                    wc_stream_t stream);

/* wc_conv_wrw_narrow64_f32 with gy read through a ReLU's backward: the sums are those of gy[p][o] * (mask[p][o] <= 0 ? 0 : 1), mask of
 * gy's shape (torch's threshold_backward(gy, mask, 0) predicate: a NaN in mask lets the gradient through) -- dw and db have the bits of
 * the plain entry on the masked copy for every finite gy, and that copy is never written. */
int    wc_conv_wrw_narrow_masked_f32(const float* x, const float* gy, const float* mask, int64_t N, int64_t H, int64_t W, int Cin, int Cout,
                                     int ksize, float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                     float* db /*nullable*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* 'same' convolution (1x1 or 3x3, stride 1) with a handful of OUTPUT channels -- the data gradient of an image layer (the critic's first
 * block: conv1 and the 1x1 shortcut, discriminator.py:41-54 on images).  g [N,H,W,Cw] fp32 NHWC is the wide tensor, out [N,H,W,Cn], p = ksize / 2:
 *     out[n][y][x][c] = sum_{r,s} sum_o m(g)[n][y - (r - p)][x - (s - p)][o] * w[o*stride_k + c*stride_n + r*stride_r + s*stride_s]
 * positions outside the image contributing zero.  m(g) = g, or with `mask` (nullable; g's shape) threshold_backward(g, mask, 0):
 * g[..] * (mask[..] <= 0 ? 0 : 1), applied as g is read -- the masked copy is never written.  With w the layer's (Cw, Cn, k, k) weight,
 * stride_k / stride_n = its strides 0 / 1, this is the layer's data gradient; with the tap strides negated (w pointing at its last
 * tap) and the channel strides exchanged it is the forward of a layer (Cn, Cw, k, k) with few outputs.  One pass over g (and mask) on the
 * fp32 matrix pipe, no atomics, a fixed summation order: the same bits on every call.  Additive: WC_ABI_VERSION keeps its value.
 * wc_conv_narrow_out_supported: ksize in {1, 3}, ksize^2 * Cn < 32, Cw % 32 == 0, W >= 2, N*H*W < 2^31, and the weight with ksize image
 * rows of the per-pixel products within a workgroup's LDS (80 KiB: W * (ksize^2 * Cn | 1) * ksize + 32 * Cw floats); WC_ERR_SHAPE
 * otherwise, nothing launched.  g and mask 16-byte aligned (WC_ERR_ARG). */
int    wc_conv_narrow_out_supported(int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize);
int    wc_conv_narrow_out_f32(const float* g, const float* mask /*nullable*/, const float* w, int64_t stride_k, int64_t stride_n,
                              int64_t stride_r, int64_t stride_s, int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize,
                              float* out, wc_stream_t stream);

/* ==== the narrow kernels at a wide side of 32 channels: the ImageNet generator's last layer, 32 -> 3 at 128 x 128 ========
 * Additive: WC_CORE_API keeps its list and WC_ABI_VERSION its value; every entry above keeps its signature, its kernel and its answers,
 * and the narrow64 / narrow predicates and workspace functions still decline what they declined.
 *
 * wc_conv_narrow32_supported: wc_conv_narrow64_supported with Cout % 32 == 0 in place of % 64 -- ksize in {1, 3}, ksize^2 * Cin < 32,
 * W >= 2, N*H*W < 2^31.  A superset.
 *
 * wc_conv_wrw_narrow32_f32 / wc_conv_wrw_narrow32_workspace_bytes: wc_conv_wrw_narrow64_f32's contract on that set.  Cout % 64 == 0: the
 * launches, the bits and the workspace size of wc_conv_wrw_narrow64_f32.  Cout % 64 == 32: a kernel whose channel group is 32 wide --
 * lane (i, k) loads the one float gy[p + k][32 grp + i], one v_mfma_f32_32x32x2_f32 per pixel pair -- and EVERY group of such a layer is
 * 32 wide (Cout = 96: three groups; 160: five), not 128-groups plus a remainder: one kernel and one element map per layer.  The same
 * pixel ranges, the same fold of a workgroup's eight waves and the same fixed order over the partials; no atomics, the same bits on
 * every call.
 *
 * wc_conv_fwd_narrow32_f32: wc_conv_fwd_narrow_f32's contract (negative strides, the bias as a row of the product, relu) on that set, with
 * N*H*W*Cin < 2^31 as there.  Cout % 64 == 0: that entry's launch and bits.  Cout % 64 == 32: the same body with one 32-channel block per
 * wave; a wave's tile leaves as 16-byte stores of whole 128-byte pixel rows. */
int    wc_conv_narrow32_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
size_t wc_conv_wrw_narrow32_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int    wc_conv_wrw_narrow32_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                                float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db /*nullable*/,
                                void* ws, size_t ws_bytes, wc_stream_t stream);
int    wc_conv_fwd_narrow32_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                const float* bias /*nullable*/, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu,
                                float* y, wc_stream_t stream);

/* wc_conv_narrow_out_f32 with bias[c] (Cn floats, nullable) added to each output behind its tap sum: the forward of a layer with few
 * outputs, bias included, in one launch.  bias == NULL: wc_conv_narrow_out_f32 itself, its kernels and its bits; with a bias the bits of
 * that result followed by one fp32 add. */
int    wc_conv_narrow_out_bias_f32(const float* g, const float* mask /*nullable*/, const float* w, int64_t stride_k, int64_t stride_n,
                                   int64_t stride_r, int64_t stride_s, const float* bias /*nullable*/, int64_t N, int64_t H, int64_t W,
                                   int Cw, int Cn, int ksize, float* out, wc_stream_t stream);

/* wc_conv_wrw_f16x3 plus the bias gradient db[Cout] = column sums of gy, from the partial rows wc_conv_split_colsum_f32
 * left while gy was split (fixed summation order, no extra launch). */
int wc_conv_wrw_bias_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* ghi, const void* glo,
                           const float* gscale, const void* zero_line, const wc_conv_geom* g, float* dw, int64_t stride_k,
                           int64_t stride_n, int64_t stride_r, int64_t stride_s, const float* colsum_partials, float* db,
                           void* ws, size_t ws_bytes, wc_stream_t stream);

/* One layer's backward in two launches instead of four: wc_conv_f16x3(gy planes, data-gradient image, gd, no bias, no ReLU) -> dx and
 * wc_conv_wrw_bias_f16x3(x planes, gy planes, gf) -> dw (, db) with the workgroups of both in ONE grid and one launch that finishes both
 * (the weight reduction, the bias gradient and -- where the data gradient is k-split -- its reduction).  Every workgroup runs what it runs
 * in the two entries, on the same operands, and the reductions keep their order: dx, dw and db have the bits of the two calls.
 * gd / gf: the data-gradient and the forward geometry of the layer.  wc_conv_bwd_pair_supported: both gradients on 128 x 128 tiles
 * (128-channel layers whose data gradient gives at most ~256 workgroups) of a 'same' or stride-2 down-sampling layer; everything else stays
 * on the two calls.  ws_dx: wc_conv_workspace_bytes(gd) bytes (may be NULL when that is 0), ws_dw: wc_conv_wrw_workspace_bytes(gf) bytes;
 * wc_conv_bwd_pair_workspace_bytes is their sum.  colsum_partials / db: both or neither, as in wc_conv_wrw_bias_f16x3.  Additive: WC_CORE_API
 * keeps its list and WC_ABI_VERSION its value. */
int    wc_conv_bwd_pair_supported(const wc_conv_geom* gd, const wc_conv_geom* gf);
size_t wc_conv_bwd_pair_workspace_bytes(const wc_conv_geom* gd, const wc_conv_geom* gf);
int    wc_conv_bwd_pair_f16x3(const void* ghi, const void* glo, const float* gscale, const void* wimage, const float* wscale,
                              const void* zero_line, const wc_conv_geom* gd, float* dx, void* ws_dx, size_t ws_dx_bytes,
                              const void* xhi, const void* xlo, const float* xscale, const wc_conv_geom* gf, float* dw,
                              int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                              const float* colsum_partials, float* db, void* ws_dw, size_t ws_dw_bytes, wc_stream_t stream);

/* A k-split finish that goes on to do what the next launch did (the critic's 128-channel blocks at 8x8).  Where a convolution's tap loop is
 * shared over workgroups (wc_conv_tail_supported: the geometries of wc_conv_res_supported), an elementwise launch finishes it -- and the
 * very next launch used to read that fp32 tensor back only to re-express it.  These entries run the convolution of wc_conv_f16x3 (no ReLU) /
 * the layer backward of wc_conv_bwd_pair_f16x3 unchanged and give the finish a tail, wc_conv_tail.kind:
 *   WC_CONV_TAIL_SPLIT   y = (conv + bias) + res (res nullable: wc_conv_res_f16x3's value) in fp32 AND the planes of relu(y), scaled by the
 *                        record `hist` of the convolution that reads them: hi / lo / scale / hist as wc_conv_split_hist_f32 with relu = 1
 *                        leaves them, the record's pairs and carried maximum included.  The forward entry only.
 *   WC_CONV_TAIL_MASKED  y (the data gradient) in fp32 AND the planes of y * (mask > 0), mask of y's shape: hi / lo / scale / hist and the
 *                        kAmaxBlocks = 512 partial rows colsum_partials (nullable; C = Cout) as wc_conv_split_hist_masked_f32 with slope 0
 *                        leaves them.
 *   WC_CONV_TAIL_DX      out = (mask > 0 ? conv : 0) + other, mask and other of the output's shape: wc_conv_block_dx_f32 with down = 0 on
 *                        the finished value, which is never written (y / dx may be NULL).  out must not alias an input.
 * redo != 0 (SPLIT, MASKED): the gated second pass of the history-scaled split follows, as behind the split entries.  The record must be
 * SEEDED (the site's first call goes through the split entries with bootstrap bit 0); every value has the bits of the two launches it
 * replaces -- the finish launch runs the split's 512 x 256 grid.  Geometries without a shared tap loop: WC_ERR_SHAPE, the caller keeps the
 * two launches.  Additive: WC_CORE_API keeps its list and WC_ABI_VERSION its value. */
#define WC_CONV_TAIL_SPLIT 1
#define WC_CONV_TAIL_MASKED 2
#define WC_CONV_TAIL_DX 3
typedef struct wc_conv_tail {
    int kind;
    int redo;
    const float* res;                 /* SPLIT */
    const float* mask;                /* MASKED, DX */
    const float* other;               /* DX */
    float* out;                       /* DX */
    void* hi; void* lo; float* scale; float* hist;      /* SPLIT, MASKED */
    float* colsum_partials; int C;    /* MASKED */
} wc_conv_tail;
int wc_conv_tail_supported(const wc_conv_geom* g);
int wc_conv_tail_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                       const float* bias, const void* zero_line, const wc_conv_geom* g, float* y,
                       void* ws, size_t ws_bytes, const wc_conv_tail* tail, wc_stream_t stream);
int wc_conv_bwd_pair_tail_f16x3(const void* ghi, const void* glo, const float* gscale, const void* wimage, const float* wscale,
                                const void* zero_line, const wc_conv_geom* gd, float* dx, void* ws_dx, size_t ws_dx_bytes,
                                const void* xhi, const void* xlo, const float* xscale, const wc_conv_geom* gf, float* dw,
                                int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                const float* colsum_partials, float* db, void* ws_dw, size_t ws_dw_bytes,
                                const wc_conv_tail* tail, wc_stream_t stream);
/* the gated second pass of wc_conv_split_hist_masked_f32 alone (behind a MASKED tail; arguments as there) */
int wc_conv_split_redo_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale, float* hist,
                                  wc_stream_t stream);

/* The same convolutions with the k-split's shares summed INSIDE the workgroup: no partial sums in memory, no finish launch, no workspace.
 * 64-point x 64-output tiles, one workgroup each; wave z computes the tile over share z of the (tap, chunk) loop, the four accumulators
 * are added in LDS in share order and the workgroup finishes the values itself.  Every value has the bits of the entries above:
 *   tail == NULL           wc_conv_f16x3 (res == NULL; relu as there) or wc_conv_res_f16x3 (res != NULL, relu == 0)
 *   tail != NULL           wc_conv_tail_f16x3 (res == NULL and relu == 0: the residual travels in the tail).  SPLIT / MASKED: the planes, the
 *                          scale word, the carried maximum and the FOLD of the record's pairs are those of that entry -- workgroup b of G
 *                          writes the pairs b, b + G, ... with its own maximum, so single pairs differ and nothing reads a single pair.
 *                          MASKED with colsum_partials: WC_ERR_SHAPE (the rows' summation order belongs to the 512-workgroup finish).
 * wc_conv_local_supported: a whole-tile geometry (wc_conv_supported) whose tap loop is shared FOUR ways (the value wc_conv_workspace_bytes
 * is computed from), Cout a multiple of 128 and not of 256, Cin a multiple of 64, and (N*H*W / 64) * nphase * (Cout / 64) workgroups at
 * most the device's CU count (256 where no device is present) and at most 512 -- the critic's 128-channel layers at 8x8, batch 128.
 * Elsewhere WC_ERR_SHAPE, nothing launched: the caller keeps the entries above, which keep their values and code.  Additive: WC_CORE_API
 * keeps its list and WC_ABI_VERSION its value. */
int wc_conv_local_supported(const wc_conv_geom* g);
int wc_conv_local_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                        const float* bias, const float* res, const void* zero_line, const wc_conv_geom* g, int relu, float* y,
                        const wc_conv_tail* tail, wc_stream_t stream);

/* Bandwidth yardstick used by bench.py: dst[i] = src[i] (float4 grid-stride copy), same stream rules. */
int wc_stream_copy_f32(const float* src, float* dst, int64_t n, wc_stream_t stream);

/* ==== norm 'b': batch standardisation + diagonal coloring =================================================================================
 * The second norm of create_norm's alphabet (generator.py:19-22), not a further route of the WC stages above -- so the rule "no new
 * extension enters without one leaving" does not apply to this block, WC_CORE_API keeps its list and WC_ABI_VERSION its value (the
 * entries are additive).  The site is the diagonal case of a WC site: the same (M, C) view, additive float64 moments, (table, slot)
 * coloring with VECTORS gamma / beta [Kc, C], the block's ReLU behind it:
 *     mu = sum / M,  var = sqsum / M - mu^2 (biased),  w = 1 / sqrt(var + eps)
 *     a[k] = gamma[k] w,  b[k] = beta[k] - a[k] mu,   y = fmaf(a[slot], x, b[slot]),   relu: y = !(y <= 0) ? y : 0
 * No matrix pipe: every kernel is an HBM stream.  The backward recomputes the ReLU's decision from x, a, b with the forward's own fmaf
 * (bit for bit), so neither y nor a mask is kept.  M < 2^31 rows. */

/* Raw additive moments (what a sync-BN would all-reduce): sum[g,c] = sum_m x[m,c], sqsum[g,c] = sum_m x[m,c]^2 over the M / groups
 * consecutive rows of group g, float64, fixed summation order.  The statistics half of BatchNormalization(center=False, scale=False),
 * generator.py:22. */
size_t wc_std_stats_workspace_bytes(int64_t M, int C, int groups);
int    wc_std_stats_f32(const float* x, int64_t M, int C, int groups, double* sum /*[groups,C]*/, double* sqsum /*[groups,C]*/,
                        void* ws, size_t ws_bytes, wc_stream_t stream);

/* Moments (training != 0) or moving statistics (training == 0: sum / sqsum ignored, may be NULL) -> mu, w [groups,C]; the moving
 * statistics' update moving <- momentum moving + (1 - momentum) batch (variance times M / (M - ddof): ddof 0 is Keras, 1 is torch), the
 * groups one after the other; and the tables a, b [groups*Kc, C], row g*Kc + k (gamma NULL = 1, beta NULL = 0).  M = rows per group.
 * 0 < eps < 1, 0 <= momentum <= 1, ddof 0 | 1 (the ranges wc_factor_f64 takes; WC_ERR_ARG otherwise); training needs M > ddof.
 * The normalising half of generator.py:22 and the centre / scale layers of generator.py:28-40 (CenterScale, ConditionalCenterScale). */
int    wc_std_factor_f64(const double* sum, const double* sqsum, int64_t M, int C, int groups, double eps, double momentum, int ddof,
                         int training, float* moving_mean /*[C] in/out, nullable*/, float* moving_variance /*[C] in/out, nullable*/,
                         const float* gamma /*[Kc,C], nullable*/, const float* beta /*[Kc,C], nullable*/, int Kc,
                         float* mu /*[groups,C]*/, float* w /*[groups,C]*/, float* a /*[groups*Kc,C]*/, float* b /*[groups*Kc,C]*/,
                         wc_stream_t stream);

/* y = fmaf(a[slot], x, b[slot]), relu != 0: the block's Activation('relu') (generator.py:155) in the same pass.  Kt = rows of a / b
 * (groups*Kc; slot values are clamped into it).  The apply half of generator.py:22 + 28-40. */
int    wc_std_apply_f32(const float* x, const float* a, const float* b, const int32_t* slot /*[N], nullable*/, int64_t N, int64_t HW,
                        int C, int Kt, int relu, float* y, wc_stream_t stream);

/* Backward (the TF graph gradients of the above, run.py:93-94).  g' = gy where the forward's fmaf(a, x, b) > 0 (relu != 0), else gy:
 *     gsum[k,c] = sum_{m in slot k} g'[m,c]      gxsum[k,c] = sum_{m in slot k} g'[m,c] x[m,c]        (float64, fixed order)
 * A slab of the reduction never straddles two samples when Kc > 1. */
size_t wc_std_bwd_reduce_workspace_bytes(int64_t N, int64_t HW, int C, int Kc);
int    wc_std_bwd_reduce_f32(const float* x, const float* gy, const float* a, const float* b, const int32_t* slot, int64_t N, int64_t HW,
                             int C, int Kc, int relu, double* gsum /*[Kc,C]*/, double* gxsum /*[Kc,C]*/,
                             void* ws, size_t ws_bytes, wc_stream_t stream);

/* dbeta[k] = gsum[k], dgamma[k] = w (gxsum[k] - mu gsum[k])  (both nullable), and with m1 = sum_k gamma[k] dbeta[k] / M,
 * m2 = sum_k gamma[k] dgamma[k] / M:  q = -w^2 m2,  r = w (w mu m2 - m1)   (training == 0: q = r = 0, the statistics are constants).
 * M = N*HW.  run.py:93-94. */
int    wc_std_bwd_factor_f64(const double* gsum, const double* gxsum, const float* mu /*[C]*/, const float* w /*[C]*/,
                             const float* gamma /*[Kc,C], nullable*/, int64_t M, int C, int Kc, int training,
                             float* dgamma /*[Kc,C]*/, float* dbeta /*[Kc,C]*/, float* q /*[C]*/, float* r /*[C]*/, wc_stream_t stream);

/* dx = a[slot] g' + q x + r, the ReLU's decision recomputed as in wc_std_bwd_reduce_f32.  run.py:93-94. */
int    wc_std_bwd_apply_f32(const float* x, const float* gy, const float* a, const float* b, const float* q, const float* r,
                            const int32_t* slot, int64_t N, int64_t HW, int C, int Kc, int relu, float* dx, wc_stream_t stream);

/* ==== decomposition = 'zca': the eigen-stage and its backward ==============================================================================
 * The layer's other `decomposition` value -- DecorelationNormalization(decomposition='zca'), the commented alternative at generator.py:24 --
 * not a further fusion of the stages above: as with norm 'b', WC_CORE_API keeps its list and WC_ABI_VERSION its value (the entries are
 * additive).  A ZCA site runs K1 + K2 as a Cholesky site does (any of their forms); the stage below turns K2's L into the symmetric
 * whitening matrix, and everything behind W (colouring, K3 and its epilogues, K4, K6) is unchanged:
 *     L L^T = (1 - eps) Sigma + eps I = U diag(sigma^2) U^T      (one-sided Jacobi on the columns of L: L J1 J2 ... = U diag(sigma))
 *     lam = (sigma^2 - eps^2) / (1 - eps)   (the eigenvalues of Sigma + eps I, same U),      W = U diag(lam^-1/2) U^T
 * Widths: C % 32 == 0, 32 <= C <= 256 (wc_zca_supported; WC_ERR_CHANNELS otherwise). */

/* The eigen-stage.  Replaces, in DecorelationNormalization.call with decomposition='zca' (generator.py:24), the tf.svd / tf.self_adjoint_eig
 * of Sigma + eps I and the products that form U diag(S^-1/2) U^T.  L [groups,C,C]: K2's lower factors.  Out: U (column j belongs to lam[j];
 * eigenvalues in no particular order), lam [groups,C], W symmetric, stored in full.  Float64 throughout.  C <= 128: one launch holds a
 * group's matrix in LDS until a sweep rotates nothing; larger: a column-block form, every outer step a launch of its own, which leave
 * at once after convergence (no workgroup waits for another).  At most 30 sweeps.  Status: `groups` uint32 words 64 bytes apart at
 * wc_zca_status_offset() of the workspace hold the sweeps used; bit 31 set: the budget ran out -- W then also holds a NaN (K2's
 * convention).  Graph-capturable, allocates nothing. */
int    wc_zca_supported(int C);
size_t wc_zca_workspace_bytes(int C, int groups);
size_t wc_zca_status_offset(int C, int groups);
int    wc_zca_f64(const double* L /*[groups,C,C]*/, int C, int groups, double eps,
                  double* U /*[groups,C,C] out*/, double* lam /*[groups,C] out*/, double* W /*[groups,C,C] out*/,
                  void* ws, size_t ws_bytes, wc_stream_t stream);

/* K5 of a ZCA site: wc_bwd_factor_f64 with (U, lam) in place of L.  dgamma[k] = W R[k], gmean, dbeta as there; the statistics path is the
 * closed form without eigenvalue differences (Daleckii-Krein for f(lam) = lam^-1/2):
 *     Wbar = sum_k Gamma_k R_k^T;  B = U^T Wbar U;  F_ij = -1 / (r_i r_j (r_i + r_j)), r = sqrt(lam);  S = 2/(M - ddof) sym(U (B o F) U^T)
 * -- finite on degenerate spectra (fewer rows than channels, zero-padded widths), where the eigenvector gradient is not.  training == 0
 * behaves exactly as in wc_bwd_factor_f64.  Replaces the TF graph gradient of the decomposition above (run.py:93-94). */
size_t wc_bwd_factor_zca_workspace_bytes(int C, int Kc);
int    wc_bwd_factor_zca_f64(const double* R, const double* gsum, const double* W, const double* U, const double* lam,
                             const float* gamma, const float* A, int Kc, int C, int64_t M,
                             double eps, int ddof, int training,
                             float* dgamma /*[Kc,C,C]*/, float* dbeta /*[Kc,C]*/,
                             float* S /*[C,C]*/, float* gmean /*[C]*/,
                             void* ws, size_t ws_bytes, wc_stream_t stream);

/* ==== norm 'dr': renorm whitening, DecorelationNormalization(renorm=True) ==================================================
 * Additive like the entries above: WC_CORE_API keeps its list and WC_ABI_VERSION its value.  In training mode a renorm site whitens with
 *     W_eff = W_m sg(L) W,    L L^T = (1 - eps) Sigma_batch + eps I,  W = L^-1  (K2, unchanged),
 *                              L_m L_m^T = (1 - eps) moving_cov + eps I,  W_m = L_m^-1  (the moving statistics BEFORE this call's update)
 * whose value is W_m and whose gradient reaches x through W alone; C0 = W_m L (lower triangular) is a constant of the step.  The forward
 * colours with W_m in W's place (no C0 there); K5 takes W_m in dgamma and C0^T in front of its chain.  K1, K3, K4, K6 are untouched.
 * Widths: C % 32 == 0, 32 <= C <= 1024 (wc_renorm_supported; WC_ERR_CHANNELS otherwise). */

/* The moving factor and C0, float64, full matrices with exact zeros above the diagonal.  Two phases, selected by the nullable inputs, so
 * that a site can take the moving factor BEFORE K2 updates moving_cov in place and the product after K2 made L:
 *     moving_cov != NULL:  W_m <- inverse of the Cholesky factor of (1 - eps) moving_cov + eps I -- K2's evaluation-mode launches themselves
 *                          (bit for bit the W of wc_factor_f64 with training == 0)
 *     L != NULL:           C0 <- W_m L  (W_m as just computed, or as given when moving_cov == NULL); tiles above the diagonal are skipped
 *                          and k runs over the block columns j..i only (v_mfma_f64_16x16x4_f64)
 * At least one of the two must be given; C0 may be NULL when L is.  Stream-ordered, graph-capturable, allocates nothing. */
int    wc_renorm_supported(int C);
size_t wc_renorm_workspace_bytes(int C);
int    wc_renorm_f64(const float* moving_cov /*[C,C], nullable*/, const double* L /*[C,C], nullable*/, int C, double eps,
                     double* Wm /*[C,C] out (in when moving_cov == NULL)*/, double* C0 /*[C,C] out*/,
                     void* ws, size_t ws_bytes, wc_stream_t stream);

/* K5 of a renorm site: wc_bwd_factor_f64 with
 *     dgamma[k] = W_m R[k];   Wbar_eff = sum_k Gamma_k R_k^T;   P = -Phi(C0^T Wbar_eff W^T);   S = 2 (1 - eps) / (M - ddof) sym(W^T P W)
 * gmean and dbeta as there (A is the site's A_k = W_m^T Gamma_k).  training == 0: dgamma and dbeta only, S and gmean untouched. */
size_t wc_bwd_factor_renorm_workspace_bytes(int C, int Kc);
int    wc_bwd_factor_renorm_f64(const double* R, const double* gsum, const double* W, const double* Wm, const double* C0,
                                const float* gamma, const float* A, int Kc, int C, int64_t M,
                                double eps, int ddof, int training,
                                float* dgamma /*[Kc,C,C]*/, float* dbeta /*[Kc,C]*/,
                                float* S /*[C,C]*/, float* gmean /*[C]*/,
                                void* ws, size_t ws_bytes, wc_stream_t stream);

/* ==== gradient penalty of the WGAN-GP recipes (scripts/cifar10_resnet_wgan_*.sh, --gradinet_penalty_weight) ================================
 * Additive like the blocks above: WC_CORE_API keeps its list and WC_ABI_VERSION its value.  The penalty's weight gradient is the weight
 * gradient of a tangent pass through the critic with the primal pass's ReLU decisions frozen: it runs on
 * wc_conv_f16x3 / wc_conv_wrw_f16x3 and the narrow-input entries; these are the pieces around them.  All stream-ordered and
 * graph-capturable; nothing allocates. */

/* The operand split of a tangent: planes of t[i] * (a[i] > 0 ? 1 : slope), a = the primal pre-activation (fp32, t's shape), 0 <= slope <= 1
 * (0: the ResNet critic's ReLU; the DC critic's LeakyReLU is 0.3).  (hi, lo, scale), the scale rule, the `hist` record, `bootstrap` and the
 * gated second pass are those of wc_conv_split_f32 / wc_conv_split_hist_f32: the planes and the scale are bit for bit what those entries
 * give for the premultiplied fp32 tensor, without that tensor.  n % 4 == 0.
 * colsum_partials / C (nullable) as in wc_conv_split_colsum_f32 / wc_conv_split_hist_f32: the 512 partial rows of the column sums of the
 * MASKED values, bit for bit the rows those entries leave for the premultiplied tensor -- a convolution's output gradient behind a ReLU
 * (t = the data gradient of the layer behind it, a = this layer's output) needs no masked fp32 copy for its split or its bias gradient.
 * SIGNATURE CHANGE (WC_ABI_VERSION stays 8, it versions WC_CORE_API): both entries had no `colsum_partials, C` before. */
int wc_conv_split_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale, void* amax_scratch,
                             float* colsum_partials /*nullable*/, int C, wc_stream_t stream);
int wc_conv_split_hist_masked_f32(const float* t, const float* a, int64_t n, float slope, void* hi, void* lo, float* scale,
                                  float* colsum_partials /*nullable*/, int C, float* hist, int bootstrap, wc_stream_t stream);

/* x_hat[n] = eps[n] real[n] + (1 - eps[n]) fake[n] for N samples of L floats, eps [N] on the device (formed in float64, rounded once). */
int wc_gp_interp_f32(const float* real, const float* fake, const float* eps, int64_t N, int64_t L, float* x_hat, wc_stream_t stream);

/* For the input gradients g [N, L] of the critic:  norms[n] = ||g_n||_2,  v[n] = 2 lambda inv_n (1 - 1 / norms[n]) g[n]  (a zero row gives
 * v = 0, the subgradient torch's norm takes),  *penalty = lambda inv_n sum_n (norms[n] - 1)^2.  Sums of squares in float64 (rows of
 * magnitude 1e-20 or 1e+15 stay finite), one workgroup per sample, the N-term finish in a fixed order: the same bits on every call.
 * `ws`: wc_gp_rows_workspace_bytes(N) device bytes. */
size_t wc_gp_rows_workspace_bytes(int64_t N);
int wc_gp_rows_f32(const float* g, int64_t N, int64_t L, double lambda, double inv_n, float* norms /*[N]*/, float* v /*[N,L]*/,
                   float* penalty /*[1]*/, void* ws, size_t ws_bytes, wc_stream_t stream);

/* ==== Adam with the recipes' learning-rate schedules (run.py:99-144, --lr_decay_schedule), DESIGN.md section 4.18 ===========================
 * Additive like the blocks above: WC_CORE_API keeps its list and WC_ABI_VERSION its value.  Stream-ordered and graph-capturable; nothing
 * allocates or synchronises.  The update counter and the step's scalars are DEVICE values, so a replayed graph advances the schedule. */

/* One launch per optimiser step.  counter[0] = it, the number of updates already applied (int64, 8-byte aligned).  Writes
 *     record[0] = lr mult(it) / (1 - beta1^(it+1)),  record[1] = 1 / sqrt(1 - beta2^(it+1)),  record[2] = lr mult(it),  record[3] = mult(it)
 * (float64 arithmetic, rounded once; record 16-byte aligned) and then counter[0] = it + 1.  kind / mult:
 *     0 none         1
 *     1 linear       max(0, 1 - it / total)
 *     2 half-linear  the linear value while it < total / 2, then 0.5
 *     3 linear-end   min(1, max(0, (total - it) / (total - 0.828 total)))
 *     4 dropat       (it < drop_at ? 1 : 0.1) max(0, 1 - it / total)
 * total > 0 unless kind == 0; drop_at is read by kind 4 alone. */
int wc_adam_tick(int64_t* counter, float* record /*[4]*/, double lr, double beta1, double beta2, int kind, double total, double drop_at,
                 wc_stream_t stream);

/* The tensors of one update launch, passed to the kernel BY VALUE (3088 bytes of the 4 KiB kernel-argument segment): a network with
 * more than WC_ADAM_CAPACITY tensors takes further launches.  Tensor i: numel[i] fp32 parameters at param[i], their gradients at grad[i]
 * (the same element order), its moments at moment_off[i] elements into the flat buffers (a multiple of 4).  The launch has
 * chunk_start[count] workgroups of `chunk` elements (a multiple of 1024); tensor i owns the workgroups
 * chunk_start[i] .. chunk_start[i + 1] - 1 = ceil(numel[i] / chunk) of them, chunk_start[0] = 0. */
#define WC_ADAM_CAPACITY 96
typedef struct {
    float*       param[WC_ADAM_CAPACITY];
    const float* grad[WC_ADAM_CAPACITY];
    int64_t      moment_off[WC_ADAM_CAPACITY];
    int32_t      numel[WC_ADAM_CAPACITY];
    int32_t      chunk_start[WC_ADAM_CAPACITY + 1];
    int32_t      count, chunk;
} wc_adam_table;
int wc_adam_capacity(void);       /* WC_ADAM_CAPACITY, for a binding to check its struct against */

/* For every element of every tensor of the table, with a = record[0], r = record[1] (torch.optim.Adam's formula, no weight decay):
 *     exp_avg    <- exp_avg + (1 - beta1) (g - exp_avg)                (beta1 == 0: exp_avg is g; the buffer is not touched, may be NULL)
 *     exp_avg_sq <- beta2 exp_avg_sq + (1 - beta2) g g                 (both moments formed in float64, rounded once)
 *     p          <- p - a exp_avg / (sqrt(exp_avg_sq) r + eps)
 * 16-byte accesses for a tensor whose param and grad pointers are both 16-byte aligned, 4-byte accesses otherwise (a gradient that is a
 * view into a flat bucket); the flat moment buffers are 16-byte aligned and hold `moment_elems` floats.  Every table entry is checked
 * against its chunk count and `moment_elems` before the launch (WC_ERR_SHAPE / WC_ERR_ARG). */
int wc_adam_update_f32(const wc_adam_table* table, float* exp_avg /*nullable when beta1 == 0*/, float* exp_avg_sq, int64_t moment_elems,
                       const float* record, double beta1, double beta2, float eps, wc_stream_t stream);

/* ==== the ResNet critic's tail and the AC-GAN class loss (scripts/cifar10_resnet_wgan_cond*.sh, --gan_type AC_GAN), DESIGN.md section 4.19 ====
 * Additive like the blocks above: WC_CORE_API keeps its list and WC_ABI_VERSION its value.  Stream-ordered and graph-capturable; nothing
 * allocates or synchronises, no atomics: the same bits on every call.  y [N, HW, C] fp32 NHWC, 16-byte aligned like dy, w_out and w_cls
 * (WC_ERR_ARG otherwise); s = 1 (sum_pool = 1)
 * or 1 / HW (sum_pool = 0); K = 0: no class head (w_cls, b_cls, logits, lse, labels, ce NULL).  Sums in float64, each value rounded once.
 *     feat[n,c]  = s sum_hw relu(y[n,hw,c])        out[n] = feat[n] . w_out + b_out        logits[n,k] = feat[n] . w_cls[k] + b_cls[k]
 *     lse[n]     = log sum_k exp(logits[n,k])  (the row maximum subtracted)                ce[n] = lse[n] - logits[n, labels[n]]
 * labels / ce: both or neither; a label outside [0, K) reads nothing, its ce is NaN and its class gradient zero.  b_out, b_cls nullable (0). */
int wc_critic_tail_supported(int64_t N, int64_t HW, int C, int K);     /* 1 iff N, HW >= 1, 4 <= C <= 1024, C % 4 == 0, 0 <= K <= 1024, N HW C < 2^31 */
int wc_critic_tail_fwd_f32(const float* y, const float* w_out /*[C]*/, const float* b_out /*[1]*/, const float* w_cls /*[K,C]*/,
                           const float* b_cls /*[K]*/, const int32_t* labels /*[N], nullable*/, int64_t N, int64_t HW, int C, int K, int sum_pool,
                           float* feat /*[N,C]*/, float* out /*[N]*/, float* logits /*[N,K]*/, float* lse /*[N]*/, float* ce /*[N], nullable*/,
                           wc_stream_t stream);
/*     dlogits[n,k] = g_logits[n,k] + g_ce[n] (exp(logits[n,k] - lse[n]) - 1[k = labels[n]])         (g_logits, g_ce nullable: zero)
 *     dy[n,hw,c]   = y[n,hw,c] > 0 ? s (g_out[n] w_out[c] + sum_k dlogits[n,k] w_cls[k,c]) : 0
 * y is read once and dy written once; no expanded gradient and no masked copy exist.  logits, lse, labels: the forward's, read with g_ce. */
int wc_critic_tail_bwd_f32(const float* y, const float* w_out, const float* w_cls, const float* g_out /*[N]*/, const float* g_logits /*[N,K]*/,
                           const float* g_ce /*[N]*/, const float* logits, const float* lse, const int32_t* labels, int64_t N, int64_t HW, int C,
                           int K, int sum_pool, float* dlogits /*[N,K]*/, float* dy /*[N,HW,C]*/, wc_stream_t stream);
/*     dw_out[c] = sum_n g_out[n] feat[n,c]    db_out = sum_n g_out[n]    dW_cls[k,c] = sum_n dlogits[n,k] feat[n,c]    db_cls[k] = sum_n dlogits[n,k]
 * summed over n in a fixed order, one thread per weight. */
int wc_critic_tail_wgrad_f32(const float* feat, const float* g_out, const float* dlogits, int64_t N, int C, int K, float* dw_out /*[C]*/,
                             float* db_out /*[1]*/, float* dW_cls /*[K,C]*/, float* db_cls /*[K]*/, wc_stream_t stream);

/* ==== the projection critic's tail (--gan_type PROJECTIVE: out = psi(f) + <emb[cls], f>, discriminator.py:77-82), DESIGN.md section 4.20 ====
 * Additive again: WC_CORE_API and WC_ABI_VERSION stay.  The rules of the block above; emb [K, C] is whatever table the caller holds (the
 * spectral-norm op's output or the Embedding's weight), 16-byte aligned like y, dy and w_out (WC_ERR_ARG otherwise); cls [N] int32.
 *     feat[n,c] = s sum_hw relu(y[n,hw,c])                     out[n] = feat[n] . (w_out + emb[cls[n]]) + b_out           (b_out nullable: 0)
 *     dy[n,hw,c] = y[n,hw,c] > 0 ? s g_out[n] (w_out[c] + emb[cls[n],c]) : 0
 *     dw_out[c] = sum_n g_out[n] feat[n,c]    db_out = sum_n g_out[n]    demb[k,c] = sum_{n : cls[n] = k} g_out[n] feat[n,c]
 * demb is dense and written in full, ascending n within a row; the row of a class no sample carries is exactly 0.  A label outside [0, K)
 * reads nothing: its out is NaN, its dy carries the w_out term alone and it adds to no row of demb. */
int wc_critic_proj_supported(int64_t N, int64_t HW, int C, int K);     /* wc_critic_tail_supported's limits with K >= 1 */
int wc_critic_proj_fwd_f32(const float* y, const float* w_out /*[C]*/, const float* b_out /*[1]*/, const float* emb /*[K,C]*/,
                           const int32_t* cls /*[N]*/, int64_t N, int64_t HW, int C, int K, int sum_pool, float* feat /*[N,C]*/,
                           float* out /*[N]*/, wc_stream_t stream);
int wc_critic_proj_bwd_f32(const float* y, const float* w_out, const float* emb, const int32_t* cls, const float* g_out /*[N]*/, int64_t N,
                           int64_t HW, int C, int K, int sum_pool, float* dy /*[N,HW,C]*/, wc_stream_t stream);
int wc_critic_proj_wgrad_f32(const float* feat, const float* g_out, const int32_t* cls, int64_t N, int C, int K, float* dw_out /*[C]*/,
                             float* db_out /*[1]*/, float* demb /*[K,C]*/, wc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WC_HIP_H */
