// Convolutions around the WC sites (the callers either side of the path -- the 3x3 'same'
// convolutions of generator.py:142-158 / discriminator.py:41-54, their up-/down-sampling forms and the matching
// data gradients), fp32-accurate on the 16-bit MFMA pipe: the same split-operand scheme as the WC apply kernel,
//     x = (xh + xl) / sx,  w = (wh + wl) / sw   (fp16 pairs, power-of-two tensor scales)
//     y = (xl*wh + xh*wl + xh*wh) / (sx*sw)     three v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator
// as an implicit GEMM over (tap, input channel):
//   * M = the points of a "virtual grid" (N, H, W); point (y, x) reads input pixel (y*in_stride + dy_t, x*in_stride + dx_t)
//     for tap t and writes output pixel (y*out_stride + off_y, x*out_stride + off_x).  With up to four "phases" (tap
//     offsets, weights and output offset per phase) one launch covers a 3x3 / 1x1 convolution, a 4x4 stride-2
//     convolution, and a 4x4 stride-2 TRANSPOSED convolution (as four 2x2 sub-pixel convolutions) -- and, with the
//     roles of the channel axes swapped in the weight image, the data gradient of each.
//   * A operand: the activation planes are split once (conv_split_kernel); a workgroup GATHERS its pixels with LDS-DMA
//     (global_load_lds_dwordx4, 16 B per lane from any address) so that each 1-KiB chunk lands in LDS as the register
//     image of one (32 pixels x 16 channels) MFMA fragment: the k-loop reads it back with one conflict-free
//     ds_read_b128 per fragment; zero padding = lanes pointed at a zero line.
//   * B operand: the weights are pre-arranged (conv_weights_kernel) as the same kind of 1-KiB fragment images in
//     (phase, tap, 32-channel chunk, n-block, k-step, hi|lo) order: a plain linear LDS-DMA copy.
//   * a workgroup = 4 waves as 2x2, each wave (32 MB) pixels x (32 NB) outputs with 16 MB NB accumulator registers; one
//     iteration = (tap, 32 input channels) = 2 k-steps; two LDS stages, one barrier per iteration, hand-placed: fragments
//     of k-step 0 right behind the barrier, then the MFMAs with the next iteration's addresses, DMAs and the fragment
//     reads of k-step 1 in their shadow.
//     NB = 1 (128 pixels x 64 outputs) is the tile of a width that is 64 beyond a multiple of 128 (the DC critic's 64-filter layers).
//     A width that is 32 beyond a multiple of 64 (the ImageNet generator's 32-filter block): 128 pixels x 32 outputs, the four waves along
//     the pixels (conv_f16x3_slim_kernel); its weight gradient on 32 x 32 tiles, a wave per pixel range (conv_wrw_slim_kernel).
//   * small grids (< ~100 workgroups) share the (tap, chunk) loop over blockIdx.z (conv_ksplit_reduce_kernel finishes).
//   * weight gradient: conv_wrw_kernel (pixel-major tiles, ds_read_b64_tr_b16 fragments, split over pixel ranges) +
//     conv_wrw_reduce_kernel (fixed-order sum into the weight's layout, 4x4 slices folded back onto 3x3 taps); 256 x 256, 128 x 128 or
//     -- a 64-channel side -- 64 x 64 tiles.
//   * one layer's backward where both gradients run on 128 x 128 tiles (the critic's 128-channel layers): the data gradient's and the
//     weight gradient's workgroups in ONE grid (conv_bwd_pair_kernel) and one launch that finishes both (conv_pair_reduce_kernel) --
//     the kernels' bodies are __device__ functions of the block coordinates, shared with the launches of their own; same bits.
//   * where a k-split's finish was followed by a launch that read its result back only to re-express it (the critic at 8x8), the finish does
//     that work too: the reader's planes, or the block input's gradient (conv_finish_tail_kernel, conv_pair_reduce_tail_kernel); same bits.
//   * where such a k-split has four shares and its 64 x 64 tiles fit the chip one per CU (the critic at 8x8, batch 128), the shares are the
//     four WAVES of a workgroup and meet in LDS: one launch, no partial sums in memory (conv_local_kernel); same bits.
//   * conv(relu(x)) and conv(leaky_relu(x)) apply the activation while x is split (conv_split_*_kernel, split_act).
// MFMA-bound by design: 3 * 2*M*Cout*K flop on the fp16 pipe against 2*M*Cout*K on the fp32 pipe (157 TFLOP/s peak).
#include "wc_common.h"
#include "wc_mask.h"
#include "../../include/wc_hip.h"
#include <stdlib.h>
#include <string.h>


namespace {

constexpr int kMaxTaps = 16, kMaxPhase = 4;

struct ConvArgs {
    const _Float16* xhi; const _Float16* xlo;      // [N][Hin][Win][Cin] each
    const _Float16* zero;                           // >= 64 B of zeros (the padding line)
    const char* wimg;                               // weight fragment images
    const float* xscale; const float* wscale;       // device scalars (powers of two)
    const float* bias;                              // [Cout] or nullptr
    float* y;                                       // [N][Hout][Wout][Cout]
    int N, H, W, Hin, Win, Cin, Cout, in_stride, ntaps, nphase, Hout, Wout, out_stride, relu;
    unsigned magHW, shHW, magW, shW;                // m / (H*W) and rem / W by multiply-shift (m < 2^31)
    int ksplit; float* partial;                     // ksplit > 1: blockIdx.z takes a share of the (tap, chunk) loop, raw sums -> partial[z][output]
    signed char dy[kMaxPhase][kMaxTaps], dx[kMaxPhase][kMaxTaps];
    signed char offy[kMaxPhase], offx[kMaxPhase];
};

__device__ __forceinline__ void lds_dma16(const void* g, unsigned lds)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}

// (the body takes the workgroup's grid coordinates as arguments: conv_bwd_pair_kernel runs it on a range of a linear grid)
// RG: the grid's last tile is partial (N*H*W a multiple of 32, not of 128; conv_f16x3_ragged_kernel).  With RG = false the body is, line
// for line, the one whole-tile grids always ran: their kernels keep their code.
template <int MB, int NB, bool KS, bool RG = false>
__device__ __forceinline__ void conv_f16x3_body(const ConvArgs& a, const unsigned bx, const unsigned by, const unsigned bz)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TM = 64 * MB, TN = 64 * NB;
    constexpr int A_BYTES = 2 * MB * 4 * 1024, B_BYTES = 2 * NB * 4 * 1024, STAGE = A_BYTES + B_BYTES;
    constexpr int AQ = (2 * MB) / 4;               // m-blocks each wave stages
    static_assert(AQ >= 1, "MB >= 2");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = a.Cout / TN;
    const int phase = by / ntn, nt = by - phase * ntn;
    const unsigned m0 = bx * TM;
    const unsigned HW = a.H * a.W;
    const int koff = (lane >> 5) * 8;

    int gy[AQ], gx[AQ];
    unsigned gpix[AQ];                             // input pixel index of (n, 0, 0)
    #pragma unroll
    for (int q = 0; q < AQ; ++q) {
        const unsigned m = m0 + (wave * AQ + q) * 32 + (lane & 31);
        const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        gy[q] = yy * a.in_stride; gx[q] = xx * a.in_stride; gpix[q] = n * (a.Hin * a.Win);
        // a partial last tile: the rows past the grid have n >= N.  Their row coordinate is put where no tap offset (a signed char) brings
        // it back inside [0, Hin), so every tap of theirs fails the test below and reads the zero line -- decided here, once; the loop
        // keeps its code -- and no address is formed from their n
        if constexpr (RG) {
            if (n >= (unsigned)a.N) { gy[q] = -1024; gpix[q] = 0; }
        }
    }
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
    const int nchunk = a.Cin >> 5;
    const int iters = a.ntaps * nchunk;
    const int nblk_all = a.Cout >> 5;

    auto issue = [&](int it, int stage) {
        const int tap = it / nchunk, ch = it - tap * nchunk;
        const int dy = a.dy[phase][tap], dx = a.dx[phase][tap];
        const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
        #pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int iy = gy[q] + dy, ix = gx[q] + dx;
            const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
            const int64_t e = ((int64_t)(gpix[q] + iy * a.Win + ix)) * a.Cin + ch * 32 + koff;
            #pragma unroll
            for (int s = 0; s < 2; ++s) {
                const _Float16* ph = ok ? a.xhi + e + s * 16 : a.zero + koff;
                const _Float16* pl = ok ? a.xlo + e + s * 16 : a.zero + koff;
                const unsigned l = sbase + (((wave * AQ + q) * 2 + s) * 2) * 1024;
                lds_dma16(ph, l);
                lds_dma16(pl, l + 1024);
            }
        }
        const char* wsrc = a.wimg + ((((int64_t)(phase * a.ntaps + tap) * nchunk + ch) * nblk_all + nt * 2 * NB) << 12);
        #pragma unroll
        for (int c = 0; c < 2 * NB; ++c) {
            const int idx = wave * 2 * NB + c;
            lds_dma16(wsrc + idx * 1024 + lane * 16, sbase + A_BYTES + idx * 1024);
        }
    };

    f32x16 acc[MB][NB];
    #pragma unroll
    for (int i = 0; i < MB; ++i)
        #pragma unroll
        for (int j = 0; j < NB; ++j)
            #pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int it0 = KS ? (int)bz * iters / a.ksplit : 0, it1 = KS ? ((int)bz + 1) * iters / a.ksplit : iters;
    // Hand-placed iteration: the fragments of k-step 0 right behind the barrier, then the MFMAs of both k-steps with the
    // next iteration's DMAs (one every GAP MFMAs) and the fragment reads of k-step 1 in their shadow -- the wave issues
    // in order, so whatever stands between the barrier and the first MFMA is time the MFMA pipe idles.
    constexpr int NA = AQ * 4, ND = NA + 2 * NB, HALF = ND / 2, PER = 3 * MB * NB, GAP = PER / HALF;
    static_assert(PER % HALF == 0, "DMAs spread evenly");
    int tabv = 0;                                   // lane t: packed (dy, dx) of tap t of this phase
    if (lane < a.ntaps) tabv = (a.dy[phase][lane] & 0xff) | ((a.dx[phase][lane] & 0xff) << 8);
    const char* pa[AQ][2];                          // next iteration: hi / lo source of this lane's A rows (k-step 0)
    int pstep[AQ];                                  // bytes to k-step 1 (0 on the zero line)
    const char* pw;                                 // next iteration: this lane's first weight chunk
    unsigned sb_next = 0;
    auto prep = [&](int it, int stage) {
        const int tap = it / nchunk, ch = it - tap * nchunk;
        const int p = __builtin_amdgcn_readlane(tabv, tap);
        const int dy = (signed char)(p & 0xff), dx = (signed char)((p >> 8) & 0xff);
        #pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int iy = gy[q] + dy, ix = gx[q] + dx;
            const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
            const int64_t e = ((int64_t)(gpix[q] + iy * a.Win + ix)) * a.Cin + ch * 32 + koff;
            pa[q][0] = reinterpret_cast<const char*>(ok ? a.xhi + e : a.zero + koff);
            pa[q][1] = reinterpret_cast<const char*>(ok ? a.xlo + e : a.zero + koff);
            pstep[q] = ok ? 32 : 0;
        }
        pw = a.wimg + ((((int64_t)(phase * a.ntaps + tap) * nchunk + ch) * nblk_all + nt * 2 * NB) << 12) + wave * (2 * NB * 1024) + lane * 16;
        sb_next = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
    };
    auto dma = [&](int d) {
        if (d < NA) {
            const int q = d >> 2, ks = (d >> 1) & 1, pl = d & 1;
            lds_dma16(pa[q][pl] + ks * pstep[q], sb_next + (((wave * AQ + q) * 2 + ks) * 2 + pl) * 1024);
        } else {
            const int c = d - NA;
            lds_dma16(pw + c * 1024, sb_next + A_BYTES + (wave * 2 * NB + c) * 1024);
        }
    };
    f16x8 fa[2][MB][2], fb[2][NB][2];               // [k-step][block][hi | lo]
    auto frags = [&](int stage, int ks) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + A_BYTES;
        #pragma unroll
        for (int i = 0; i < MB; ++i) {
            const char* p = sa + (((wm * MB + i) * 2 + ks) * 2) * 1024 + lane * 16;
            fa[ks][i][0] = *reinterpret_cast<const f16x8*>(p);
            fa[ks][i][1] = *reinterpret_cast<const f16x8*>(p + 1024);
        }
        #pragma unroll
        for (int j = 0; j < NB; ++j) {
            const char* p = sb + (((wn * NB + j) * 2 + ks) * 2) * 1024 + lane * 16;
            fb[ks][j][0] = *reinterpret_cast<const f16x8*>(p);
            fb[ks][j][1] = *reinterpret_cast<const f16x8*>(p + 1024);
        }
    };
    prep(it0, 0);
    #pragma unroll
    for (int d = 0; d < ND; ++d) dma(d);
    for (int it = it0; it < it1; ++it) {
        const int stage = (it - it0) & 1;
        __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's chunks of the stage have landed
        __syncthreads();                           // ... and everybody's; the other stage is free (its readers are done)
        frags(stage, 0);
        // the last iteration re-fetches its own data into the idle stage: no branch in the loop, nobody reads it
        prep(it + 1 < it1 ? it + 1 : it, stage ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            #pragma unroll
            for (int g = 0; g < PER; ++g) {
                const int prod = g / (MB * NB), i = (g / NB) % MB, j = g % NB;
                // lo*hi, hi*lo, hi*hi
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][i][prod == 0 ? 1 : 0], fb[ks][j][prod == 1 ? 1 : 0], acc[i][j], 0, 0, 0);
                if ((g + 1) % GAP == 0) {
                    dma(ks * HALF + g / GAP);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (ks == 0 && g == PER / 2) {
                    frags(stage, 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);            // the idle stage's last DMAs
    // epilogue: unscale, bias, scatter rows to their output pixels
    const float inv = 1.0f / (a.xscale[0] * a.wscale[0]);
    const int oy0 = a.offy[phase], ox0 = a.offx[phase];
    float bj[NB];
    #pragma unroll
    for (int j = 0; j < NB; ++j) bj[j] = a.bias ? a.bias[nt * TN + (wn * NB + j) * 32 + (lane & 31)] : 0.f;
    #pragma unroll
    for (int i = 0; i < MB; ++i) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const unsigned m = m0 + (wm * MB + i) * 32 + row;
            const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            if constexpr (RG) {
                if (n >= (unsigned)a.N) continue;   // a row past the grid: nothing to write, to y or to the partial sums
            }
            const int64_t opix = ((int64_t)n * a.Hout + (yy * a.out_stride + oy0)) * a.Wout + (xx * a.out_stride + ox0);
            const int64_t oe = opix * a.Cout + nt * TN + wn * NB * 32 + (lane & 31);
            if (KS) {                               // raw partial sums; conv_ksplit_reduce_kernel finishes
                float* o = a.partial + (int64_t)bz * ((int64_t)a.N * a.Hout * a.Wout * a.Cout) + oe;
                #pragma unroll
                for (int j = 0; j < NB; ++j) o[j * 32] = acc[i][j][r];
            } else {
                float* o = a.y + oe;
                #pragma unroll
                for (int j = 0; j < NB; ++j) {
                    float v = acc[i][j][r] * inv + bj[j];
                    if (a.relu) v = fmaxf(v, 0.f);
                    o[j * 32] = v;
                }
            }
        }
    }
}

template <int MB, int NB, bool KS>
__global__ __launch_bounds__(256) void conv_f16x3_kernel(ConvArgs a) { conv_f16x3_body<MB, NB, KS>(a, blockIdx.x, blockIdx.y, blockIdx.z); }

// the same tiles on a grid whose last tile along x is partial (wc_conv_ragged_supported; the 128-point tiles only): a kernel of its own, so
// that the one above keeps its code
template <int NB, bool KS>
__global__ __launch_bounds__(256) void conv_f16x3_ragged_kernel(ConvArgs a) { conv_f16x3_body<2, NB, KS, true>(a, blockIdx.x, blockIdx.y, blockIdx.z); }

// ---- 32-output tiles: a width that is 32 beyond a multiple of 64 (wc_conv_slim_supported; the ImageNet generator's 32-filter block) ----------
// The body above lays its four waves out 2 x 2 and gives the second wave column the tile's outputs 32 NB ... 64 NB - 1: at 32 outputs that
// column has nothing to own, and a masked 64-wide tile would gather, multiply and address twice what exists.  Here the tile is 128 points x
// 32 outputs and the four waves lie ALONG THE POINTS: wave w owns the m-block m0 + 32 w (one 32 x 32 accumulator, 16 registers), stages its
// own rows of A (four 1-KiB fragment images per iteration: 2 k-steps x hi | lo) and one of the four 1-KiB chunks of the single n-block's
// weight fragments, which all four waves read.  The scheme is conv_f16x3_body's -- split operands, three MFMAs into one accumulator,
// LDS-DMA gather with the zero line for padding, two stages, one barrier per (tap, 32-channel chunk) iteration, the next iteration's five
// DMAs between this one's six MFMAs -- and so are the weight image's order (blockIdx.y = phase * (Cout / 32) + n-block), the epilogue's
// row mapping and the k-split's partial sums: a lane's column is n-block * 32 + (lane & 31) < Cout, in y and in the partial sums alike.
// Whole tiles only (N*H*W a multiple of 128): every row of every wave is a point of the grid.  LDS: 2 x (16 + 4) KiB.
template <bool KS>
__global__ __launch_bounds__(256) void conv_f16x3_slim_kernel(ConvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int A_BYTES = 4 * 4 * 1024, B_BYTES = 4 * 1024, STAGE = A_BYTES + B_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntn = a.Cout >> 5;
    const int phase = blockIdx.y / ntn, nt = blockIdx.y - phase * ntn;
    const unsigned m0 = blockIdx.x * 128;
    const unsigned HW = a.H * a.W;
    const int koff = (lane >> 5) * 8;

    int gy, gx;
    unsigned gpix;                                  // input pixel index of (n, 0, 0)
    {
        const unsigned m = m0 + wave * 32 + (lane & 31);
        const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        gy = yy * a.in_stride; gx = xx * a.in_stride; gpix = n * (a.Hin * a.Win);
    }
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
    const int nchunk = a.Cin >> 5;
    const int iters = a.ntaps * nchunk;

    f32x16 acc;
    #pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int it0 = KS ? (int)blockIdx.z * iters / a.ksplit : 0, it1 = KS ? ((int)blockIdx.z + 1) * iters / a.ksplit : iters;
    int tabv = 0;                                   // lane t: packed (dy, dx) of tap t of this phase
    if (lane < a.ntaps) tabv = (a.dy[phase][lane] & 0xff) | ((a.dx[phase][lane] & 0xff) << 8);
    const char* pa[2];                              // next iteration: hi / lo source of this lane's A row (k-step 0)
    int pstep = 0;                                  // bytes to k-step 1 (0 on the zero line)
    const char* pw;                                 // next iteration: this wave's chunk of the weight fragments
    unsigned sb_next = 0;
    auto prep = [&](int it, int stage) {
        const int tap = it / nchunk, ch = it - tap * nchunk;
        const int p = __builtin_amdgcn_readlane(tabv, tap);
        const int dy = (signed char)(p & 0xff), dx = (signed char)((p >> 8) & 0xff);
        const int iy = gy + dy, ix = gx + dx;
        const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
        const int64_t e = ((int64_t)(gpix + iy * a.Win + ix)) * a.Cin + ch * 32 + koff;
        pa[0] = reinterpret_cast<const char*>(ok ? a.xhi + e : a.zero + koff);
        pa[1] = reinterpret_cast<const char*>(ok ? a.xlo + e : a.zero + koff);
        pstep = ok ? 32 : 0;
        pw = a.wimg + ((((int64_t)(phase * a.ntaps + tap) * nchunk + ch) * ntn + nt) << 12) + wave * 1024 + lane * 16;
        sb_next = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
    };
    auto dma = [&](int d) {
        if (d < 4) {
            const int ks = d >> 1, pl = d & 1;
            lds_dma16(pa[pl] + ks * pstep, sb_next + ((wave * 2 + ks) * 2 + pl) * 1024);
        } else {
            lds_dma16(pw, sb_next + A_BYTES + wave * 1024);
        }
    };
    f16x8 fa[2][2], fb[2][2];                       // [k-step][hi | lo]
    auto frags = [&](int stage, int ks) {
        const char* sa = smem + stage * STAGE + ((wave * 2 + ks) * 2) * 1024 + lane * 16;
        const char* sb = smem + stage * STAGE + A_BYTES + (ks * 2) * 1024 + lane * 16;
        fa[ks][0] = *reinterpret_cast<const f16x8*>(sa);
        fa[ks][1] = *reinterpret_cast<const f16x8*>(sa + 1024);
        fb[ks][0] = *reinterpret_cast<const f16x8*>(sb);
        fb[ks][1] = *reinterpret_cast<const f16x8*>(sb + 1024);
    };
    prep(it0, 0);
    #pragma unroll
    for (int d = 0; d < 5; ++d) dma(d);
    for (int it = it0; it < it1; ++it) {
        const int stage = (it - it0) & 1;
        __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): this wave's chunks of the stage have landed
        __syncthreads();                           // ... and everybody's; the other stage is free (its readers are done)
        frags(stage, 0);
        // the last iteration re-fetches its own data into the idle stage: no branch in the loop, nobody reads it
        prep(it + 1 < it1 ? it + 1 : it, stage ^ 1);
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            #pragma unroll
            for (int prod = 0; prod < 3; ++prod) {
                // lo*hi, hi*lo, hi*hi
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][prod == 0 ? 1 : 0], fb[ks][prod == 1 ? 1 : 0], acc, 0, 0, 0);
                if (ks * 3 + prod < 5) {
                    dma(ks * 3 + prod);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (ks == 0 && prod == 1) {
                    frags(stage, 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);            // the idle stage's last DMAs
    // epilogue: unscale, bias, scatter rows to their output pixels
    const float inv = 1.0f / (a.xscale[0] * a.wscale[0]);
    const int oy0 = a.offy[phase], ox0 = a.offx[phase];
    const float bj = a.bias ? a.bias[nt * 32 + (lane & 31)] : 0.f;
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const unsigned m = m0 + wave * 32 + row;
        const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        const int64_t opix = ((int64_t)n * a.Hout + (yy * a.out_stride + oy0)) * a.Wout + (xx * a.out_stride + ox0);
        const int64_t oe = opix * a.Cout + nt * 32 + (lane & 31);
        if (KS) {                                   // raw partial sums; conv_ksplit_reduce_kernel finishes
            a.partial[(int64_t)blockIdx.z * ((int64_t)a.N * a.Hout * a.Wout * a.Cout) + oe] = acc[r];
        } else {
            float v = acc[r] * inv + bj;
            if (a.relu) v = fmaxf(v, 0.f);
            a.y[oe] = v;
        }
    }
}

// ---- small grids: the (tap, chunk) loop split over blockIdx.z; y = (sum of the partial sums) / (sx*sw) + bias ---------
struct KsplitReduceArgs {
    const float* partial; int ksplit; int64_t n4; int cout;
    const float* xscale; const float* wscale; const float* bias; int relu; float* y;
};

// the finished value of float4 i: (sum of the shares in order) * inv + bias (, ReLU) (+ res).  ONE source for every kernel that finishes a
// k-split -- the plain finish below and the finishes that go on to write what the next launch used to read back (conv_finish_split_body,
// conv_finish_dx_body): whether `v * inv` and `+ bias` contract is decided here, for all of them
// SUMMED: the caller has added the shares itself, in this order, and hands the sum in as `v` (conv_local_kernel: its shares meet in LDS);
// the existing callers instantiate the function as it always was
template <bool SUMMED = false>
__device__ __forceinline__ f32x4 conv_ksplit_finish_elem(const float* __restrict__ partial, int ksplit, int64_t n4, int cout, const float inv,
                                                         const float* __restrict__ bias, int relu, const float* __restrict__ res, const int64_t i,
                                                         f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f})
{
    if constexpr (!SUMMED) {
        v = *reinterpret_cast<const f32x4*>(partial + 4 * i);
        int z = 1;
        for (; z + 3 < ksplit; z += 4) {                 // four shares in flight, added in order
            f32x4 t[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = *reinterpret_cast<const f32x4*>(partial + 4 * ((z + u) * n4 + i));
            #pragma unroll
            for (int u = 0; u < 4; ++u) v += t[u];
        }
        for (; z < ksplit; ++z) v += *reinterpret_cast<const f32x4*>(partial + 4 * (z * n4 + i));
    }
    v = v * inv;
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + (4 * i) % cout);
    if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    if (res) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(res + 4 * i);
        #pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fadd_rn(v[j], r[j]);        // (its own rounding: never contracted into the line above)
    }
    return v;
}

// "finish the sum": the second half alone
__device__ __forceinline__ f32x4 conv_ksplit_finish_sum(const f32x4 v, int cout, const float inv, const float* __restrict__ bias, int relu,
                                                        const float* __restrict__ res, const int64_t i)
{
    return conv_ksplit_finish_elem<true>(nullptr, 0, 0, cout, inv, bias, relu, res, i, v);
}

__device__ __forceinline__ void conv_ksplit_reduce_body(const float* __restrict__ partial, int ksplit, int64_t n4, int cout,
                                                        const float* __restrict__ xscale, const float* __restrict__ wscale,
                                                        const float* __restrict__ bias, int relu, float* __restrict__ y,
                                                        const unsigned bid, const unsigned nblocks, const float* __restrict__ res = nullptr)
{
    // res (y's shape, nullable): the residual block's other branch, added to the finished value -- y = (acc * inv + bias) + res, the bits of
    // the elementwise add that used to read y straight back (discriminator.py:41-54 `Add()([h, s])`)
    const float inv = 1.0f / (xscale[0] * wscale[0]);
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < n4; i += (int64_t)nblocks * 256)
        *reinterpret_cast<f32x4*>(y + 4 * i) = conv_ksplit_finish_elem(partial, ksplit, n4, cout, inv, bias, relu, res, i);
}

__global__ __launch_bounds__(256) void conv_ksplit_reduce_kernel(const float* __restrict__ partial, int ksplit, int64_t n4, int cout,
                                                                 const float* __restrict__ xscale, const float* __restrict__ wscale,
                                                                 const float* __restrict__ bias, int relu, float* __restrict__ y)
{
    conv_ksplit_reduce_body(partial, ksplit, n4, cout, xscale, wscale, bias, relu, y, blockIdx.x, gridDim.x);
}

// the same finish with the residual operand (wc_conv_res_f16x3); a kernel of its own, so that the one above keeps its code
__global__ __launch_bounds__(256) void conv_ksplit_reduce_res_kernel(const float* __restrict__ partial, int ksplit, int64_t n4, int cout,
                                                                     const float* __restrict__ xscale, const float* __restrict__ wscale,
                                                                     const float* __restrict__ bias, const float* __restrict__ res,
                                                                     float* __restrict__ y)
{
    conv_ksplit_reduce_body(partial, ksplit, n4, cout, xscale, wscale, bias, 0, y, blockIdx.x, gridDim.x, res);
}

// the activation in front of a split: relu 0 = none, 1 = ReLU, 2 = LeakyReLU (x > 0 ? x : slope * x, one fp32 multiply; Keras's
// LeakyReLU of the DC critic, discriminator.py:59-60)
__device__ __forceinline__ f32x4 split_act(f32x4 v, int relu, float slope)
{
    if (relu == 1) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    else if (relu == 2) {
        #pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : slope * v[j];
    }
    return v;
}

// ---- max |x|: one partial per workgroup (no atomics: deterministic, nothing to clear); the consumers fold the partials ---
constexpr int kAmaxBlocks = 512;

__global__ __launch_bounds__(256) void conv_absmax_kernel(const float* __restrict__ x, int64_t n4, int64_t n, float* __restrict__ partial,
                                                          float* __restrict__ colsum = nullptr, int c4n = 0, float leaky = -1.f)
{
    // leaky >= 0: the maximum of LeakyReLU(x) with that slope (the planes of the leaky split are those of the activated tensor: the same
    // scale as measuring leaky_relu(x) itself); the column sums stay those of x as given
    __shared__ float red[4];
    __shared__ f32x4 red4[256];
    float m = 0.f;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        const f32x4 u = leaky >= 0.f ? split_act(v, 2, leaky) : v;
        m = fmaxf(fmaxf(m, fabsf(u[0])), fmaxf(fabsf(u[1]), fmaxf(fabsf(u[2]), fabsf(u[3]))));
        cs += v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) for (int64_t i = 4 * n4; i < n; ++i) m = fmaxf(m, fabsf(x[i]));
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    if (colsum) red4[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // column sums of a [rows][C] tensor (the bias gradient) while it streams by: a thread always sees the same 4 channels
    // (256 and the grid stride are multiples of C/4); the threads of a channel group meet in LDS, the workgroups' partial
    // rows are added up behind the weight-gradient reduction (conv_wrw_reduce_kernel) in a fixed order
    if (colsum && (int)threadIdx.x < c4n) {
        f32x4 t = red4[threadIdx.x];
        for (int p = threadIdx.x + c4n; p < 256; p += c4n) t += red4[p];
        *reinterpret_cast<f32x4*>(colsum + (int64_t)blockIdx.x * 4 * c4n + 4 * threadIdx.x) = t;
    }
}

// power-of-two scale that puts max|x| into [2^13, 2^14); every thread of a workgroup folds the partials (L2 hits)
__device__ __forceinline__ float scale_of(const float* __restrict__ partial, float mul = 1.0f, int count = kAmaxBlocks)
{
    float amax = 0.f;
    for (int i = threadIdx.x & 63; i < count; i += 64) amax = fmaxf(amax, partial[i]);
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    amax *= mul;
    if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(amax, &e);                        // amax = f * 2^e, f in [0.5, 1)
    return ldexpf(1.0f, 14 - e);
}

// the backward of that LeakyReLU on the data gradient, in place: dx *= (x > 0 ? 1 : slope)
__global__ __launch_bounds__(256) void conv_leaky_bwd_kernel(float* __restrict__ dx, const float* __restrict__ x, int64_t n4, float slope)
{
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 g = *reinterpret_cast<const f32x4*>(dx + 4 * i);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        #pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] : slope * g[j];
        *reinterpret_cast<f32x4*>(dx + 4 * i) = g;
    }
}

// The gradient of a critic block's input in one pass (discriminator.py:41-54: the block is conv(relu(x)) ... + shortcut(pool(x)) or + x):
//     DOWN == false:  out = (x > 0 ? dx1 : 0) + g                              g = the block's output gradient (identity shortcut)
//     DOWN == true:   out = (x > 0 ? dx1 : 0) + 0.25 * ds[n][y / 2][x / 2][c]   ds = the shortcut's data gradient at half resolution
// i.e. threshold_backward, the 2x2 average pooling's backward and the add that joins them, with their bits: the masked-out value is +0,
// a NaN in x lets the gradient through (x <= 0 is false), 0.25 * ds is rounded on its own and the sum once.  c4 = C / 4, W, H of dx1.
// (one source for the expression: conv_finish_dx_body applies it to a data gradient it has just finished)
template <bool DOWN>
__device__ __forceinline__ f32x4 conv_block_dx_elem(const f32x4 d, const f32x4 a, const f32x4 o)
{
    f32x4 r;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float m = a[k] <= 0.f ? 0.f : d[k];
        // (the pooling's backward accumulates its one term onto +0: a -0 quarter leaves it as +0)
        r[k] = __fadd_rn(m, DOWN ? __fadd_rn(0.f, __fmul_rn(0.25f, o[k])) : o[k]);
    }
    return r;
}

template <bool DOWN>
__global__ __launch_bounds__(256) void conv_block_dx_kernel(const float* __restrict__ dx1, const float* __restrict__ x,
                                                            const float* __restrict__ other, int64_t n4, int c4, int W, int H,
                                                            float* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(dx1 + 4 * i);
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + 4 * i);
        int64_t j = i;
        if (DOWN) {
            const int64_t pix = i / c4;
            const int c = (int)(i - pix * c4);
            const int64_t row = pix / W;
            const int xx = (int)(pix - row * W);
            const int64_t n = row / H;
            const int yy = (int)(row - n * H);
            j = ((n * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1)) * c4 + c;
        }
        const f32x4 o = *reinterpret_cast<const f32x4*>(other + 4 * j);
        *reinterpret_cast<f32x4*>(out + 4 * i) = conv_block_dx_elem<DOWN>(d, a, o);
    }
}

// ---- activation split: hi = fp16(x*s), lo = fp16(x*s - hi), optional ReLU first ------------------------------------
__global__ __launch_bounds__(256) void conv_split_kernel(const float* __restrict__ x, int64_t n4, const float* __restrict__ amax,
                                                         int relu, _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                         float* __restrict__ scale_out, float slope = 0.f)
{
    const float s = scale_of(amax);
    if (blockIdx.x == 0 && threadIdx.x == 0) scale_out[0] = s;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        v = split_act(v, relu, slope);
        v = v * s;
        f16x4 h, l;
        #pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = (_Float16)v[j]; l[j] = (_Float16)(v[j] - (float)h[j]); }
        *reinterpret_cast<f16x4*>(hi + 4 * i) = h;
        *reinterpret_cast<f16x4*>(lo + 4 * i) = l;
    }
}

// ---- the same split in ONE launch, its scale taken from the call before (round 5) ----------------------------------------------------
// conv_absmax + conv_split run ~240 times per G+D step on the critic's small tensors: two latency-bound launches of 3-8 us each for a
// pass whose only purpose is one number, the tensor's scale -- and hi + lo carry 22 bits of an element wherever the scaled maximum lies
// between 2^-5 and fp16's 65504 (an absolute error of 2^-25 / scaled-max of the tensor's maximum below that): twenty binary orders of
// slack.  So a call site (one convolution's input, or its output gradient) keeps a small record across calls: TWO arrays of kAmaxBlocks
// (maximum, tag) pairs, one pair per workgroup.  A launch writes all pairs of one array with one tag; an array whose tags are all equal
// is COMPLETE.  Every workgroup starts by reading both arrays, takes the complete array with the larger tag -- what the previous call
// left -- and its maximum: the scale is the power of two that puts 64 x that maximum into [2^13, 2^14), i.e. the maximum itself into
// [2^7, 2^8): room for a 255-fold growth from one call to the next before fp16 overflows, a 4000-fold shrink before the absolute
// error leaves 2^-20 of the maximum.  At its end it writes (its own maximum, that tag + 1) into its pair of the OTHER array.  While the
// launch runs, the other array is a mixture of old and new tags (or still looks old through another XCD's L2): never complete with a
// larger tag, so a workgroup that starts late makes the same choice as one that started first -- no atomics, no fences, no counters,
// nothing to clear, and no host-side state beyond "has this site been called": the record is a function of the sequence of tensors
// alone, an eager run and a replayed hipGraph of the same calls produce the same bits.  (Two forms with an arrival counter were
// measured first: with a __threadfence every workgroup waits for its plane stores to reach memory, 15.8 us minimum per launch; with
// relaxed device-scope atomics the 1024 operations on one cache line serialise, 15.4 us against 7.1 for both launches of the measuring
// form at 128x4x4x256.)  NOTHING clamps: an element that does not fit becomes inf in the planes and NaN / inf in the convolution's
// output -- loud, never quietly wrong.  The first call of a site measures (the two-launch form) and seeds the record.
// (csrc/wc_gp.hip restates this record protocol -- seed, history split, gated second pass, these constants -- around a two-tensor load:
// change both; tests/test_penalty_gpu.py compares the planes, the scales and the records bit for bit)
constexpr float kHistMargin = 64.0f;
constexpr int kHistArray = 2 * kAmaxBlocks;         // floats per array: (maximum, tag) per workgroup

__device__ __forceinline__ float scale_for(float amax)
{
    if (!(amax > 0.f) || !(amax < 3.0e38f)) return 1.0f;
    int e;
    (void)frexpf(amax, &e);
    return ldexpf(1.0f, 14 - e);
}

// the first call: conv_absmax_kernel's per-workgroup maxima (in the first kAmaxBlocks floats) -> array 0 with tag 1, array 1 with tag 0
__global__ __launch_bounds__(kAmaxBlocks) void conv_hist_seed_kernel(float* __restrict__ hist)
{
    const float m = hist[threadIdx.x];
    __syncthreads();
    typedef float f32x2h __attribute__((ext_vector_type(2)));
    f32x2h a = {m, __builtin_bit_cast(float, 1u)}, b = {0.f, __builtin_bit_cast(float, 0u)};
    *reinterpret_cast<f32x2h*>(hist + 2 * threadIdx.x) = a;
    *reinterpret_cast<f32x2h*>(hist + kHistArray + 2 * threadIdx.x) = b;
    // the carried maximum (round 6: what a call falls back on when the call before saw an all-zero tensor), both parities
    __shared__ float red[kAmaxBlocks / 64];
    float mm = m;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mm;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < kAmaxBlocks / 64; ++i) t = fmaxf(t, red[i]);
        hist[2 * kHistArray + 2] = t; hist[2 * kHistArray + 3] = t;
    }
}

// The record's protocol and the split's per-element work as __device__ pieces: conv_split_hist_kernel and the k-split finishes that write
// their reader's planes (conv_finish_split_body) are put together from the same ones, so a launch of either kind leaves the planes, the
// scale word, the pairs and the carried maximum that the other would have left.
struct HistPick { int src, tag; float s; };

// pick: the complete array with the larger tag -> the scale of this call; workgroup 0 leaves the scale and the maximum it assumed
__device__ __forceinline__ HistPick conv_hist_pick(float* __restrict__ hist, float* __restrict__ scale_out, const unsigned bid)
{
    // every wave folds both arrays: the maximum and the smallest / largest tag of each (tags as int: __shfl_xor has no unsigned form --
    // an unsigned argument travels as a float and comes back rounded)
    typedef int i32x2h __attribute__((ext_vector_type(2)));
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
    // the complete array with the larger tag (one of the two always is: the launch in flight writes the other one)
    const int src = (ok1 && (!ok0 || thi[1] > thi[0])) ? 1 : 0;
    const int tag = (src ? thi[1] : thi[0]) + 1;
    // Round 6: an all-zero tensor says nothing about the next one (a hinge critic whose margins are all met hands back exactly-zero
    // gradients; round 5 then split the next tensor with scale 1.0, whatever it held).  The site's scale stays where it was instead: every
    // call leaves the maximum it ASSUMED in a word of the record (one per array parity: this call reads the one the call before wrote).
    const float prev = src ? mx[1] : mx[0];
    const float assumed = prev > 0.f ? prev : hist[2 * kHistArray + 2 + src];
    const float s = scale_for(assumed * kHistMargin);
    if (bid == 0 && threadIdx.x == 0) { scale_out[0] = s; hist[2 * kHistArray + 2 + (1 - src)] = assumed; }
    return HistPick{src, tag, s};
}

// one float4 of the (activated) tensor: its part of the workgroup's maximum, its two plane entries
__device__ __forceinline__ float conv_split_elem(f32x4 v, float m, const float s, _Float16* __restrict__ hi, _Float16* __restrict__ lo, const int64_t i)
{
    m = fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    v = v * s;
    f16x4 h, l;
    #pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = (_Float16)v[j]; l[j] = (_Float16)(v[j] - (float)h[j]); }
    *reinterpret_cast<f16x4*>(hi + 4 * i) = h;
    *reinterpret_cast<f16x4*>(lo + 4 * i) = l;
    return m;
}

// publish: the workgroup's (maximum, tag) pair into the OTHER array, its partial row of the column sums
__device__ __forceinline__ void conv_hist_publish(float m, const f32x4 cs, const HistPick pk, float* __restrict__ hist, float* __restrict__ colsum,
                                                  int c4n, const unsigned bid, float* red, f32x4* red4)
{
    typedef float f32x2h __attribute__((ext_vector_type(2)));
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    if (colsum) red4[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x == 0) {
        const f32x2h p = {fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), __builtin_bit_cast(float, pk.tag)};
        *reinterpret_cast<f32x2h*>(hist + (1 - pk.src) * kHistArray + 2 * bid) = p;       // one 8-byte store: the pair is never torn
    }
    if (colsum && (int)threadIdx.x < c4n) {
        f32x4 t = red4[threadIdx.x];
        for (int p = threadIdx.x + c4n; p < 256; p += c4n) t += red4[p];
        *reinterpret_cast<f32x4*>(colsum + (int64_t)bid * 4 * c4n + 4 * threadIdx.x) = t;
    }
}

__global__ __launch_bounds__(256) void conv_split_hist_kernel(const float* __restrict__ x, int64_t n4, int relu, _Float16* __restrict__ hi,
                                                              _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                              float* __restrict__ hist, float* __restrict__ colsum, int c4n,
                                                              float slope = 0.f)
{
    __shared__ float red[4];
    __shared__ f32x4 red4[256];
    const HistPick pk = conv_hist_pick(hist, scale_out, blockIdx.x);
    float m = 0.f;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        cs += v;                                   // (the bias gradient's column sums are of the tensor as given, as in conv_absmax_kernel)
        v = split_act(v, relu, slope);
        m = conv_split_elem(v, m, pk.s, hi, lo, i);
    }
    conv_hist_publish(m, cs, pk, hist, colsum, c4n, blockIdx.x, red, red4);
}

// ---- a k-split's finish that goes on to do what the next launch did (the critic at 8x8: conv._CriticBlock) ----------------------------------
// The convolutions of the critic's 128-channel blocks at 8x8 (and the DOWN block's conv2) share their tap loop over workgroups; an
// elementwise launch sums the shares and writes fp32 -- and the very next launch read that tensor back only to re-express it: as the next
// convolution's fp16 planes, or, with the block's other branch, as the block input's gradient.  4 MiB streams in under 2 us; each of
// these launches costs 4-8 us on a dependent chain.  Here the finish does the follower's work on the value it holds:
//   SPLIT   (forward)   y = finish(+ res) in fp32 AND the planes of relu(y) for the convolution that reads it: conv1's finish -> conv2's
//                       input, conv2's finish (with the residual) -> the next block's conv1 input.  y stays (masks, hooks, the shortcut).
//   MASKED  (backward)  dh = finish in fp32 AND the planes of dh * (h > 0) for conv1's backward, with the bias gradient's partial rows of
//                       the masked values (gp_split_hist_kernel's work, csrc/wc_gp.hip; wc_mask.h holds the shared expressions).
//   DX      (backward)  out = (x > 0 ? finish : 0) + other, the SAME block's input gradient: conv1's data gradient never reaches memory.
// SPLIT and MASKED run on kAmaxBlocks workgroups, as the split kernels always do: workgroup b owns pair b of the reader's record and row
// b of the partial rows, thread t visits the float4s the split's thread t visited, in its order -- the finish is a function of the
// element alone, so regridding it changes nothing.  Every expression comes from the function the two-launch route calls: same bits.
enum { kTailSplit = 1, kTailMasked = 2, kTailDx = 3 };
struct FinishTailArgs {
    KsplitReduceArgs k;                             // the finish (k.y: the fp32 output of SPLIT and MASKED; unused by DX)
    const float* res;                               // SPLIT: the residual operand (nullable)
    const float* mask;                              // MASKED: conv1's output h; DX: the block input x
    const float* other;                             // DX: the block's output gradient
    float* out;                                     // DX: the block input's gradient
    _Float16* hi; _Float16* lo; float* scale_out; float* hist;      // SPLIT, MASKED: the reader's planes, scale word and record
    float* colsum; int c4n;                         // MASKED: the partial rows (nullable)
};

template <bool MASKED>
__device__ __forceinline__ void conv_finish_split_body(const FinishTailArgs& a, const unsigned bid)
{
    __shared__ float red[4];
    __shared__ f32x4 red4[256];
    const HistPick pk = conv_hist_pick(a.hist, a.scale_out, bid);
    const float inv = 1.0f / (a.k.xscale[0] * a.k.wscale[0]);
    float m = 0.f;
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = bid * 256 + threadIdx.x; i < a.k.n4; i += (int64_t)kAmaxBlocks * 256) {
        f32x4 v = conv_ksplit_finish_elem(a.k.partial, a.k.ksplit, a.k.n4, a.k.cout, inv, a.k.bias, a.k.relu, a.res, i);
        *reinterpret_cast<f32x4*>(a.k.y + 4 * i) = v;
        if (MASKED) {
            v = wc_mask_apply(v, *reinterpret_cast<const f32x4*>(a.mask + 4 * i), 0.f);
            cs = wc_colsum_add(cs, v);
        } else {
            v = split_act(v, 1, 0.f);
        }
        m = conv_split_elem(v, m, pk.s, a.hi, a.lo, i);
    }
    conv_hist_publish(m, cs, pk, a.hist, MASKED ? a.colsum : nullptr, a.c4n, bid, red, red4);
}

__device__ __forceinline__ void conv_finish_dx_body(const FinishTailArgs& a, const unsigned bid, const unsigned nblocks)
{
    const float inv = 1.0f / (a.k.xscale[0] * a.k.wscale[0]);
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < a.k.n4; i += (int64_t)nblocks * 256) {
        const f32x4 d = conv_ksplit_finish_elem(a.k.partial, a.k.ksplit, a.k.n4, a.k.cout, inv, a.k.bias, a.k.relu, nullptr, i);
        const f32x4 x = *reinterpret_cast<const f32x4*>(a.mask + 4 * i);
        const f32x4 o = *reinterpret_cast<const f32x4*>(a.other + 4 * i);
        *reinterpret_cast<f32x4*>(a.out + 4 * i) = conv_block_dx_elem<false>(d, x, o);
    }
}

template <int KIND>
__device__ __forceinline__ void conv_finish_tail_body(const FinishTailArgs& a, const unsigned bid, const unsigned nblocks)
{
    if (KIND == kTailDx) conv_finish_dx_body(a, bid, nblocks);
    else conv_finish_split_body<KIND == kTailMasked>(a, bid);
}

template <int KIND>
__global__ __launch_bounds__(256) void conv_finish_tail_kernel(FinishTailArgs a) { conv_finish_tail_body<KIND>(a, blockIdx.x, gridDim.x); }

// ---- the history-scaled split's gated second pass (round 6) ---------------------------------------------------------------------------
// The launch above trusts the previous call's maximum.  Three things can make that wrong: the previous tensor was all zero (nothing to
// go by: a saturated hinge loss gives the critic exactly-zero gradients), the tensor grew more than 255-fold (inf in the planes), or it
// shrank more than 4096-fold (the lo plane sinks into fp16's subnormals: fewer than 20 bits of the maximum, quietly).  This launch
// follows the split on the same stream: both arrays of the record are complete and at rest now -- the one with the larger tag holds the
// maximum of THIS tensor, the other one what the split assumed -- so every workgroup reaches the same verdict from the same 8 KB
// without a flag, a fence or a counter: inside the window it returns (the usual case: a launch of ~2 us that reads 8 KB), outside it
// splits the tensor again with the measured scale, exactly as conv_split_kernel would have (same bits as the two-launch form).
// hist[WC_CONV_HIST_REDO] counts the second passes taken (tests, long-run logs).  Capturable; no host synchronisation.
constexpr int kHistRedoWord = 2 * kHistArray;
__global__ __launch_bounds__(256) void conv_split_redo_kernel(const float* __restrict__ x, int64_t n4, int relu, _Float16* __restrict__ hi,
                                                              _Float16* __restrict__ lo, float* __restrict__ scale_out,
                                                              float* __restrict__ hist, float slope = 0.f)
{
    typedef int i32x2h __attribute__((ext_vector_type(2)));
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
    const float own = mx[now], assumed = hist[2 * kHistArray + 2 + now];       // (what the split assumed: it left the value here)
    const float s_used = scale_for(assumed * kHistMargin);
    const float top = own * s_used;                // the scaled maximum the planes were written with
    // (a NaN maximum never reaches here: fmaxf drops NaN operands; a tensor holding inf has own = inf -> no finite scale exists, leave it loud)
    const bool fine = !(own > 0.f) || !(own < 3.0e38f) || (top >= 0.03125f && top < 65504.0f);
    if (fine) return;
    const float s = scale_for(own);                // the measured form's scale: the maximum into [2^13, 2^14)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scale_out[0] = s;
        reinterpret_cast<unsigned*>(hist)[kHistRedoWord] += 1u;
    }
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        v = split_act(v, relu, slope);
        v = v * s;
        f16x4 h, l;
        #pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = (_Float16)v[j]; l[j] = (_Float16)(v[j] - (float)h[j]); }
        *reinterpret_cast<f16x4*>(hi + 4 * i) = h;
        *reinterpret_cast<f16x4*>(lo + 4 * i) = l;
    }
}

// ---- a k-split whose shares meet inside the workgroup (wc_conv_local_f16x3: the critic's 128-channel layers at 8x8, k-split 4) ----------------
// conv_f16x3_kernel<2, 2, true> gives share z of the (tap, chunk) loop to blockIdx.z: 4 x 4 MiB of raw sums go to memory and a second launch
// reads them back.  Here the tensor is cut into 64-point x 64-output tiles, one workgroup each (256 at the critic's shape: one per CU), and
// WAVE z computes the whole tile over share z: the four accumulators meet in LDS, are added in share order ((p0 + p1) + p2) + p3 and the
// workgroup finishes the values itself (conv_ksplit_finish_sum: conv_ksplit_finish_elem's second half) and goes on to the tail's work with
// the functions the finish launches call -- no workspace, no second launch, nothing between workgroups.  Same bits: a wave's accumulator
// element sees the products of conv_f16x3_body<2, 2, true>'s -- iterations [z iters / 4, (z + 1) iters / 4) ascending, k-step 0 then 1,
// lo*hi, hi*lo, hi*hi -- through the same fragment images, so it holds that kernel's partial sum; the tile shape does not enter.
// Staging is private to the wave (2 stages x 16 KiB: A = 2 m-blocks, B = 2 n-blocks, each x 2 k-steps x hi | lo; 128 KiB per workgroup),
// so the loop has NO workgroup barrier, only the wave's own counted vmcnt waits (LDS-DMAs retire in issue order): a pipeline of half
// iterations -- while the MFMAs of k-step h run, the 8 DMAs of k-step h + 2 go out between them (into the 1-KiB slots k-step h - 2 was
// read from during k-step h - 3) and, once 6 of them are out, vmcnt(6) says k-step h + 1 has landed and its fragments are read.
// SPLIT / MASKED: workgroup b writes the pairs b, b + G, ... of the reader's record with its own maximum (conv_fwd_narrow_split_kernel's
// idiom): the record folds to the same maximum, so the next call takes the same scale.  MASKED without partial rows only: another
// assignment of elements to the 512 rows would change the bias gradient's summation order (the host refuses).
enum { kTailNone = 0 };
constexpr int kLocalWaveBytes = 32 * 1024;          // a wave's two stages; after the loop its 64 x 64 accumulator image (64 x kLocalLd floats)
constexpr int kLocalLd = 64 + 4;                    // floats per row of that image (16-byte aligned rows, the lane halves 16 banks apart)

template <int KIND>
__global__ __launch_bounds__(256) void conv_local_kernel(ConvArgs a, FinishTailArgs f)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int A_BYTES = 8 * 1024, STAGE = 16 * 1024;
    constexpr bool PLANES = KIND == kTailSplit || KIND == kTailMasked;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // = the share z
    const int ntn = a.Cout >> 6;
    const int phase = blockIdx.y / ntn, nt = blockIdx.y - phase * ntn;
    const unsigned m0 = blockIdx.x * 64;
    const unsigned HW = a.H * a.W;
    const int koff = (lane >> 5) * 8;
    [[maybe_unused]] const unsigned bid = blockIdx.y * gridDim.x + blockIdx.x;

    int gy[2], gx[2];
    unsigned gpix[2];                               // input pixel index of (n, 0, 0)
    #pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned m = m0 + q * 32 + (lane & 31);
        const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        gy[q] = yy * a.in_stride; gx[q] = xx * a.in_stride; gpix[q] = n * (a.Hin * a.Win);
    }
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem) + wave * kLocalWaveBytes;
    const char* const wbase = smem + wave * kLocalWaveBytes;
    const int nchunk = a.Cin >> 5;
    const int iters = a.ntaps * nchunk;
    const int nblk_all = a.Cout >> 5;

    f32x16 acc[2][2];
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < 2; ++j)
            #pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int it0 = wave * iters / 4, it1 = (wave + 1) * iters / 4;
    int tabv = 0;                                   // lane t: packed (dy, dx) of tap t of this phase
    if (lane < a.ntaps) tabv = (a.dy[phase][lane] & 0xff) | ((a.dx[phase][lane] & 0xff) << 8);
    const char* pa[2][2];                           // next iteration: hi / lo source of this lane's A rows (k-step 0)
    int pstep[2];                                   // bytes to k-step 1 (0 on the zero line)
    const char* pw;                                 // next iteration: this lane's 16 bytes of the first weight chunk
    unsigned sb_next = 0;
    auto prep = [&](int it, int stage) {
        const int tap = it / nchunk, ch = it - tap * nchunk;
        const int p = __builtin_amdgcn_readlane(tabv, tap);
        const int dy = (signed char)(p & 0xff), dx = (signed char)((p >> 8) & 0xff);
        #pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int iy = gy[q] + dy, ix = gx[q] + dx;
            const bool ok = (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
            const int64_t e = ((int64_t)(gpix[q] + iy * a.Win + ix)) * a.Cin + ch * 32 + koff;
            pa[q][0] = reinterpret_cast<const char*>(ok ? a.xhi + e : a.zero + koff);
            pa[q][1] = reinterpret_cast<const char*>(ok ? a.xlo + e : a.zero + koff);
            pstep[q] = ok ? 32 : 0;
        }
        pw = a.wimg + ((((int64_t)(phase * a.ntaps + tap) * nchunk + ch) * nblk_all + nt * 2) << 12) + lane * 16;
        sb_next = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
    };
    // DMA d of an iteration: k-step d >> 3 first; inside a k-step the rows' four chunks (m-block, hi | lo), then the weights' four
    // (n-block, hi | lo) -- the chunk order of the fragment images, so a k-step's eight DMAs are all that k-step's fragment reads need
    auto dma = [&](int d) {
        const int ks = d >> 3, e = d & 7;
        if (e < 4) {
            const int q = e >> 1, pl = e & 1;
            lds_dma16(pa[q][pl] + ks * pstep[q], sb_next + ((q * 2 + ks) * 2 + pl) * 1024);
        } else {
            const int idx = (((e - 4) >> 1) * 2 + ks) * 2 + (e & 1);
            lds_dma16(pw + idx * 1024, sb_next + A_BYTES + idx * 1024);
        }
    };
    f16x8 fa[2][2][2], fb[2][2][2];                 // [k-step][block][hi | lo]
    auto frags = [&](int stage, int ks) {
        const char* sa = wbase + stage * STAGE + lane * 16;
        const char* sb = sa + A_BYTES;
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            const char* p = sa + ((i * 2 + ks) * 2) * 1024;
            fa[ks][i][0] = *reinterpret_cast<const f16x8*>(p);
            fa[ks][i][1] = *reinterpret_cast<const f16x8*>(p + 1024);
        }
        #pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* p = sb + ((j * 2 + ks) * 2) * 1024;
            fb[ks][j][0] = *reinterpret_cast<const f16x8*>(p);
            fb[ks][j][1] = *reinterpret_cast<const f16x8*>(p + 1024);
        }
    };
    prep(it0, 0);
    #pragma unroll
    for (int d = 0; d < 16; ++d) dma(d);
    // (the record's 8 KB are read behind the first stage's DMAs: one wait covers both)
    [[maybe_unused]] HistPick pk = {0, 0, 1.0f};
    if constexpr (PLANES) pk = conv_hist_pick(f.hist, f.scale_out, bid);
    __builtin_amdgcn_s_waitcnt(0x0F78);            // vmcnt(8): k-step 0 of the first iteration has landed
    frags(0, 0);
    for (int it = it0; it < it1; ++it) {
        const int stage = (it - it0) & 1;
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            #pragma unroll
            for (int g = 0; g < 12; ++g) {
                const int prod = g >> 2, i = (g >> 1) & 1, j = g & 1;
                // lo*hi, hi*lo, hi*hi
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][i][prod == 0 ? 1 : 0], fb[ks][j][prod == 1 ? 1 : 0], acc[i][j], 0, 0, 0);
                if (ks == 0 && g == 0) {
                    // the last iteration re-fetches its own data into the idle stage: no branch in the loop, nobody uses it
                    prep(it + 1 < it1 ? it + 1 : it, stage ^ 1);
                }
                if (g % 3 != 2) {
                    dma(ks * 8 + g - g / 3);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (g == 7) {
                    __builtin_amdgcn_s_waitcnt(0x0F76);        // vmcnt(6): all but this half's six DMAs -- the next k-step has landed
                    if (ks == 0) frags(stage, 1);
                    else frags(stage ^ 1, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);            // the idle stage's last DMAs: the wave's LDS is its own to overwrite
    // the wave's 64 x 64 accumulator -> its own LDS, rows = points, columns = outputs of the tile
    {
        float* tl = reinterpret_cast<float*>(smem + wave * kLocalWaveBytes);
        #pragma unroll
        for (int i = 0; i < 2; ++i)
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                #pragma unroll
                for (int j = 0; j < 2; ++j) tl[row * kLocalLd + j * 32 + (lane & 31)] = acc[i][j][r];
            }
    }
    __syncthreads();
    // finish: thread t takes the float4 (row t / 16 + 16 k, columns 4 (t % 16) ..) of the tile, k = 0..3: a 256-byte row of y per 16 lanes
    const float inv = 1.0f / (a.xscale[0] * a.wscale[0]);
    const int oy0 = a.offy[phase], ox0 = a.offx[phase];
    [[maybe_unused]] float amax = 0.f;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int row = (tid >> 4) + 16 * k;
        const float* p = reinterpret_cast<const float*>(smem) + row * kLocalLd + 4 * (tid & 15);
        f32x4 v = *reinterpret_cast<const f32x4*>(p);
        #pragma unroll
        for (int z = 1; z < 4; ++z) v += *reinterpret_cast<const f32x4*>(p + z * (kLocalWaveBytes / 4));      // ((p0 + p1) + p2) + p3
        const unsigned m = m0 + row;
        const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        const int64_t opix = ((int64_t)n * a.Hout + (yy * a.out_stride + oy0)) * a.Wout + (xx * a.out_stride + ox0);
        const int64_t i4 = (opix * a.Cout + nt * 64 + 4 * (tid & 15)) >> 2;
        v = conv_ksplit_finish_sum(v, f.k.cout, inv, f.k.bias, f.k.relu, KIND == kTailSplit || KIND == kTailNone ? f.res : nullptr, i4);
        if constexpr (KIND == kTailDx) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(f.mask + 4 * i4);
            const f32x4 o = *reinterpret_cast<const f32x4*>(f.other + 4 * i4);
            *reinterpret_cast<f32x4*>(f.out + 4 * i4) = conv_block_dx_elem<false>(v, x, o);
        } else {
            *reinterpret_cast<f32x4*>(f.k.y + 4 * i4) = v;
            if constexpr (KIND == kTailMasked) v = wc_mask_apply(v, *reinterpret_cast<const f32x4*>(f.mask + 4 * i4), 0.f);
            if constexpr (KIND == kTailSplit) v = split_act(v, 1, 0.f);
            if constexpr (PLANES) amax = conv_split_elem(v, amax, pk.s, f.hi, f.lo, i4);
        }
    }
    if constexpr (PLANES) {
        // publish (conv_hist_publish's fold and 8-byte store): the workgroup's pairs of the OTHER array
        typedef float f32x2h __attribute__((ext_vector_type(2)));
        __shared__ float red[4];
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        if (lane == 0) red[wave] = amax;
        __syncthreads();
        const f32x2h pr = {fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), __builtin_bit_cast(float, pk.tag)};
        const unsigned G = gridDim.x * gridDim.y;
        for (unsigned pair = bid + tid * G; pair < (unsigned)kAmaxBlocks; pair += 256u * G)
            *reinterpret_cast<f32x2h*>(f.hist + (1 - pk.src) * kHistArray + 2 * pair) = pr;
    }
}

// ---- weight fragment images ----------------------------------------------------------------------------------------
struct WeightArgs {
    const float* w; int64_t sk, sn, sr, ss;        // element (k, n, r, s) of the source = w[k*sk + n*sn + r*sr + s*ss]
    const float* amax; float* scale_out; char* img;
    int K, Nn, ntaps, nphase;                      // K = reduction channels, Nn = output channels of the product
    int64_t n4;                                    // amax == nullptr: float4s of the whole tensor
    float coef, bound_mul;                         // slice = coef * sum of its sources; max|slice| <= bound_mul * max|w|
    int amax_count;                                // floats behind amax
    signed char nsrc[kMaxPhase][kMaxTaps];
    signed char r[kMaxPhase][kMaxTaps][4], s[kMaxPhase][kMaxTaps][4];
};

__device__ __forceinline__ void conv_weights_body(const WeightArgs& a, const int bid, const int nblocks)
{
    float sc;
    if (a.amax) sc = scale_of(a.amax, a.bound_mul, a.amax_count);
    else {
        // small tensors: every workgroup takes the maximum of the whole (L2-resident) tensor itself -- no separate pass
        __shared__ float red[4];
        float m = 0.f;
        for (int64_t i = threadIdx.x; i < a.n4; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.w + 4 * i);
            m = fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
        #pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * a.bound_mul;
        sc = 1.0f;
        if (m > 0.f && m < 3.0e38f) { int e; (void)frexpf(m, &e); sc = ldexpf(1.0f, 14 - e); }
    }
    if (bid == 0 && threadIdx.x == 0) a.scale_out[0] = sc;
    const int nchunk = a.K >> 5, nblk = a.Nn >> 5;
    const int64_t groups = (int64_t)a.nphase * a.ntaps * nchunk * nblk * 2 * 64;       // one (hi, lo) pair of 16-B lane chunks each
    for (int64_t g = (int64_t)bid * 256 + threadIdx.x; g < groups; g += (int64_t)nblocks * 256) {
        const int lane = g & 63;
        int64_t t = g >> 6;
        const int ks = t & 1; t >>= 1;
        const int nb = t % nblk; t /= nblk;
        const int ch = t % nchunk; t /= nchunk;
        const int tap = t % a.ntaps; const int ph = t / a.ntaps;
        const int n = nb * 32 + (lane & 31);
        const int k0 = ch * 32 + ks * 16 + (lane >> 5) * 8;
        const float* base = a.w + n * a.sn;
        const int ns = a.nsrc[ph][tap];
        float acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < ns; ++m) {
            const float* src = base + a.r[ph][tap][m] * a.sr + a.s[ph][tap][m] * a.ss;
            #pragma unroll
            for (int j = 0; j < 8; ++j) acc8[j] += src[(k0 + j) * a.sk];
        }
        const float cs = a.coef * sc;
        f16x8 h, l;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = acc8[j] * cs;
            h[j] = (_Float16)v; l[j] = (_Float16)(v - (float)h[j]);
        }
        char* dst = a.img + (((((int64_t)(ph * a.ntaps + tap) * nchunk + ch) * nblk + nb) * 2 + ks) * 2) * 1024 + lane * 16;
        *reinterpret_cast<f16x8*>(dst) = h;
        *reinterpret_cast<f16x8*>(dst + 1024) = l;
    }
}

__global__ __launch_bounds__(256) void conv_weights_kernel(WeightArgs a) { conv_weights_body(a, blockIdx.x, gridDim.x); }

// the forward image and the data-gradient image of one weight in ONE launch (same source, same scale, other geometry)
__global__ __launch_bounds__(256) void conv_weights_pair_kernel(WeightArgs a, WeightArgs b, int blocks_a)
{
    if ((int)blockIdx.x < blocks_a) conv_weights_body(a, blockIdx.x, blocks_a);
    else conv_weights_body(b, blockIdx.x - blocks_a, gridDim.x - blocks_a);
}

// ---- the images of MANY weights in one grid (wc_conv_weights_batch_f32) -----------------------------------------------------------------
// A pass's images depend on its weights only, so they need not sit one launch each between a layer's split and its convolution.  The
// role of a workgroup is a range of the linear block index (the idiom above); each job's workgroups run conv_weights_body on a
// WeightArgs of their own.  680 bytes of WeightArgs per job would not fit the kernel arguments, and most of it is the tap-source tables,
// which depend on the KIND of geometry only: the arguments carry a small record per job and the few distinct tables (r and s, both
// 0..3, in one byte), and a workgroup puts its job's WeightArgs together in LDS.
constexpr int kBatchJobs = 16, kBatchTables = 6;
constexpr int kBatchBlocks = 16384;                 // workgroups of one launch (one job: at most grid_for's 2048)

struct BatchJob {
    const float* w; const float* amax; float* scale_out; char* img;
    int64_t sk, sn, sr, ss, n4;
    int K, Nn;
    float coef, bound_mul;
    int amax_count, table;
};
struct BatchTable {
    int ntaps, nphase;
    signed char nsrc[kMaxPhase][kMaxTaps];
    unsigned char rs[kMaxPhase][kMaxTaps][4];       // r | s << 2
};
struct WeightBatch {
    BatchJob job[kBatchJobs];
    BatchTable table[kBatchTables];
    int first[kBatchJobs + 1];
    int count;
};
static_assert(sizeof(WeightBatch) <= 4096, "the batch travels in the kernel arguments");

__global__ __launch_bounds__(256) void conv_weights_batch_kernel(WeightBatch q)
{
    __shared__ WeightArgs a;
    int i = 0;
    while (i + 1 < q.count && (int)blockIdx.x >= q.first[i + 1]) ++i;
    const BatchJob& j = q.job[i];
    const BatchTable& t = q.table[j.table];
    if (threadIdx.x == 0) {
        a.w = j.w; a.sk = j.sk; a.sn = j.sn; a.sr = j.sr; a.ss = j.ss;
        a.amax = j.amax; a.scale_out = j.scale_out; a.img = j.img;
        a.K = j.K; a.Nn = j.Nn; a.ntaps = t.ntaps; a.nphase = t.nphase;
        a.n4 = j.n4; a.coef = j.coef; a.bound_mul = j.bound_mul; a.amax_count = j.amax_count;
    }
    for (int e = threadIdx.x; e < kMaxPhase * kMaxTaps * 4; e += 256) {
        const int p = e / (kMaxTaps * 4), tp = (e >> 2) % kMaxTaps, m = e & 3;
        const unsigned char v = t.rs[p][tp][m];
        a.r[p][tp][m] = (signed char)(v & 3);
        a.s[p][tp][m] = (signed char)(v >> 2);
        if (m == 0) a.nsrc[p][tp] = t.nsrc[p][tp];
    }
    __syncthreads();
    conv_weights_body(a, (int)blockIdx.x - q.first[i], q.first[i + 1] - q.first[i]);
}

// max|x| of many tensors in one grid: kAmaxBlocks workgroups per tensor, conv_absmax_kernel's mapping of elements to workgroups (the
// same partials, so the same scale_of)
constexpr int kAbsmaxJobs = 32;
struct AbsmaxJob { const float* x; int64_t n; float* partial; };
struct AbsmaxBatch { AbsmaxJob job[kAbsmaxJobs]; };

__global__ __launch_bounds__(256) void conv_absmax_batch_kernel(AbsmaxBatch q)
{
    __shared__ float red[4];
    const AbsmaxJob& j = q.job[blockIdx.x / kAmaxBlocks];
    const int bid = blockIdx.x % kAmaxBlocks;
    const float* __restrict__ x = j.x;
    const int64_t n4 = j.n >> 2;
    float m = 0.f;
    for (int64_t i = bid * 256 + threadIdx.x; i < n4; i += (int64_t)kAmaxBlocks * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        m = fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    if (bid == 0 && threadIdx.x == 0) for (int64_t i = 4 * n4; i < j.n; ++i) m = fmaxf(m, fabsf(x[i]));
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) j.partial[bid] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- weight gradient: dW[slice][ci][co] = sum over grid points of x[in pixel][ci] * gy[out pixel][co] -------------------
// The reduction runs over PIXELS, which are the slow axis of both NHWC operands: the tiles are staged pixel-major
// (LDS-DMA: one 1-KiB chunk = 16 pixels x 32 channels, 64 B per pixel from 4 lanes) and the MFMA fragments -- 8
// consecutive pixels of one channel per lane -- come out of two ds_read_b64_tr_b16 each (gfx950's transposing read: a
// 16-lane group reads 4 pixels x 16 channels and gets them channel-major; the 4 x 64 B of a 32-lane half cover all 64
// banks once).  A workgroup owns one (slice, 64 MB input channels, 64 NB output channels) tile and a range of 32-point
// chunks of the grid; the per-range partial sums go to a workspace and conv_wrw_reduce_kernel adds them in a fixed order
// (deterministic) and writes dW in the weight's own layout.
struct WrwOperand {                                 // one side of the product: split planes [N][Hp][Wp][C], pixel = grid * stride + offset
    const _Float16* hi; const _Float16* lo;
    int Hp, Wp, C, stride;
    signed char dy[kMaxPhase][kMaxTaps], dx[kMaxPhase][kMaxTaps];
};

struct WrwArgs {
    WrwOperand A, B;                                // rows / columns of the result tile
    const _Float16* zero;
    float* partial;                                 // [splits][slices][A.C][B.C]
    int N, H, W, ntaps, nphase;
    unsigned magHW, shHW, magW, shW;                // m / (H*W) and rem / W by multiply-shift (m < 2^31)
    int nchunks, cps;                               // 32-point chunks in the grid, chunks per split
};

typedef short s16x4v __attribute__((__vector_size__(4 * sizeof(short))));

__device__ __forceinline__ f16x8 tr_read8(const char* block, int lane_off)
{
    // rows q..q+3 and q+4..q+7 of this lane's channel: two transposing reads 256 B (4 pixels) apart
    auto p = (__attribute__((address_space(3))) s16x4v*)((__attribute__((address_space(3))) char*)(block + lane_off));
    auto q = (__attribute__((address_space(3))) s16x4v*)((__attribute__((address_space(3))) char*)(block + lane_off + 256));
    const s16x4v a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p);
    const s16x4v b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(q);
    typedef short s16x8v __attribute__((__vector_size__(8 * sizeof(short))));
    const s16x8v ab = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(f16x8, ab);
}

template <int MB, int NB>
__device__ __forceinline__ void conv_wrw_body(const WrwArgs& a, const unsigned bx, const unsigned by)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TA = 64 * MB, TB = 64 * NB;
    constexpr int A_BYTES = 2 * MB * 4 * 1024, B_BYTES = 2 * NB * 4 * 1024, STAGE = A_BYTES + B_BYTES;
    constexpr int AQ = (2 * MB) / 4, BQ = (2 * NB) / 4;
    // <1, 1> (a 64 x 64 tile, for layers with a 64-channel side): two 32-channel blocks per operand and four waves, so a wave stages ONE
    // block of ONE operand (waves 0, 1: the rows' blocks, waves 2, 3: the columns') instead of AQ blocks of each
    constexpr bool ONE = MB == 1 && NB == 1;
    static_assert(ONE || (MB >= 2 && NB >= 2), "a wave stages whole blocks of both operands, or one block of one");

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nta = a.A.C / TA, ntb = a.B.C / TB;
    int idx = by;
    const int tb = idx % ntb; idx /= ntb;
    const int ta = idx % nta; idx /= nta;
    const int tap = idx % a.ntaps, phase = idx / a.ntaps;
    const int c0 = bx * a.cps, c1 = min(c0 + a.cps, a.nchunks);
    const int dya = a.A.dy[phase][tap], dxa = a.A.dx[phase][tap], dyb = a.B.dy[phase][tap], dxb = a.B.dx[phase][tap];
    const unsigned HW = a.H * a.W;
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
    const int c8 = (lane & 3) * 8;                  // this lane's 8 channels inside a 32-channel block

    auto issue = [&](int c, int stage) {
        const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
        #pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned m = c * 32 + s * 16 + (lane >> 2);
            const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            const int ay = yy * a.A.stride + dya, ax = xx * a.A.stride + dxa;
            const int by = yy * a.B.stride + dyb, bx = xx * a.B.stride + dxb;
            const bool oka = (unsigned)ay < (unsigned)a.A.Hp && (unsigned)ax < (unsigned)a.A.Wp;
            const bool okb = (unsigned)by < (unsigned)a.B.Hp && (unsigned)bx < (unsigned)a.B.Wp;
            const int64_t ea = ((int64_t)((n * a.A.Hp + ay) * a.A.Wp + ax)) * a.A.C + ta * TA + c8;
            const int64_t eb = ((int64_t)((n * a.B.Hp + by) * a.B.Wp + bx)) * a.B.C + tb * TB + c8;
            #pragma unroll
            for (int q = 0; q < AQ; ++q) {
                const int b = wave * AQ + q;
                const _Float16* ph = oka ? a.A.hi + ea + b * 32 : a.zero + c8;
                const _Float16* pl = oka ? a.A.lo + ea + b * 32 : a.zero + c8;
                const unsigned l = sbase + ((b * 2 + s) * 2) * 1024;
                lds_dma16(ph, l);
                lds_dma16(pl, l + 1024);
            }
            #pragma unroll
            for (int q = 0; q < BQ; ++q) {
                const int b = wave * BQ + q;
                const _Float16* ph = okb ? a.B.hi + eb + b * 32 : a.zero + c8;
                const _Float16* pl = okb ? a.B.lo + eb + b * 32 : a.zero + c8;
                const unsigned l = sbase + A_BYTES + ((b * 2 + s) * 2) * 1024;
                lds_dma16(ph, l);
                lds_dma16(pl, l + 1024);
            }
        }
    };

    f32x16 acc[MB][NB];
    #pragma unroll
    for (int i = 0; i < MB; ++i)
        #pragma unroll
        for (int j = 0; j < NB; ++j)
            #pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposing-read address of this lane inside a 1-KiB (16 pixels x 64 B) block
    const int tr_off = ((lane >> 5) * 8 + ((lane & 15) >> 2)) * 64 + (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;

    // the hand-placed iteration of conv_f16x3_kernel: fragments of k-step 0 behind the barrier, the next chunk's
    // addresses and DMAs and the transposing reads of k-step 1 in the shadow of the MFMAs
    constexpr int NA = ONE ? 4 : AQ * 4, ND = ONE ? 4 : NA + BQ * 4, HALF = ND / 2, PER = 3 * MB * NB, GAP = ONE ? 1 : PER / HALF;
    static_assert(ONE || PER % HALF == 0, "DMAs spread evenly");
    const char* pA[2][2]; const char* pB[2][2];     // [k-step][hi | lo] sources of this lane's first block
    int stA[2], stB[2];                             // bytes to the next 32-channel block (0 on the zero line)
    unsigned sb_next = 0;
    auto prep = [&](int c, int stage) {
        #pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned m = c * 32 + s * 16 + (lane >> 2);
            const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            if constexpr (ONE) {                    // this wave's operand (wave-uniform) and block: pA carries its sources
                const bool isb = wave >= 2;
                const int py = isb ? yy * a.B.stride + dyb : yy * a.A.stride + dya, px = isb ? xx * a.B.stride + dxb : xx * a.A.stride + dxa;
                const int Hp = isb ? a.B.Hp : a.A.Hp, Wp = isb ? a.B.Wp : a.A.Wp, Cc = isb ? a.B.C : a.A.C;
                const bool okp = (unsigned)py < (unsigned)Hp && (unsigned)px < (unsigned)Wp;
                const int64_t ep = ((int64_t)((n * Hp + py) * Wp + px)) * Cc + (isb ? tb * TB : ta * TA) + (wave & 1) * 32 + c8;
                pA[s][0] = reinterpret_cast<const char*>(okp ? (isb ? a.B.hi : a.A.hi) + ep : a.zero + c8);
                pA[s][1] = reinterpret_cast<const char*>(okp ? (isb ? a.B.lo : a.A.lo) + ep : a.zero + c8);
                continue;
            }
            const int ay = yy * a.A.stride + dya, ax = xx * a.A.stride + dxa;
            const int by = yy * a.B.stride + dyb, bx = xx * a.B.stride + dxb;
            const bool oka = (unsigned)ay < (unsigned)a.A.Hp && (unsigned)ax < (unsigned)a.A.Wp;
            const bool okb = (unsigned)by < (unsigned)a.B.Hp && (unsigned)bx < (unsigned)a.B.Wp;
            const int64_t ea = ((int64_t)((n * a.A.Hp + ay) * a.A.Wp + ax)) * a.A.C + ta * TA + wave * (AQ * 32) + c8;
            const int64_t eb = ((int64_t)((n * a.B.Hp + by) * a.B.Wp + bx)) * a.B.C + tb * TB + wave * (BQ * 32) + c8;
            pA[s][0] = reinterpret_cast<const char*>(oka ? a.A.hi + ea : a.zero + c8);
            pA[s][1] = reinterpret_cast<const char*>(oka ? a.A.lo + ea : a.zero + c8);
            pB[s][0] = reinterpret_cast<const char*>(okb ? a.B.hi + eb : a.zero + c8);
            pB[s][1] = reinterpret_cast<const char*>(okb ? a.B.lo + eb : a.zero + c8);
            stA[s] = oka ? 64 : 0; stB[s] = okb ? 64 : 0;
        }
        sb_next = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
    };
    auto dma = [&](int d) {
        if constexpr (ONE) {                        // d = (k-step, hi | lo) of the wave's block; A's blocks first, then B's (A_BYTES = 8 KiB)
            lds_dma16(pA[d >> 1][d & 1], sb_next + (((wave * 2) + (d >> 1)) * 2 + (d & 1)) * 1024);
        } else if (d < NA) {
            const int s = d / (AQ * 2), q = (d >> 1) % AQ, pl = d & 1;
            lds_dma16(pA[s][pl] + q * stA[s], sb_next + (((wave * AQ + q) * 2 + s) * 2 + pl) * 1024);
        } else {
            const int e = d - NA;
            const int s = e / (BQ * 2), q = (e >> 1) % BQ, pl = e & 1;
            lds_dma16(pB[s][pl] + q * stB[s], sb_next + A_BYTES + (((wave * BQ + q) * 2 + s) * 2 + pl) * 1024);
        }
    };
    f16x8 fa[2][MB][2], fb[2][NB][2];               // [k-step][block][hi | lo]
    auto frags = [&](int stage, int ks) {
        const char* sa = smem + stage * STAGE;
        const char* sb = sa + A_BYTES;
        #pragma unroll
        for (int i = 0; i < MB; ++i) {
            const char* p = sa + (((wm * MB + i) * 2 + ks) * 2) * 1024;
            fa[ks][i][0] = tr_read8(p, tr_off);
            fa[ks][i][1] = tr_read8(p + 1024, tr_off);
        }
        #pragma unroll
        for (int j = 0; j < NB; ++j) {
            const char* p = sb + (((wn * NB + j) * 2 + ks) * 2) * 1024;
            fb[ks][j][0] = tr_read8(p, tr_off);
            fb[ks][j][1] = tr_read8(p + 1024, tr_off);
        }
    };
    if (c0 < c1) {
        prep(c0, 0);
        #pragma unroll
        for (int d = 0; d < ND; ++d) dma(d);
    }
    for (int c = c0; c < c1; ++c) {
        const int stage = (c - c0) & 1;
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        frags(stage, 0);
        prep(c + 1 < c1 ? c + 1 : c, stage ^ 1);    // the last chunk re-fetches itself into the idle stage: no branch
        __builtin_amdgcn_sched_barrier(0);
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            #pragma unroll
            for (int g = 0; g < PER; ++g) {
                const int prod = g / (MB * NB), i = (g / NB) % MB, j = g % NB;
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][i][prod == 0 ? 1 : 0], fb[ks][j][prod == 1 ? 1 : 0], acc[i][j], 0, 0, 0);
                if ((g + 1) % GAP == 0 && g / GAP < HALF) {     // (<1, 1>: two DMAs behind the first two of three MFMAs)
                    dma(ks * HALF + g / GAP);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (ks == 0 && g == PER / 2) {
                    frags(stage, 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);

    const int slice = phase * a.ntaps + tap, nslice = a.nphase * a.ntaps;
    float* out = a.partial + ((int64_t)bx * nslice + slice) * a.A.C * a.B.C;
    #pragma unroll
    for (int i = 0; i < MB; ++i)
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ci = ta * TA + (wm * MB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            float* o = out + (int64_t)ci * a.B.C + tb * TB + wn * NB * 32 + (lane & 31);
            #pragma unroll
            for (int j = 0; j < NB; ++j) o[j * 32] = acc[i][j][r];
        }
}

template <int MB, int NB>
__global__ __launch_bounds__(256) void conv_wrw_kernel(WrwArgs a) { conv_wrw_body<MB, NB>(a, blockIdx.x, blockIdx.y); }

// ---- 32 x 32 tiles: a side that is 32 beyond a multiple of 64 (wc_conv_slim_supported) --------------------------------------------------
// One 32 x 32 result tile is one MFMA block: a single wave's work.  So the four waves of a workgroup do not share a tile's blocks, they
// share its PIXELS: wave w of workgroup x is pixel range 4 x + w of the launch (`ranges` of them: wrw_prepare's split count), with two
// LDS stages of its own (2 x 8 KiB a wave: the rows' and the columns' 16 pixels x 32 channels, k-step and hi | lo) that no other wave
// reads or writes -- no workgroup barrier anywhere; a wave waits for its own LDS-DMAs (vmcnt) and the in-order issue of its transposing
// reads and MFMAs keeps a stage's readers ahead of the DMAs that refill it.  The staging (pixel-major chunks), the ds_read_b64_tr_b16
// fragments, the partial sums' layout [range][slice][rows][columns] and therefore conv_wrw_reduce_kernel are conv_wrw_body's; which
// operand the 32-wide side is (rows or columns: x_cols in wrw_prepare) makes no difference here, both sides are cut into 32s.
__global__ __launch_bounds__(256) void conv_wrw_slim_kernel(WrwArgs a, int ranges)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int STAGE = 8 * 1024;                 // A: [k-step][hi | lo] 1 KiB each, then B's four
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rng = blockIdx.x * 4 + wave;
    if (rng >= ranges) return;                      // (wave-uniform; the waves never meet at a barrier)
    const int nta = a.A.C >> 5, ntb = a.B.C >> 5;
    int idx = blockIdx.y;
    const int tb = idx % ntb; idx /= ntb;
    const int ta = idx % nta; idx /= nta;
    const int tap = idx % a.ntaps, phase = idx / a.ntaps;
    const int c0 = rng * a.cps, c1 = min(c0 + a.cps, a.nchunks);
    const int dya = a.A.dy[phase][tap], dxa = a.A.dx[phase][tap], dyb = a.B.dy[phase][tap], dxb = a.B.dx[phase][tap];
    const unsigned HW = a.H * a.W;
    char* mine = smem + wave * (2 * STAGE);
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)mine);
    const int c8 = (lane & 3) * 8;                  // this lane's 8 channels inside a 32-channel block

    // the eight 1-KiB chunks of pixel chunk c -> stage
    auto issue = [&](int c, int stage) {
        const unsigned sbase = __builtin_amdgcn_readfirstlane(lds0 + stage * STAGE);
        #pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned m = c * 32 + s * 16 + (lane >> 2);
            const unsigned n = __umulhi(m, a.magHW) >> a.shHW, rem = m - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            const int ay = yy * a.A.stride + dya, ax = xx * a.A.stride + dxa;
            const int by = yy * a.B.stride + dyb, bx = xx * a.B.stride + dxb;
            const bool oka = (unsigned)ay < (unsigned)a.A.Hp && (unsigned)ax < (unsigned)a.A.Wp;
            const bool okb = (unsigned)by < (unsigned)a.B.Hp && (unsigned)bx < (unsigned)a.B.Wp;
            const int64_t ea = ((int64_t)((n * a.A.Hp + ay) * a.A.Wp + ax)) * a.A.C + ta * 32 + c8;
            const int64_t eb = ((int64_t)((n * a.B.Hp + by) * a.B.Wp + bx)) * a.B.C + tb * 32 + c8;
            lds_dma16(oka ? a.A.hi + ea : a.zero + c8, sbase + (s * 2) * 1024);
            lds_dma16(oka ? a.A.lo + ea : a.zero + c8, sbase + (s * 2 + 1) * 1024);
            lds_dma16(okb ? a.B.hi + eb : a.zero + c8, sbase + 4096 + (s * 2) * 1024);
            lds_dma16(okb ? a.B.lo + eb : a.zero + c8, sbase + 4096 + (s * 2 + 1) * 1024);
        }
    };

    f32x16 acc;
    #pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // transposing-read address of this lane inside a 1-KiB (16 pixels x 64 B) block
    const int tr_off = ((lane >> 5) * 8 + ((lane & 15) >> 2)) * 64 + (((lane >> 4) & 1) * 16 + (lane & 3) * 4) * 2;

    if (c0 < c1) issue(c0, 0);
    for (int c = c0; c < c1; ++c) {
        const int stage = (c - c0) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the stage's chunks have landed (this wave's own; nobody else's are read)
        const char* sa = mine + stage * STAGE;
        f16x8 fa[2][2], fb[2][2];                   // [k-step][hi | lo]
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            fa[ks][0] = tr_read8(sa + (ks * 2) * 1024, tr_off);
            fa[ks][1] = tr_read8(sa + (ks * 2 + 1) * 1024, tr_off);
            fb[ks][0] = tr_read8(sa + 4096 + (ks * 2) * 1024, tr_off);
            fb[ks][1] = tr_read8(sa + 4096 + (ks * 2 + 1) * 1024, tr_off);
        }
        // the other stage's readers are the chunk before's: an LDS queue answers in order, so with these fragments in, theirs are
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (c + 1 < c1) issue(c + 1, stage ^ 1);
        #pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            #pragma unroll
            for (int prod = 0; prod < 3; ++prod)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[ks][prod == 0 ? 1 : 0], fb[ks][prod == 1 ? 1 : 0], acc, 0, 0, 0);
    }

    const int slice = phase * a.ntaps + tap, nslice = a.nphase * a.ntaps;
    float* out = a.partial + ((int64_t)rng * nslice + slice) * a.A.C * a.B.C;
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ci = ta * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        out[(int64_t)ci * a.B.C + tb * 32 + (lane & 31)] = acc[r];
    }
}

struct WrwReduceArgs {
    const float* partial; int splits, nslice, Ca, Cb;    // partial [splits][slices][Ca][Cb]
    const float* xscale; const float* gscale;
    float* dw; int64_t sa, sb, sr, ss;                   // element (a, b, r, s) -> dw[a*sa + b*sb + r*sr + s*ss]
    float coef;
    const float* colsum; float* db; int c4n, main_blocks;   // optional bias gradient: kAmaxBlocks partial rows [C] -> db[C]
    int nout;                                            // source taps of the weight; each collects the slices built from it
    signed char r[kMaxTaps], s[kMaxTaps], cnt[kMaxTaps], slice[kMaxTaps][4];
};

__device__ __forceinline__ void conv_wrw_reduce_body(const WrwReduceArgs& a, const unsigned bid)
{
    // four lanes per output float4: each takes every fourth range, a fixed two-step butterfly joins them (the order of the
    // additions is the same in every run) -- four times the loads in flight of one thread walking all the ranges
    if ((int)bid >= a.main_blocks) {
        // bias gradient: one wave per 4 channels, a lane adds every 64th partial row, fixed butterfly
        const int u = ((int)bid - a.main_blocks) * 256 + threadIdx.x, cg = u >> 6, lane = u & 63;
        if (cg >= a.c4n) return;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int b = lane; b < kAmaxBlocks; b += 64) v += *reinterpret_cast<const f32x4*>(a.colsum + (int64_t)b * 4 * a.c4n + 4 * cg);
        #pragma unroll
        for (int j = 0; j < 4; ++j)
            #pragma unroll
            for (int o = 1; o < 64; o <<= 1) v[j] += __shfl_xor(v[j], o);
        if (lane == 0) *reinterpret_cast<f32x4*>(a.db + 4 * cg) = v;
        return;
    }
    const int64_t plane = (int64_t)a.Ca * a.Cb, per = (int64_t)a.nslice * plane, total4 = (int64_t)a.nout * plane >> 2;
    const float inv = a.coef / (a.xscale[0] * a.gscale[0]);
    const int part = threadIdx.x & 3;
    for (int64_t e4 = ((int64_t)bid * 256 + threadIdx.x) >> 2; e4 < total4; e4 += (int64_t)a.main_blocks * 64) {
        const int64_t e = e4 * 4;
        const int o = e / plane; const int64_t w = e - o * plane;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < a.cnt[o]; ++i) {
            const float* src = a.partial + a.slice[o][i] * plane + w;
            int sp = part;
            for (; sp + 28 < a.splits; sp += 32) {      // eight ranges in flight (the additions keep their order: the same bits)
                f32x4 t[8];
                #pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(sp + 4 * u) * per);
                #pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
            for (; sp < a.splits; sp += 4) v += *reinterpret_cast<const f32x4*>(src + sp * per);
        }
        #pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += __shfl_xor(v[j], 1); v[j] += __shfl_xor(v[j], 2); }
        if (part != 0) continue;
        v = v * inv;
        const int cb = w % a.Cb, ca = w / a.Cb;
        float* out = a.dw + ca * a.sa + cb * a.sb + a.r[o] * a.sr + a.s[o] * a.ss;
        if (a.sb == 1 && ((uintptr_t)out & 15) == 0) *reinterpret_cast<f32x4*>(out) = v;
        else { out[0] = v[0]; out[a.sb] = v[1]; out[2 * a.sb] = v[2]; out[3 * a.sb] = v[3]; }
    }
}

__global__ __launch_bounds__(256) void conv_wrw_reduce_kernel(WrwReduceArgs a) { conv_wrw_reduce_body(a, blockIdx.x); }

// ---- one layer's backward in two launches: data gradient and weight gradient side by side -----------------------------------------------
// The critic's 128-channel layers at 8x8 and 16x16 give each gradient about one workgroup per CU (one wave per SIMD), and the two need
// nothing from each other: both read only the output gradient's planes and saved tensors.  As four launches the second pair waits behind
// the first; here ONE grid holds the workgroups of both (conv_weights_pair_kernel's idiom: the role is a range of the linear block index,
// wave-uniform) and one launch finishes both.  Two <2, 2> workgroups (<= 84 + 64 registers, 64 KiB of LDS each) share a CU.  No
// cross-workgroup waits, atomics or counters: every workgroup runs the body it runs in conv_f16x3_kernel<2, 2, KS> / conv_wrw_kernel<2, 2>
// on the same operands and the reductions keep their order, so dx, dW and db have the bits of the four launches.
//   blocks [0, conv_blocks):  the data gradient's 3-d grid (gx, gy, ksplit), x fastest.  Its workgroups are the longer ones (9-36
//                             iterations against the weight gradient's 4-20 chunks) and go first: measured against the other order at
//                             batch 128, 37.3 / 77.7 / 50.5 / 19.2 us against 38.4 / 83.3 / 53.0 / 19.2 (profiles/conv_pair_shapes.txt)
//   blocks [wrw_off, ...):    the weight gradient's (split, tile) as dim3(splits, tiles) linearises; wrw_off = conv_blocks rounded up to a
//                             multiple of 8 (the blocks between return at once), so a pixel range keeps its residue mod 8, i.e. the
//                             workgroups that read one range still share an XCD as wrw_splits means them to.
template <bool KS, bool RG>
__device__ __forceinline__ void conv_bwd_pair_body(const ConvArgs& d, const WrwArgs& w, int conv_blocks, int wrw_off, int wrw_splits, int gx, int gy)
{
    const int b = blockIdx.x;
    if (b < conv_blocks) {
        const int t = b / gx, z = t / gy;
        conv_f16x3_body<2, 2, KS, RG>(d, (unsigned)(b - t * gx), (unsigned)(t - z * gy), (unsigned)z);
    } else if (b >= wrw_off) {
        const int e = b - wrw_off, tile = e / wrw_splits;
        conv_wrw_body<2, 2>(w, (unsigned)(e - tile * wrw_splits), (unsigned)tile);
    }
}

template <bool KS>
__global__ __launch_bounds__(256) void conv_bwd_pair_kernel(ConvArgs d, WrwArgs w, int conv_blocks, int wrw_off, int wrw_splits, int gx, int gy)
{
    conv_bwd_pair_body<KS, false>(d, w, conv_blocks, wrw_off, wrw_splits, gx, gy);
}

// the data gradient's grid with a partial last tile (conv_f16x3_ragged_kernel's body); the weight gradient's part is the same
template <bool KS>
__global__ __launch_bounds__(256) void conv_bwd_pair_ragged_kernel(ConvArgs d, WrwArgs w, int conv_blocks, int wrw_off, int wrw_splits, int gx, int gy)
{
    conv_bwd_pair_body<KS, true>(d, w, conv_blocks, wrw_off, wrw_splits, gx, gy);
}

// blocks [0, wrw_blocks): conv_wrw_reduce_kernel's (main and bias-gradient blocks); the rest: conv_ksplit_reduce_kernel's
__global__ __launch_bounds__(256) void conv_pair_reduce_kernel(WrwReduceArgs r, KsplitReduceArgs k, int wrw_blocks)
{
    if ((int)blockIdx.x < wrw_blocks) conv_wrw_reduce_body(r, blockIdx.x);
    else conv_ksplit_reduce_body(k.partial, k.ksplit, k.n4, k.cout, k.xscale, k.wscale, k.bias, k.relu, k.y,
                                 blockIdx.x - wrw_blocks, gridDim.x - wrw_blocks);
}

// the same launch with the data gradient's finish going on to its follower's work (conv_finish_tail_body): kAmaxBlocks workgroups behind
// the weight reduction's for MASKED, conv_pair_reduce_kernel's count for DX.  A kernel of its own: the one above keeps its code.
template <int KIND>
__global__ __launch_bounds__(256) void conv_pair_reduce_tail_kernel(WrwReduceArgs r, FinishTailArgs a, int wrw_blocks)
{
    if ((int)blockIdx.x < wrw_blocks) conv_wrw_reduce_body(r, blockIdx.x);
    else conv_finish_tail_body<KIND>(a, blockIdx.x - wrw_blocks, gridDim.x - wrw_blocks);
}

// ---- weight and bias gradient of a convolution with a handful of INPUT channels (round 5) ---------------------------------------------
// The critic's first block reads images: Conv2D 3 -> 128 (3x3) and the 1x1 shortcut 3 -> 128 (discriminator.py:41-54 with input_image_shape
// (32, 32, 3)).  Their forward stays with MIOpen (15 us); their weight gradients were MIOpen's too, at 138 and 54 us per critic update for
// 0.9 GFLOP -- 67 MB of gy read at 0.5 TB/s.  Here it is ONE pass over gy at the stream rate on the fp32 matrix pipe:
//     D[m][o] = sum_p A[p][m] gy[p][o],   m = tap * Cin + c (< 32):  A[p][m] = x[p + tap][c] (zero padding),  row ntaps * Cin: A = 1  (-> db)
// as v_mfma_f32_32x32x2_f32 over pixel pairs: lane (i, k) gathers A[p + k][i] (4 bytes out of L1: x is 1.5 MB) and loads 16 bytes of
// gy[p + k][4 i ..] -- the four floats feed four MFMAs, i.e. output block q holds the channels 4 j + q.  A workgroup of 8 waves takes a pixel
// range, folds its waves' accumulators in LDS (fixed order) and leaves one partial; conv_wrw_narrow_reduce_kernel adds the partials in a
// fixed order and scatters into the weight's layout.  fp32 throughout (as MIOpen's kernel): no split, no scales.
struct NarrowWrwArgs {
    const float* x; const float* gy; float* partial;
    int N, H, W, Cin, Cout, ks, nrow;                // ks = 1 | 3 ('same' padding); nrow = ks * ks * Cin (< 32)
    unsigned magHW, shHW, magW, shW;
    int64_t M; int64_t pix_per_wave;                 // (even)
};

// MASKED (the critic's first block, conv._CriticFirstBlock): gy is conv2's data gradient as it comes and `mask` conv1's output h -- the
// ReLU between the two is applied to the 16 bytes a lane has just loaded (wc_relu_mask_apply: threshold_backward's predicate), so the
// masked copy of the block's largest tensor is never written or read.  A masked-out product is (+-0) * x onto an accumulator that
// started as +0: the sums keep the bits they have behind threshold_backward's +0 for every finite gy.  The plain kernel keeps its code.
template <bool MASKED>
__device__ __forceinline__ void conv_wrw_narrow_body(const NarrowWrwArgs& a, const float* __restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) float nw_part[];     // [8 waves][4 q][16 r][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, k = lane >> 5;
    const int grp = blockIdx.y;                                         // 128 output channels
    const bool is_tap = i < a.nrow, is_one = i == a.nrow;
    int dy = 0, dx = 0, c = 0;
    if (is_tap) {
        const int tap = i / a.Cin;
        c = i - tap * a.Cin;
        dy = tap / a.ks - a.ks / 2; dx = tap % a.ks - a.ks / 2;
    }
    const unsigned HW = (unsigned)(a.H * a.W);
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int64_t p0 = ((int64_t)blockIdx.x * 8 + wave) * a.pix_per_wave;
    int64_t p1 = p0 + a.pix_per_wave;
    if (p1 > a.M) p1 = a.M;
    // (Cout % 128 == 64: the last group's upper half has no channels -- those lanes read the group's first ones, nobody reads their results)
    const int gyo = grp * 128 + (grp * 128 + 4 * i < a.Cout ? 4 * i : 0);
    const float* gyc = a.gy + gyo;
    const float* mkc = MASKED ? mask + gyo : nullptr;                   // (the mask at the offset of gy's 16 bytes: clamped and half-group lanes too)
    constexpr int U = 8;
    for (int64_t p = p0; p < p1; p += 2 * U) {
        float av[U]; f32x4 bv[U];
        [[maybe_unused]] f32x4 mv[MASKED ? U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pp = p + 2 * u + k;
            const bool ok = pp < p1;
            const unsigned pc = (unsigned)(ok ? pp : a.M - 1);          // clamped, not predicated: the loads stay in flight together
            const unsigned n = __umulhi(pc, a.magHW) >> a.shHW, rem = pc - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            const int iy = (int)yy + dy, ix = (int)xx + dx;
            const bool inb = ok && is_tap && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const float xv = a.x[inb ? ((int64_t)(n * a.H + iy) * a.W + ix) * a.Cin + c : 0];
            av[u] = inb ? xv : ((ok && is_one) ? 1.f : 0.f);
            bv[u] = *reinterpret_cast<const f32x4*>(gyc + (int64_t)pc * a.Cout);
            if (MASKED) mv[u] = *reinterpret_cast<const f32x4*>(mkc + (int64_t)pc * a.Cout);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (MASKED) bv[u] = wc_relu_mask_apply(bv[u], mv[u]);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][q], acc[q], 0, 0, 0);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) nw_part[((wave * 4 + q) * 16 + r) * 64 + lane] = acc[q][r];
    __syncthreads();
    float* out = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int e = tid + 512 * m;
        float sum = nw_part[e];
#pragma unroll
        for (int w = 1; w < 8; ++w) sum += nw_part[w * 4096 + e];
        out[e] = sum;
    }
}

__global__ __launch_bounds__(512, 1) void conv_wrw_narrow_kernel(NarrowWrwArgs a) { conv_wrw_narrow_body<false>(a, nullptr); }

__global__ __launch_bounds__(512, 1) void conv_wrw_narrow_masked_kernel(NarrowWrwArgs a, const float* __restrict__ mask)
{
    conv_wrw_narrow_body<true>(a, mask);
}

// element e = (q, r, lane) of a partial -> row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), output channel 128 grp + 4 (lane & 31) + q.
// A workgroup = 32 elements x 8 groups of partials (every 8th partial each, 16 loads in flight), folded through LDS in a fixed order.
__global__ __launch_bounds__(256) void conv_wrw_narrow_reduce_kernel(const float* __restrict__ partial, int nparts, int Cin, int ks, int nrow,
                                                                     float* __restrict__ dw, int64_t sk, int64_t sn, int64_t sr, int64_t ss,
                                                                     float* __restrict__ db, int Cout)
{
    __shared__ float red[8][32];
    const int el = threadIdx.x & 31, pg = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + el;                                 // < 4096
    const float* p = partial + (int64_t)blockIdx.y * nparts * 4096 + e;
    float sum = 0.f;
    int z = pg;
    for (; z + 8 * 15 < nparts; z += 8 * 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = p[(int64_t)(z + 8 * u) * 4096];
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += v[u];
    }
    for (; z < nparts; z += 8) sum += p[(int64_t)z * 4096];
    red[pg][el] = sum;
    __syncthreads();
    if (pg != 0) return;
#pragma unroll
    for (int g = 1; g < 8; ++g) sum += red[g][el];
    const int q = e >> 10, r = (e >> 6) & 15, ln = e & 63;
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
    const int o = blockIdx.y * 128 + 4 * (ln & 31) + q;
    if (o >= Cout) return;
    if (row < nrow) {
        const int tap = row / Cin, c = row - tap * Cin;
        dw[c * sk + o * sn + (tap / ks) * sr + (tap % ks) * ss] = sum;
    } else if (row == nrow && db) db[o] = sum;
}

// ---- the same gradient with a channel group of 32 (wc_conv_wrw_narrow32_f32 where Cout % 64 == 32) ----------------------------------------
// The generator's last layer at 32 filters (ImageNet recipe, 32 -> 3 at 128 x 128) with the operands exchanged: "gy" is the layer's input,
// 32 channels wide.  The body above gives a lane 16 bytes of gy and four MFMAs per pixel pair; at 32 channels three of the four and 24 of
// 32 lanes' loads would be waste.  Here lane (i, k) loads the ONE float gy[p + k][32 grp + i] (a half-wave reads a pixel's whole 128-byte
// row) and a pixel pair is one v_mfma_f32_32x32x2_f32.  The same pixel ranges per wave, the same LDS fold over the eight waves in wave
// order, the same ones-row for db; a partial is 1024 floats.  Every group of such a layer is 32 wide (Cout = 96: three groups, not a
// 64-group and a remainder): one kernel, one element map.  With 16 accumulator registers the loop keeps 16 pixel pairs in flight.
__global__ __launch_bounds__(512, 1) void conv_wrw_narrow32_kernel(NarrowWrwArgs a)
{
    __shared__ float nw32_part[8 * 1024];                               // [8 waves][16 r][64 lanes]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, k = lane >> 5;
    const int grp = blockIdx.y;                                         // 32 output channels
    const bool is_tap = i < a.nrow, is_one = i == a.nrow;
    int dy = 0, dx = 0, c = 0;
    if (is_tap) {
        const int tap = i / a.Cin;
        c = i - tap * a.Cin;
        dy = tap / a.ks - a.ks / 2; dx = tap % a.ks - a.ks / 2;
    }
    const unsigned HW = (unsigned)(a.H * a.W);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int64_t p0 = ((int64_t)blockIdx.x * 8 + wave) * a.pix_per_wave;
    int64_t p1 = p0 + a.pix_per_wave;
    if (p1 > a.M) p1 = a.M;
    const float* gyc = a.gy + grp * 32 + i;
    constexpr int U = 16;
    for (int64_t p = p0; p < p1; p += 2 * U) {
        float av[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t pp = p + 2 * u + k;
            const bool ok = pp < p1;
            const unsigned pc = (unsigned)(ok ? pp : a.M - 1);          // clamped, not predicated (A is zero there): the loads stay in flight together
            const unsigned n = __umulhi(pc, a.magHW) >> a.shHW, rem = pc - n * HW;
            const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
            const int iy = (int)yy + dy, ix = (int)xx + dx;
            const bool inb = ok && is_tap && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const float xv = a.x[inb ? ((int64_t)(n * a.H + iy) * a.W + ix) * a.Cin + c : 0];
            av[u] = inb ? xv : ((ok && is_one) ? 1.f : 0.f);
            bv[u] = gyc[(int64_t)pc * a.Cout];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) nw32_part[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    float* out = a.partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 1024;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int e = tid + 512 * m;
        float sum = nw32_part[e];
#pragma unroll
        for (int w = 1; w < 8; ++w) sum += nw32_part[w * 1024 + e];
        out[e] = sum;
    }
}

// conv_wrw_narrow_reduce_kernel for partials of 1024: element e = (r, lane) -> the same row, output channel 32 grp + (lane & 31); the same
// eight groups of partials and the same fold.  Grid (32, Cout / 32).
__global__ __launch_bounds__(256) void conv_wrw_narrow32_reduce_kernel(const float* __restrict__ partial, int nparts, int Cin, int ks, int nrow,
                                                                       float* __restrict__ dw, int64_t sk, int64_t sn, int64_t sr, int64_t ss,
                                                                       float* __restrict__ db, int Cout)
{
    __shared__ float red[8][32];
    const int el = threadIdx.x & 31, pg = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + el;                                 // < 1024
    const float* p = partial + (int64_t)blockIdx.y * nparts * 1024 + e;
    float sum = 0.f;
    int z = pg;
    for (; z + 8 * 15 < nparts; z += 8 * 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = p[(int64_t)(z + 8 * u) * 1024];
#pragma unroll
        for (int u = 0; u < 16; ++u) sum += v[u];
    }
    for (; z < nparts; z += 8) sum += p[(int64_t)z * 1024];
    red[pg][el] = sum;
    __syncthreads();
    if (pg != 0) return;
#pragma unroll
    for (int g = 1; g < 8; ++g) sum += red[g][el];
    const int r = e >> 6, ln = e & 63;
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5);
    const int o = blockIdx.y * 32 + (ln & 31);
    if (o >= Cout) return;
    if (row < nrow) {
        const int tap = row / Cin, c = row - tap * Cin;
        dw[c * sk + o * sn + (tap / ks) * sr + (tap % ks) * ss] = sum;
    } else if (row == nrow && db) db[o] = sum;
}

// ---- forward of a convolution with a handful of INPUT channels (round 5): y[p][o] = sum_m A[p][m] Wm[m][o],  m = tap * Cin + c ------------
// The critic's first convolution and shortcut on images (3 -> 128) and -- with the weight read through mirrored tap strides -- the data
// gradient of the generator's last layer (gy with 3 channels -> dx with 256).  MIOpen's kernel (23 us at 128x32x32, 3 -> 128) is followed by
// two bias launches (12 + 22 us); here the bias is row k*k*Cin of the product (A = 1) and the pass is bound by the 67 MB it writes.
// v_mfma_f32_32x32x2_f32 with the 32 PIXELS of a tile as rows: lane (i, k) gathers A[p_i][2 s + k] (4 bytes out of L1) for the KS k-steps,
// the weight's KS x 4 fragments (128 output channels per wave) stay in registers across the wave's tiles.  fp32 throughout.
struct NarrowFwdArgs {
    const float* x; const float* w; const float* bias; float* y;
    int N, H, W, Cin, Cout, ks, nrow, relu;          // nrow = ks * ks * Cin (< 32)
    int64_t sk, sn, sr, ss;                          // w[c * sk + o * sn + r * sr + s * ss]
    unsigned magHW, shHW, magW, shW;
    int64_t M; int ntiles, tiles_per_wave;
    signed char tdy[32], tdx[32], tch[32], tr[32], ts[32];     // row m of A: tap offsets, input channel, the weight's tap indices (host-made: no divisions on the device)
};

constexpr int kNarrowNQ = 2;          // 32-channel output blocks per wave: 64 channels (4 blocks took 316 registers: one wave per SIMD, 35 us)
// floats per pixel row of a wave's LDS tile.  64 channels: 16-byte aligned, the two lane halves 16 banks apart.  32 channels (NQ = 1,
// wc_conv_fwd_narrow32_f32): no padding -- a half-wave's ds_write_b32 is one row of 32 consecutive floats, and the four (row, column half)
// pieces that one 16-lane group of the ds_read_b128 takes -- (0, lo) (1, hi) (2, hi) (3, lo) or (0, hi) (1, lo) (2, lo) (3, hi) -- lie
// at 0, 48, 16, 32 or 16, 32, 0, 48 of the 64 banks: no bank twice.
template <int NQ> constexpr int kNarrowLd = NQ == 2 ? 32 * 2 + 4 : 32 * NQ;
// SPLIT (the critic's first block, conv._CriticFirstBlock): the float4 a lane stores to y is the unit conv_split_elem works on, so the
// kernel also leaves the planes of act(y) for the convolution that reads y next, scaled by that reader's record -- what
// conv_split_hist_kernel would have left after reading all of y back.  The record has kAmaxBlocks pairs and this grid G <= kAmaxBlocks
// workgroups (the host refuses more): workgroup b writes the pairs b, b + G, b + 2 G, ... with its maximum and the new tag -- a maximum
// may be repeated, so the array is complete, its fold is the tensor's maximum, and a mixture of tags mid-launch is never complete: the
// protocol's argument holds as it stands (no atomics, fences or counters).  nt: y leaves as non-temporal stores.
struct NarrowSplitArgs {
    _Float16* hi; _Float16* lo; float* scale_out; float* hist;
    int act; float slope; int nt;                    // split_act's convention
};

template <int KS, bool SPLIT, int NQ = kNarrowNQ>
__device__ __forceinline__ void conv_fwd_narrow_body(const NarrowFwdArgs& a, const NarrowSplitArgs* sp)
{
    __shared__ __attribute__((aligned(16))) float nf_tile[4 * 32 * kNarrowLd<NQ>];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, k = lane >> 5;
    const int grp = blockIdx.y;
    static_assert(NQ == 1 || NQ == 2, "a wave's tile: 32 pixels x 32 or 64 channels");
    constexpr int LD = kNarrowLd<NQ>;
    constexpr int RL = 8 * NQ;                                       // lanes per pixel row of the tile (16 bytes each), 64 / RL rows per store
    // the workgroup's 32 x 64 slice of the weight (row m = tap * Cin + c, the bias row, zero rows) and the rows' tap tables go through LDS:
    // eight coalesced loads per thread with wave-uniform row indices (scalar table reads) instead of ~100 dependent gathers per wave
    __shared__ float nf_w[32][32 * NQ];
    __shared__ int nf_tab[32][2];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int m = wave + 4 * j;                                  // wave-uniform
        const int kind = m < a.nrow ? 0 : (m == a.nrow ? 1 : 2);     // 0: a tap, 1: the bias row, 2: padding of K
        const int o = grp * (32 * NQ) + lane;
        const bool col = NQ == 2 || lane < 32;                       // (a 32-channel group: the upper lanes have no column, they load and write nothing)
        float v = 0.f;
        if (col && kind == 0) v = a.w[a.tch[m] * a.sk + o * a.sn + a.tr[m] * a.sr + a.ts[m] * a.ss];
        else if (col && kind == 1) v = a.bias ? a.bias[o] : 0.f;
        if (col) nf_w[m][lane] = v;
        if (lane == 0) {
            const int dy = a.tdy[m], dx = a.tdx[m];
            nf_tab[m][0] = (dy & 0xff) | ((dx & 0xff) << 8) | (kind << 16);
            nf_tab[m][1] = (dy * a.W + dx) * a.Cin + a.tch[m];
        }
    }
    __syncthreads();
    // this lane's KS rows of A: m = 2 s + k -> (dy, dx, kind), the element offset of the tap, the weight's fragments
    int dyx[KS], off[KS]; float bw[KS][NQ];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int m = 2 * s + k;
        dyx[s] = nf_tab[m][0];
        off[s] = nf_tab[m][1];
#pragma unroll
        for (int q = 0; q < NQ; ++q) bw[s][q] = nf_w[m][q * 32 + i];
    }
    const unsigned HW = (unsigned)(a.H * a.W);
    const int t0 = (blockIdx.x * 4 + wave) * a.tiles_per_wave;
    int t1 = t0 + a.tiles_per_wave;
    if (t1 > a.ntiles) t1 = a.ntiles;
    // the tile's KS values of A for this lane: gathered one tile AHEAD of the MFMAs that use them
    auto gather = [&](int t, float (&av)[KS]) __attribute__((always_inline)) {
        const int64_t p = (int64_t)t * 32 + i;
        const unsigned pc = (unsigned)(p < a.M ? p : a.M - 1);
        const unsigned n = __umulhi(pc, a.magHW) >> a.shHW, rem = pc - n * HW;
        const unsigned yy = __umulhi(rem, a.magW) >> a.shW, xx = rem - yy * a.W;
        const int pb = (int)pc * a.Cin;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int dy = (signed char)(dyx[s] & 0xff), dx = (signed char)((dyx[s] >> 8) & 0xff), kind = dyx[s] >> 16;
            const bool inb = kind == 0 && (unsigned)((int)yy + dy) < (unsigned)a.H && (unsigned)((int)xx + dx) < (unsigned)a.W;
            const float xv = a.x[inb ? pb + off[s] : 0];
            av[s] = inb ? xv : (kind == 1 ? 1.f : 0.f);
        }
    };
    [[maybe_unused]] HistPick pk = {0, 0, 1.0f};
    [[maybe_unused]] float amax = 0.f;
    [[maybe_unused]] const unsigned bid = blockIdx.y * gridDim.x + blockIdx.x;
    if constexpr (SPLIT) pk = conv_hist_pick(sp->hist, sp->scale_out, bid);
    float av[KS], an[KS];
    if (t0 < t1) gather(t0, av);
    for (int t = t0; t < t1; ++t) {
        if (t + 1 < t1) gather(t + 1, an);
        f32x16 acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bw[s][q], acc[q], 0, 0, 0);
        // rows = pixels (r & 3) + 8 (r >> 2) + 4 k of the tile, columns = output channel q * 32 + i of the group: through LDS, so that the
        // tile leaves as 16 bytes per lane, four whole 256-byte pixel rows per store (4 bytes per lane in 128-byte pieces ran at 2.6 TB/s)
        float* tl = nf_tile + wave * (32 * LD);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * k;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                float v = acc[q][r];
                if (a.relu) v = fmaxf(v, 0.f);
                tl[row * LD + q * 32 + i] = v;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);         // lgkmcnt(0): the wave's own writes (no other wave touches its slice)
#pragma unroll
        for (int j = 0; j < 32 * RL / 64; ++j) {
            const int row = (64 / RL) * j + lane / RL;
            const int64_t pr = (int64_t)t * 32 + row;
            const f32x4 v = *reinterpret_cast<const f32x4*>(tl + row * LD + 4 * (lane & (RL - 1)));
            if constexpr (!SPLIT) {
                if (pr < a.M) *reinterpret_cast<f32x4*>(a.y + pr * a.Cout + grp * (32 * NQ) + 4 * (lane & (RL - 1))) = v;
            } else if (pr < a.M) {                  // (a row past the tensor: no stores, no part in the maximum)
                const int64_t e = pr * a.Cout + grp * (32 * NQ) + 4 * (lane & (RL - 1));
                if (sp->nt) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(a.y + e));
                else *reinterpret_cast<f32x4*>(a.y + e) = v;
                amax = conv_split_elem(split_act(v, sp->act, sp->slope), amax, pk.s, sp->hi, sp->lo, e >> 2);
            }
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) av[s] = an[s];
    }
    if constexpr (SPLIT) {
        // publish (conv_hist_publish's fold and 8-byte store): the workgroup's pairs of the OTHER array
        typedef float f32x2h __attribute__((ext_vector_type(2)));
        __shared__ float nf_red[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        if (lane == 0) nf_red[wave] = amax;
        __syncthreads();
        const f32x2h p = {fmaxf(fmaxf(nf_red[0], nf_red[1]), fmaxf(nf_red[2], nf_red[3])), __builtin_bit_cast(float, pk.tag)};
        const unsigned G = gridDim.x * gridDim.y;
        for (unsigned pair = bid + tid * G; pair < (unsigned)kAmaxBlocks; pair += 256u * G)
            *reinterpret_cast<f32x2h*>(sp->hist + (1 - pk.src) * kHistArray + 2 * pair) = p;
    }
}

template <int KS>
__global__ __launch_bounds__(256, 2) void conv_fwd_narrow_kernel(NarrowFwdArgs a) { conv_fwd_narrow_body<KS, false>(a, nullptr); }

// one 32-channel block per wave (wc_conv_fwd_narrow32_f32 where Cout % 64 == 32: the mirrored data gradient of a 32 -> 3 layer)
template <int KS>
__global__ __launch_bounds__(256, 2) void conv_fwd_narrow32_kernel(NarrowFwdArgs a) { conv_fwd_narrow_body<KS, false, 1>(a, nullptr); }

template <int KS>
__global__ __launch_bounds__(256, 2) void conv_fwd_narrow_split_kernel(NarrowFwdArgs a, NarrowSplitArgs s) { conv_fwd_narrow_body<KS, true>(a, &s); }

// ---- 'same' convolution with a handful of OUTPUT channels: the data gradient of an image layer ---------------------------------------------
//     out[n, y, x, c] = sum_{r,s} sum_o m(g)[n, y - (r - p), x - (s - p), o] w[o][c][r][s],   p = ks / 2,   c < Cn,   o < Cw
// g is the wide tensor (the critic's first block: conv2's data gradient, 64 channels at 128 x 128) and m(g) = g or, with a mask tensor h
// of g's shape, threshold_backward(g, h, 0) applied to the 16 bytes a lane has just loaded (wc_relu_mask_apply): the masked copy is never
// written.  Counted directly -- rows = pixels, K = ks^2 Cw, Cn useful columns of 32 -- the product issues ks^2 times the MFMAs it needs.
// Instead, per 32-pixel tile,
//     Z[q][m] = sum_o m(g)[q][o] w[o][c][tap],   m = tap * Cn + c < 32
// is Cw / 2 v_mfma_f32_32x32x2_f32 (rows = pixels; lane (i, k) loads the floats 8 j + 4 k .. + 3 of pixel i's row, and MFMA (j, e) reduces
// channel 8 j + 4 k + e: any order of K serves as long as both operands use it), and
//     out[q][c] = sum_tap Z[q - d(tap)][tap * Cn + c]
// gathers from an LDS band of image rows.  A workgroup owns R output rows of one image and computes the Z of its ks / 2 halo rows itself
// (those rows of g come out of the L2: the grid is laid out so that neighbouring bands run on one XCD).  The rows of a band are one
// contiguous pixel range, so the tiles run over it flat, the last one partial (clamped loads, no stores).  The weight lies in LDS as
// [Cw][32].  One pass over g (and h), no atomics, every sum in a fixed order: the same bits on every call.  fp32 throughout.
struct NarrowOutArgs {
    const float* g; const float* mask; const float* w; float* out;
    int N, H, W, Cw, Cn, ks, nrow, ld;               // nrow = ks * ks * Cn (< 32); ld = floats per pixel of the band (odd: a thread per pixel meets no bank twice)
    int R, bands;                                    // output rows per workgroup, workgroups per image
    int nwg, per_xcd;                                // workgroup b of the grid works on band (b & 7) * per_xcd + (b >> 3)
    int64_t sk, sn, sr, ss;                          // w[o * sk + c * sn + r * sr + s * ss]
    unsigned magW, shW;
    const float* bias;                               // the BIAS instantiations only: Cn floats
};

constexpr int kNarrowOutThreads = 512;
constexpr int kNarrowOutLds = 80 * 1024;             // two workgroups per CU

// BIAS (wc_conv_narrow_out_bias_f32, the forward of a layer with few outputs): a.bias[c] is added to an output behind its tap sum, one fp32
// add in the gather epilogue.  The instantiations without one keep their instructions.
template <bool MASKED, bool BIAS = false>
__global__ __launch_bounds__(kNarrowOutThreads) void conv_narrow_out_kernel(NarrowOutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float no_lds[];     // [Cw][32] weight rows | [band pixels][ld] Z
    const int b = (int)(blockIdx.x & 7) * a.per_xcd + (int)(blockIdx.x >> 3);
    if (b >= a.nwg) return;                                             // (the whole workgroup, in front of every barrier)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, k = lane >> 5;
    const int n = b / a.bands, band = b - n * a.bands;
    const int pad = a.ks >> 1;
    const int y0 = band * a.R, y1 = min(y0 + a.R, a.H);
    const int z0 = max(y0 - pad, 0), z1 = min(y1 + pad, a.H);          // the rows of Z the band's outputs read
    float* wl = no_lds;
    float* zl = no_lds + a.Cw * 32;
    for (int e = tid; e < a.Cw * 32; e += kNarrowOutThreads) {
        const int o = e >> 5, m = e & 31;
        float v = 0.f;
        if (m < a.nrow) {
            const int tap = m / a.Cn, c = m - tap * a.Cn;
            const int r = tap / a.ks, s = tap - r * a.ks;
            v = a.w[o * a.sk + c * a.sn + r * a.sr + s * a.ss];
        }
        wl[e] = v;
    }
    __syncthreads();
    const int64_t P0 = ((int64_t)n * a.H + z0) * a.W;                   // the band's first pixel
    const int npix = (z1 - z0) * a.W;
    const int ntiles = (npix + 31) >> 5, nch = a.Cw >> 5;
    const int mine = wave < ntiles ? (ntiles - wave + 7) >> 3 : 0;      // this wave's tiles: wave, wave + 8, ...
    const int steps = mine * nch;                                       // (tile, 32-channel chunk), the chunks of a tile in order
    // lane (i, k): pixel i of the tile, the floats 8 j + 4 k .. + 3 of each chunk; a pixel past the band reads the band's last one
    auto address = [&](int step) __attribute__((always_inline)) -> int64_t {
        const int t = wave + 8 * (step / nch), ch = step % nch;
        const int pl = min(t * 32 + i, npix - 1);
        return (P0 + pl) * a.Cw + ch * 32 + 4 * k;
    };
    f32x4 gv[4], gn[4];
    [[maybe_unused]] f32x4 mv[MASKED ? 4 : 1], mn[MASKED ? 4 : 1];
    auto fetch = [&](int64_t at, f32x4 (&gd)[4], f32x4 (&md)[MASKED ? 4 : 1]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gd[j] = *reinterpret_cast<const f32x4*>(a.g + at + 8 * j);
            if constexpr (MASKED) md[j] = *reinterpret_cast<const f32x4*>(a.mask + at + 8 * j);
        }
    };
    if (steps > 0) fetch(address(0), gv, mv);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int step = 0; step < steps; ++step) {
        if (step + 1 < steps) fetch(address(step + 1), gn, mn);         // one chunk ahead of the MFMAs that use it
        const int ch = step % nch;
        const float* wr = wl + (ch * 32 + 4 * k) * 32 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (MASKED) gv[j] = wc_relu_mask_apply(gv[j], mv[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[j][e], wr[(8 * j + e) * 32], acc, 0, 0, 0);
        }
        if (ch == nch - 1) {
            // rows = pixels (r & 3) + 8 (r >> 2) + 4 k of the tile, column m = i
            const int t = wave + 8 * (step / nch);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int pz = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * k;
                if (pz < npix && i < a.nrow) zl[pz * a.ld + i] = acc[r];
                acc[r] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gv[j] = gn[j];
            if constexpr (MASKED) mv[j] = mn[j];
        }
    }
    __syncthreads();
    // a thread per output pixel: the taps in their order, then the channels
    const int nout = (y1 - y0) * a.W;
    for (int q = tid; q < nout; q += kNarrowOutThreads) {
        const int qy = (int)(__umulhi((unsigned)q, a.magW) >> a.shW), xx = q - qy * a.W;
        const int yy = y0 + qy;
        float* op = a.out + (((int64_t)n * a.H + yy) * a.W + xx) * a.Cn;
        for (int c = 0; c < a.Cn; ++c) {
            float sum = 0.f;
            for (int r = 0; r < a.ks; ++r) {
                const int iy = yy - (r - pad);
                for (int s = 0; s < a.ks; ++s) {
                    const int ix = xx - (s - pad);
                    if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                        sum += zl[((iy - z0) * a.W + ix) * a.ld + (r * a.ks + s) * a.Cn + c];
                }
            }
            if constexpr (BIAS) sum += a.bias[c];
            op[c] = sum;
        }
    }
}

void magic_u31(unsigned d, unsigned* mag, unsigned* sh)
{
    // q = umulhi(m, mag) >> sh == m / d for m < 2^31, d >= 2
    unsigned s = 0;
    while ((1u << s) < d) ++s;
    const unsigned long long num = 1ull << (31 + s);
    *mag = (unsigned)((num + d - 1) / d);
    *sh = s - 1;
}

int grid_for(int64_t work_items)
{
    int64_t g = (work_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

template <int MB, int NB, bool KS = false>
hipError_t launch_conv(const ConvArgs& a, hipStream_t st)
{
    constexpr int LDS = 2 * (2 * MB * 4 * 1024 + 2 * NB * 4 * 1024);
    const int64_t M = (int64_t)a.N * a.H * a.W;
    if constexpr (MB == 2) {
        if (M % 128) {      // a partial last tile (wc_conv_ragged_supported): only ever on the 128-point tiles, conv_big_tile keeps M % 256 == 0
            hipError_t e = wc_set_max_lds(reinterpret_cast<const void*>(conv_f16x3_ragged_kernel<NB, KS>), LDS);
            if (e != hipSuccess) return e;
            dim3 grid((unsigned)((M + 127) / 128), (unsigned)(a.nphase * (a.Cout / (64 * NB))), (unsigned)a.ksplit);
            hipLaunchKernelGGL((conv_f16x3_ragged_kernel<NB, KS>), grid, dim3(256), LDS, st, a);
            return hipGetLastError();
        }
    }
    hipError_t e = wc_set_max_lds(reinterpret_cast<const void*>(conv_f16x3_kernel<MB, NB, KS>), LDS);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(M / (64 * MB)), (unsigned)(a.nphase * (a.Cout / (64 * NB))), (unsigned)a.ksplit);
    hipLaunchKernelGGL((conv_f16x3_kernel<MB, NB, KS>), grid, dim3(256), LDS, st, a);
    return hipGetLastError();
}

// the 128-point x 32-output tiles of a width that is 32 beyond a multiple of 64 (whole tiles: wc_conv_slim_supported)
template <bool KS>
hipError_t launch_conv_slim(const ConvArgs& a, hipStream_t st)
{
    constexpr int LDS = 2 * (4 * 4 * 1024 + 4 * 1024);
    const int64_t M = (int64_t)a.N * a.H * a.W;
    hipError_t e = wc_set_max_lds(reinterpret_cast<const void*>(conv_f16x3_slim_kernel<KS>), LDS);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)(M / 128), (unsigned)(a.nphase * (a.Cout / 32)), (unsigned)a.ksplit);
    hipLaunchKernelGGL((conv_f16x3_slim_kernel<KS>), grid, dim3(256), LDS, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" {

static int split_measured(const float* x, int64_t n, int relu, float slope, void* hi, void* lo, float* scale, void* amax_scratch,
                          float* colsum_partials, int C, hipStream_t st)
{
    if (!x || !hi || !lo || !scale || !amax_scratch || n <= 0 || (n & 3)) return WC_ERR_ARG;
    if (colsum_partials && (C <= 0 || (C & 3) || 256 % (C >> 2) != 0 || n % C != 0)) return WC_ERR_SHAPE;
    hipLaunchKernelGGL(conv_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, x, n / 4, n, (float*)amax_scratch,
                       colsum_partials, colsum_partials ? C >> 2 : 0, relu == 2 ? slope : -1.f);
    hipLaunchKernelGGL(conv_split_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, x, n / 4, (const float*)amax_scratch, relu,
                       (_Float16*)hi, (_Float16*)lo, scale, slope);
    return (int)hipGetLastError();
}

static int split_hist(const float* x, int64_t n, int relu, float slope, void* hi, void* lo, float* scale, float* colsum_partials, int C,
                      float* hist, int bootstrap, hipStream_t st)
{
    if (!x || !hi || !lo || !scale || !hist || n <= 0 || (n & 3)) return WC_ERR_ARG;
    if (colsum_partials && (C <= 0 || (C & 3) || 256 % (C >> 2) != 0 || n % C != 0)) return WC_ERR_SHAPE;
    if (bootstrap & 1) {   // the site's first call: the measured maximum (the two-launch form, bit for bit), left in the record
        hipLaunchKernelGGL(conv_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, x, n / 4, n, hist, colsum_partials, colsum_partials ? C >> 2 : 0,
                           relu == 2 ? slope : -1.f);
        hipLaunchKernelGGL(conv_split_kernel, dim3(grid_for(n / 4)), dim3(256), 0, st, x, n / 4, (const float*)hist, relu, (_Float16*)hi,
                           (_Float16*)lo, scale, slope);
        hipLaunchKernelGGL(conv_hist_seed_kernel, dim3(1), dim3(kAmaxBlocks), 0, st, hist);
        return (int)hipGetLastError();
    }
    // always kAmaxBlocks workgroups: they are the partial rows conv_wrw_reduce_kernel adds up
    hipLaunchKernelGGL(conv_split_hist_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, x, n / 4, relu, (_Float16*)hi, (_Float16*)lo, scale,
                       hist, colsum_partials, colsum_partials ? C >> 2 : 0, slope);
    if (!(bootstrap & 2)) {
        // (a small grid: inside the window -- the usual case -- the launch is 64 workgroups reading 8 KB each and returning; outside it they
        // stride over the tensor)
        const unsigned g2 = grid_for(n / 4) < 64u ? grid_for(n / 4) : 64u;
        hipLaunchKernelGGL(conv_split_redo_kernel, dim3(g2), dim3(256), 0, st, x, n / 4, relu, (_Float16*)hi, (_Float16*)lo, scale, hist, slope);
    }
    return (int)hipGetLastError();
}

int wc_conv_split_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, void* amax_scratch, wc_stream_t stream)
{
    return wc_conv_split_colsum_f32(x, n, relu, hi, lo, scale, amax_scratch, nullptr, 0, stream);
}

int wc_conv_split_colsum_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, void* amax_scratch,
                             float* colsum_partials, int C, wc_stream_t stream)
{
    return split_measured(x, n, relu ? 1 : 0, 0.f, hi, lo, scale, amax_scratch, colsum_partials, C, (hipStream_t)stream);
}

int wc_conv_split_hist_f32(const float* x, int64_t n, int relu, void* hi, void* lo, float* scale, float* colsum_partials, int C,
                           float* hist, int bootstrap, wc_stream_t stream)
{
    return split_hist(x, n, relu ? 1 : 0, 0.f, hi, lo, scale, colsum_partials, C, hist, bootstrap, (hipStream_t)stream);
}

// LeakyReLU in front of the split.  Slope 0 IS the ReLU: it takes the ReLU form (fmaxf: the same plane bits as relu = 1).
int wc_conv_split_leaky_f32(const float* x, int64_t n, float negative_slope, void* hi, void* lo, float* scale, void* amax_scratch,
                            float* colsum_partials, int C, wc_stream_t stream)
{
    if (!(negative_slope >= 0.f && negative_slope <= 1.f)) return WC_ERR_ARG;     // (the activation must not grow the tensor: the history's window is sized for |x|)
    return split_measured(x, n, negative_slope == 0.f ? 1 : 2, negative_slope, hi, lo, scale, amax_scratch, colsum_partials, C, (hipStream_t)stream);
}

int wc_conv_split_hist_leaky_f32(const float* x, int64_t n, float negative_slope, void* hi, void* lo, float* scale, float* colsum_partials, int C,
                                 float* hist, int bootstrap, wc_stream_t stream)
{
    if (!(negative_slope >= 0.f && negative_slope <= 1.f)) return WC_ERR_ARG;
    return split_hist(x, n, negative_slope == 0.f ? 1 : 2, negative_slope, hi, lo, scale, colsum_partials, C, hist, bootstrap, (hipStream_t)stream);
}

int wc_conv_leaky_bwd_f32(float* dx, const float* x, int64_t n, float negative_slope, wc_stream_t stream)
{
    if (!dx || !x || n <= 0 || (n & 3)) return WC_ERR_ARG;
    hipLaunchKernelGGL(conv_leaky_bwd_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, dx, x, n / 4, negative_slope);
    return (int)hipGetLastError();
}

size_t wc_conv_weights_bytes(const wc_conv_geom* g)
{
    if (!g) return 0;
    return (size_t)g->nphase * g->ntaps * g->Cin * g->Cout * 4;      // hi + lo halves
}

static int fill_weight_args(WeightArgs& a, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                            int64_t n_elems, const wc_conv_geom* g, void* image, float* scale, const float* amax, int amax_count)
{
    if (g->ntaps < 1 || g->ntaps > kMaxTaps || g->nphase < 1 || g->nphase > kMaxPhase || (g->Cin & 31) || (g->Cout & 31)) return WC_ERR_ARG;
    a.w = w; a.sk = stride_k; a.sn = stride_n; a.sr = stride_r; a.ss = stride_s;
    a.amax = amax; a.amax_count = amax_count; a.scale_out = scale; a.img = (char*)image;
    a.n4 = n_elems / 4;
    a.K = g->Cin; a.Nn = g->Cout; a.ntaps = g->ntaps; a.nphase = g->nphase;
    int most = 1;
    for (int p = 0; p < kMaxPhase; ++p)
        for (int t = 0; t < kMaxTaps; ++t) {
            a.nsrc[p][t] = g->nsrc[p][t];
            if (p < g->nphase && t < g->ntaps) {
                if (g->nsrc[p][t] < 1 || g->nsrc[p][t] > 4) return WC_ERR_ARG;
                if (g->nsrc[p][t] > most) most = g->nsrc[p][t];
            }
            for (int m = 0; m < 4; ++m) { a.r[p][t][m] = g->wr[p][t][m]; a.s[p][t][m] = g->ws[p][t][m]; }
        }
    a.coef = g->wcoef; a.bound_mul = fabsf(g->wcoef) * most;
    return WC_OK;
}

int wc_conv_weights_f32(const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, int64_t n_elems,
                        const wc_conv_geom* g, void* image, float* scale, void* amax_scratch,
                        const float* known_amax, int known_count, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!w || !g || !image || !scale || (!amax_scratch && !known_amax) || n_elems <= 0) return WC_ERR_ARG;
    if (known_amax && (known_count < 1 || known_count > 4096)) return WC_ERR_ARG;
    // the scale comes from the whole source tensor (n_elems covers its storage extent)
    const bool inline_max = !known_amax && n_elems <= 32768 && (n_elems & 3) == 0 && ((uintptr_t)w & 15) == 0;   // (a 128 x 128 x 1 x 1 shortcut)
    if (!inline_max && !known_amax) hipLaunchKernelGGL(conv_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, w, n_elems / 4, n_elems, (float*)amax_scratch);
    WeightArgs a;
    const int rc = fill_weight_args(a, w, stride_k, stride_n, stride_r, stride_s, n_elems, g, image, scale,
                                    inline_max ? nullptr : (known_amax ? known_amax : (const float*)amax_scratch), known_amax ? known_count : kAmaxBlocks);
    if (rc != WC_OK) return rc;
    const int64_t groups = (int64_t)g->nphase * g->ntaps * (g->Cin >> 5) * (g->Cout >> 5) * 128;
    hipLaunchKernelGGL(conv_weights_kernel, dim3(grid_for(groups)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

int wc_conv_weights_pair_f32(const float* w, int64_t stride_r, int64_t stride_s, int64_t n_elems,
                             int64_t a_stride_k, int64_t a_stride_n, const wc_conv_geom* ga, void* image_a,
                             int64_t b_stride_k, int64_t b_stride_n, const wc_conv_geom* gb, void* image_b,
                             float* scale, void* amax_scratch, const float* known_amax, int known_count, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!w || !ga || !gb || !image_a || !image_b || !scale || (!amax_scratch && !known_amax) || n_elems <= 0) return WC_ERR_ARG;
    if (known_amax && (known_count < 1 || known_count > 4096)) return WC_ERR_ARG;
    if (!known_amax) hipLaunchKernelGGL(conv_absmax_kernel, dim3(kAmaxBlocks), dim3(256), 0, st, w, n_elems / 4, n_elems, (float*)amax_scratch);
    const float* amax = known_amax ? known_amax : (const float*)amax_scratch;
    const int cnt = known_amax ? known_count : kAmaxBlocks;
    WeightArgs a, b;
    int rc = fill_weight_args(a, w, a_stride_k, a_stride_n, stride_r, stride_s, n_elems, ga, image_a, scale, amax, cnt);
    if (rc != WC_OK) return rc;
    rc = fill_weight_args(b, w, b_stride_k, b_stride_n, stride_r, stride_s, n_elems, gb, image_b, scale + 1, amax, cnt);
    if (rc != WC_OK) return rc;
    if (a.bound_mul != b.bound_mul) return WC_ERR_ARG;             // (one weight, one kind: the same scale both ways)
    const int blocks_a = grid_for((int64_t)ga->nphase * ga->ntaps * (ga->Cin >> 5) * (ga->Cout >> 5) * 128);
    const int blocks_b = grid_for((int64_t)gb->nphase * gb->ntaps * (gb->Cin >> 5) * (gb->Cout >> 5) * 128);
    hipLaunchKernelGGL(conv_weights_pair_kernel, dim3(blocks_a + blocks_b), dim3(256), 0, st, a, b, blocks_a);
    return (int)hipGetLastError();
}

// the table of a geometry kind: the entries conv_weights_body reads (phase < nphase, tap < ntaps, source < nsrc), zero elsewhere
static void fill_batch_table(BatchTable& t, const WeightArgs& a)
{
    memset(&t, 0, sizeof(t));
    t.ntaps = a.ntaps; t.nphase = a.nphase;
    for (int p = 0; p < a.nphase; ++p)
        for (int k = 0; k < a.ntaps; ++k) {
            t.nsrc[p][k] = a.nsrc[p][k];
            for (int m = 0; m < a.nsrc[p][k]; ++m) t.rs[p][k][m] = (unsigned char)(a.r[p][k][m] | (a.s[p][k][m] << 2));
        }
}

static int check_weights_job(const wc_conv_weights_job& j, WeightArgs& a)
{
    if (!j.w || !j.g || !j.image || !j.scale) return WC_ERR_NULL;
    if (j.n_elems <= 0) return WC_ERR_ARG;
    if (j.amax) { if (j.amax_count < 1 || j.amax_count > 4096) return WC_ERR_ARG; }
    else if (j.n_elems > 32768 || (j.n_elems & 3) || ((uintptr_t)j.w & 15)) return WC_ERR_ARG;   // (wc_conv_weights_f32's rule for the maximum taken inside)
    const int rc = fill_weight_args(a, j.w, j.stride_k, j.stride_n, j.stride_r, j.stride_s, j.n_elems, j.g, j.image, j.scale, j.amax,
                                    j.amax ? j.amax_count : 0);
    if (rc != WC_OK) return rc;
    for (int p = 0; p < a.nphase; ++p)
        for (int k = 0; k < a.ntaps; ++k)
            for (int m = 0; m < a.nsrc[p][k]; ++m)
                if (a.r[p][k][m] < 0 || a.r[p][k][m] > 3 || a.s[p][k][m] < 0 || a.s[p][k][m] > 3) return WC_ERR_ARG;
    return WC_OK;
}

// checks every job, then fills launches greedily (a launch ends at kBatchJobs jobs, kBatchTables distinct tables or kBatchBlocks
// workgroups); st == nullptr with launch == false: only counts them
static int weights_batch(const wc_conv_weights_job* jobs, int count, bool launch, hipStream_t st, int* launches)
{
    if (!jobs) return WC_ERR_NULL;
    if (count <= 0) return WC_ERR_SHAPE;
    *launches = 0;
    WeightArgs a, b;
    for (int i = 0; i < count; ++i) {
        int rc = check_weights_job(jobs[i], a);
        if (rc != WC_OK) return rc;
        const int p = jobs[i].pair_of;
        if (p < 0) continue;
        // the second image of a weight whose first is job p: one weight, one kind, the same scale both ways
        if (p >= i) return WC_ERR_ARG;
        rc = check_weights_job(jobs[p], b);
        if (rc != WC_OK) return rc;
        if (jobs[p].w != jobs[i].w || jobs[p].amax != jobs[i].amax || jobs[p].amax_count != jobs[i].amax_count
            || jobs[p].n_elems != jobs[i].n_elems || a.bound_mul != b.bound_mul) return WC_ERR_ARG;
    }
    for (int c0 = 0; c0 < count;) {
        WeightBatch q;
        memset(&q, 0, sizeof(q));
        int take = 0, blocks = 0, ntab = 0;
        while (c0 + take < count && take < kBatchJobs) {
            const wc_conv_weights_job& j = jobs[c0 + take];
            (void)check_weights_job(j, a);
            BatchTable t;
            fill_batch_table(t, a);
            int ti = 0;
            while (ti < ntab && memcmp(&q.table[ti], &t, sizeof(t)) != 0) ++ti;
            const int nb = grid_for((int64_t)a.nphase * a.ntaps * (a.K >> 5) * (a.Nn >> 5) * 128);
            if (take > 0 && (ti == kBatchTables || blocks + nb > kBatchBlocks)) break;
            if (ti == ntab) q.table[ntab++] = t;
            BatchJob& o = q.job[take];
            o.w = a.w; o.amax = a.amax; o.scale_out = a.scale_out; o.img = a.img;
            o.sk = a.sk; o.sn = a.sn; o.sr = a.sr; o.ss = a.ss; o.n4 = a.n4;
            o.K = a.K; o.Nn = a.Nn; o.coef = a.coef; o.bound_mul = a.bound_mul; o.amax_count = a.amax_count; o.table = ti;
            q.first[take] = blocks;
            blocks += nb; ++take;
        }
        q.first[take] = blocks;
        q.count = take;
        if (launch) hipLaunchKernelGGL(conv_weights_batch_kernel, dim3(blocks), dim3(256), 0, st, q);
        ++*launches;
        c0 += take;
    }
    return launch ? (int)hipGetLastError() : WC_OK;
}

int wc_conv_weights_batch_f32(const wc_conv_weights_job* jobs, int count, wc_stream_t stream)
{
    int launches;
    return weights_batch(jobs, count, true, (hipStream_t)stream, &launches);
}

int wc_conv_weights_batch_launches(const wc_conv_weights_job* jobs, int count)
{
    int launches = 0;
    const int rc = weights_batch(jobs, count, false, nullptr, &launches);
    return rc != WC_OK ? rc : launches;
}

int wc_conv_absmax_batch_f32(const wc_conv_absmax_job* jobs, int count, wc_stream_t stream)
{
    if (!jobs) return WC_ERR_NULL;
    if (count <= 0) return WC_ERR_SHAPE;
    for (int i = 0; i < count; ++i) {
        if (!jobs[i].x || !jobs[i].partial) return WC_ERR_NULL;
        if (jobs[i].n <= 0 || ((uintptr_t)jobs[i].x & 15)) return WC_ERR_ARG;
    }
    for (int c0 = 0; c0 < count; c0 += kAbsmaxJobs) {
        AbsmaxBatch q;
        memset(&q, 0, sizeof(q));
        const int take = count - c0 < kAbsmaxJobs ? count - c0 : kAbsmaxJobs;
        for (int i = 0; i < take; ++i) q.job[i] = AbsmaxJob{jobs[c0 + i].x, jobs[c0 + i].n, jobs[c0 + i].partial};
        hipLaunchKernelGGL(conv_absmax_batch_kernel, dim3(take * kAmaxBlocks), dim3(256), 0, (hipStream_t)stream, q);
    }
    return (int)hipGetLastError();
}

// rows: what N*H*W must be a multiple of -- 128 (whole tiles: wc_conv_supported) or 32 (whole m-blocks, a partial last tile:
// wc_conv_ragged_supported); every other rule is shared
static int conv_geom_ok(const wc_conv_geom* g, int rows, int cout_mask = 63)
{
    if (!g) return 0;
    if (g->ntaps < 1 || g->ntaps > kMaxTaps || g->nphase < 1 || g->nphase > kMaxPhase) return 0;
    if ((g->Cin & 31) || (g->Cout & cout_mask)) return 0;    // (Cout % 128 == 64: the 64-output tile <2, 1>; cout_mask 31: the slim set)
    const int64_t M = (int64_t)g->N * g->H * g->W;
    // (M <= 2^31 - 128: the last tile's rows past the grid stay below 2^31, where the multiply-shift division is exact)
    if (M <= 0 || (M % rows) || M > ((int64_t)1 << 31) - (rows == 128 ? 0 : 128)) return 0;
    if ((int64_t)g->N * g->Hin * g->Win > (int64_t)1 << 31) return 0;
    if (g->W < 2 || g->H < 1) return 0;             // (the multiply-shift division wants divisors >= 2)
    return 1;
}

int wc_conv_supported(const wc_conv_geom* g) { return conv_geom_ok(g, 128); }

// what the launch entries take: wc_conv_supported's set and the same geometries with N*H*W a multiple of 32 -- the last 128-point tile then
// has 32, 64 or 96 rows, the others read zeros and write nothing (conv_f16x3_body).  wc_conv_supported keeps its value: the layer entry of
// an unmarked layer (wc_gan_amd/conv.py) asks it.
int wc_conv_ragged_supported(const wc_conv_geom* g) { return conv_geom_ok(g, 32); }

// the third set the launch entries take: wc_conv_supported's rules with an output width that is any multiple of 32 -- a width 32 beyond a
// multiple of 64 runs on tiles of 32 outputs (conv_f16x3_slim_kernel), a weight gradient with such a side on 32 x 32 tiles
// (conv_wrw_slim_kernel).  Whole 128-point tiles only: a slim width on a partial last tile is in neither set.  The other two predicates
// keep their values; a layer built with slim_conv=True asks this one (wc_gan_amd/conv.py).
int wc_conv_slim_supported(const wc_conv_geom* g) { return conv_geom_ok(g, 128, 31); }

// what wc_conv_f16x3 / wc_conv_workspace_bytes take: the union
static int conv_takes(const wc_conv_geom* g) { return wc_conv_ragged_supported(g) || wc_conv_slim_supported(g); }

static int64_t conv_tiles(int64_t M) { return (M + 127) / 128; }       // 128-point tiles along x, the last one partial or whole

constexpr int kKsplitMaxWgs = 96;         // k-split only grids of at most this many output tiles ...
constexpr int kKsplitTargetWgs = 256;     // ... into about this many workgroups
constexpr int kWrwTargetWgs = 512;        // weight gradient: workgroups over all tiles and pixel ranges

static int conv_ksplit(const wc_conv_geom* g)
{
    // small grids leave most CUs idle with 128-point x (128|256)-output tiles: share the (tap, chunk) loop
    const int64_t M = (int64_t)g->N * g->H * g->W;
    const bool wide = (g->Cout % 256) == 0;
    // (a width 32 beyond a multiple of 64: tiles of 32 outputs -- never a tile count of zero)
    const int64_t wgs = conv_tiles(M) * g->nphase * (g->Cout / (wide ? 256 : (g->Cout % 64) ? 32 : (g->Cout % 128) ? 64 : 128));
    const int iters = g->ntaps * (g->Cin / 32);
    if (wgs > kKsplitMaxWgs || iters < 8) return 1;
    int k = (int)((kKsplitTargetWgs + wgs - 1) / wgs);
    if (k > iters / 4) k = iters / 4;               // at least 4 iterations each
    return k < 1 ? 1 : (k > 8 ? 8 : k);
}

size_t wc_conv_workspace_bytes(const wc_conv_geom* g)
{
    if (!g || g->Cout < 32) return 0;
    const int k = conv_ksplit(g);
    return k > 1 ? (size_t)k * g->N * g->Hout * g->Wout * g->Cout * 4 : 0;
}

// the 256-point tile <4, NB>: when it still gives every CU a workgroup
static bool conv_big_tile(const wc_conv_geom* g, int ksplit)
{
    const int64_t M = (int64_t)g->N * g->H * g->W;
    const bool wide = (g->Cout % 256) == 0;
    const int64_t wgs_big = (M / 256) * g->nphase * (g->Cout / (wide ? 256 : 128));
    if (g->Cout % 128) return false;                // (the 64- and 32-output tiles have no 256-point form)
    return ksplit == 1 && (M % 256) == 0 && wgs_big >= 256;
}

// argument checks and the kernel's argument block of wc_conv_f16x3 (shared with wc_conv_bwd_pair_f16x3)
static int conv_prepare(ConvArgs& a, const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                        const float* bias, const void* zero_line, const wc_conv_geom* g, int relu, float* y, void* ws, size_t ws_bytes,
                        bool need_ws = true)
{
    if (!xhi || !xlo || !xscale || !wimage || !wscale || !zero_line || !g || !y) return WC_ERR_ARG;
    if (!conv_takes(g)) return WC_ERR_SHAPE;
    a.xhi = (const _Float16*)xhi; a.xlo = (const _Float16*)xlo; a.zero = (const _Float16*)zero_line;
    a.wimg = (const char*)wimage; a.xscale = xscale; a.wscale = wscale; a.bias = bias; a.y = y;
    a.N = g->N; a.H = g->H; a.W = g->W; a.Hin = g->Hin; a.Win = g->Win; a.Cin = g->Cin; a.Cout = g->Cout;
    a.in_stride = g->in_stride; a.ntaps = g->ntaps; a.nphase = g->nphase; a.Hout = g->Hout; a.Wout = g->Wout;
    a.out_stride = g->out_stride; a.relu = relu;
    a.ksplit = conv_ksplit(g); a.partial = (float*)ws;
    magic_u31((unsigned)(g->H * g->W), &a.magHW, &a.shHW);
    magic_u31((unsigned)g->W, &a.magW, &a.shW);
    if (need_ws && a.ksplit > 1 && (!ws || ws_bytes < wc_conv_workspace_bytes(g))) return WC_ERR_WORKSPACE;
    for (int p = 0; p < kMaxPhase; ++p) {
        a.offy[p] = g->off_y[p]; a.offx[p] = g->off_x[p];
        for (int t = 0; t < kMaxTaps; ++t) { a.dy[p][t] = g->dy[p][t]; a.dx[p][t] = g->dx[p][t]; }
    }
    return WC_OK;
}

int wc_conv_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                  const float* bias, const void* zero_line, const wc_conv_geom* g, int relu, float* y,
                  void* ws, size_t ws_bytes, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    ConvArgs a;
    const int rc = conv_prepare(a, xhi, xlo, xscale, wimage, wscale, bias, zero_line, g, relu, y, ws, ws_bytes);
    if (rc != WC_OK) return rc;
    const bool wide = (g->Cout % 256) == 0;
    hipError_t e;
    if (g->Cout % 64)                                       e = a.ksplit > 1 ? launch_conv_slim<true>(a, st) : launch_conv_slim<false>(a, st);
    else if (g->Cout % 128)                                 e = a.ksplit > 1 ? launch_conv<2, 1, true>(a, st) : launch_conv<2, 1>(a, st);
    else if (conv_big_tile(g, a.ksplit))                    e = wide ? launch_conv<4, 4>(a, st) : launch_conv<4, 2>(a, st);
    else if (a.ksplit > 1)                                  e = wide ? launch_conv<2, 4, true>(a, st) : launch_conv<2, 2, true>(a, st);
    else                                                    e = wide ? launch_conv<2, 4>(a, st) : launch_conv<2, 2>(a, st);
    if (e != hipSuccess) return (int)e;
    if (a.ksplit > 1) {
        const int64_t n4 = (int64_t)g->N * g->Hout * g->Wout * g->Cout / 4;
        hipLaunchKernelGGL(conv_ksplit_reduce_kernel, dim3(grid_for(n4)), dim3(256), 0, st, (const float*)ws, a.ksplit, n4, g->Cout,
                           xscale, wscale, bias, relu, y);
    }
    return (int)hipGetLastError();
}

// wc_conv_f16x3 with the residual operand in the k-split finish: only geometries whose tap loop is shared (wc_conv_workspace_bytes > 0)
// and whose width is a multiple of 128 -- the critic's conv2 at 8x8 and 16->8; the tiles' direct epilogue (and with it every
// conv_f16x3_kernel instantiation's code) is left as it is, its caller adds the residual itself.
int wc_conv_res_supported(const wc_conv_geom* g)
{
    return g && wc_conv_ragged_supported(g) && (g->Cout % 128) == 0 && conv_ksplit(g) > 1;
}

int wc_conv_res_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                      const float* bias, const float* res, const void* zero_line, const wc_conv_geom* g, float* y,
                      void* ws, size_t ws_bytes, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!res) return WC_ERR_ARG;
    ConvArgs a;
    const int rc = conv_prepare(a, xhi, xlo, xscale, wimage, wscale, bias, zero_line, g, 0, y, ws, ws_bytes);
    if (rc != WC_OK) return rc;
    if (!wc_conv_res_supported(g)) return WC_ERR_SHAPE;
    const hipError_t e = (g->Cout % 256) == 0 ? launch_conv<2, 4, true>(a, st) : launch_conv<2, 2, true>(a, st);
    if (e != hipSuccess) return (int)e;
    const int64_t n4 = (int64_t)g->N * g->Hout * g->Wout * g->Cout / 4;
    hipLaunchKernelGGL(conv_ksplit_reduce_res_kernel, dim3(grid_for(n4)), dim3(256), 0, st, (const float*)ws, a.ksplit, n4, g->Cout,
                       xscale, wscale, bias, res, y);
    return (int)hipGetLastError();
}

// ---- a k-split finish with its follower's work (conv_finish_tail_kernel): wc_conv_tail_f16x3, wc_conv_bwd_pair_tail_f16x3 ----------------
int wc_conv_tail_supported(const wc_conv_geom* g)
{
    return wc_conv_res_supported(g);                // a shared tap loop (so there IS a finish launch) on 128-wide tiles
}

// the tail's own operands against the convolution's output [N][Hout][Wout][Cout] -> the finish launch's argument block
static int tail_prepare(FinishTailArgs& f, const wc_conv_tail* t, const ConvArgs& a, const wc_conv_geom* g, const float* xscale,
                        const float* wscale, const float* bias, float* y, const void* ws)
{
    if (!t) return WC_ERR_NULL;
    if (!wc_conv_tail_supported(g)) return WC_ERR_SHAPE;
    memset(&f, 0, sizeof(f));
    f.k.n4 = (int64_t)g->N * g->Hout * g->Wout * g->Cout / 4;
    f.k.partial = (const float*)ws; f.k.ksplit = a.ksplit; f.k.cout = g->Cout;
    f.k.xscale = xscale; f.k.wscale = wscale; f.k.bias = bias; f.k.relu = 0; f.k.y = y;
    if (t->kind == WC_CONV_TAIL_DX) {
        if (!t->mask || !t->other || !t->out) return WC_ERR_NULL;
        if (t->out == t->mask || t->out == t->other) return WC_ERR_ARG;
        f.mask = t->mask; f.other = t->other; f.out = t->out;
        return WC_OK;
    }
    if (t->kind != WC_CONV_TAIL_SPLIT && t->kind != WC_CONV_TAIL_MASKED) return WC_ERR_ARG;
    if (!y || !t->hi || !t->lo || !t->scale || !t->hist) return WC_ERR_NULL;
    f.hi = (_Float16*)t->hi; f.lo = (_Float16*)t->lo; f.scale_out = t->scale; f.hist = t->hist;
    if (t->kind == WC_CONV_TAIL_SPLIT) { f.res = t->res; return WC_OK; }
    if (!t->mask) return WC_ERR_NULL;
    f.mask = t->mask;
    if (t->colsum_partials) {                       // (split_hist's rule: a thread of the 512 x 256 grid always sees the same 4 channels)
        if (t->C != g->Cout || (t->C & 3) || 256 % (t->C >> 2) != 0) return WC_ERR_SHAPE;
        f.colsum = t->colsum_partials; f.c4n = t->C >> 2;
    }
    return WC_OK;
}

// the gated second pass of a SPLIT or MASKED tail: the launches wc_conv_split_hist_f32 / wc_conv_split_hist_masked_f32 put behind theirs
static int tail_redo(const wc_conv_tail* t, const FinishTailArgs& f, hipStream_t st)
{
    if (t->kind == WC_CONV_TAIL_DX || !t->redo) return WC_OK;
    const int64_t n4 = f.k.n4;
    if (t->kind == WC_CONV_TAIL_MASKED)
        return wc_conv_split_redo_masked_f32(f.k.y, f.mask, 4 * n4, 0.f, t->hi, t->lo, t->scale, t->hist, (wc_stream_t)st);
    const unsigned g2 = grid_for(n4) < 64u ? grid_for(n4) : 64u;
    hipLaunchKernelGGL(conv_split_redo_kernel, dim3(g2), dim3(256), 0, st, (const float*)f.k.y, n4, 1, f.hi, f.lo, f.scale_out, f.hist, 0.f);
    return (int)hipGetLastError();
}

int wc_conv_tail_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                       const float* bias, const void* zero_line, const wc_conv_geom* g, float* y,
                       void* ws, size_t ws_bytes, const wc_conv_tail* tail, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!tail) return WC_ERR_NULL;
    ConvArgs a;
    if (tail->kind == WC_CONV_TAIL_DX && !tail->out) return WC_ERR_NULL;
    float* y_or_out = tail->kind == WC_CONV_TAIL_DX ? tail->out : y;        // (DX: no fp32 copy of the convolution's own output)
    const int rc = conv_prepare(a, xhi, xlo, xscale, wimage, wscale, bias, zero_line, g, 0, y_or_out, ws, ws_bytes);
    if (rc != WC_OK) return rc;
    FinishTailArgs f;
    const int rt = tail_prepare(f, tail, a, g, xscale, wscale, bias, y, ws);
    if (rt != WC_OK) return rt;
    const hipError_t e = (g->Cout % 256) == 0 ? launch_conv<2, 4, true>(a, st) : launch_conv<2, 2, true>(a, st);
    if (e != hipSuccess) return (int)e;
    if (tail->kind == WC_CONV_TAIL_SPLIT) hipLaunchKernelGGL((conv_finish_tail_kernel<kTailSplit>), dim3(kAmaxBlocks), dim3(256), 0, st, f);
    else if (tail->kind == WC_CONV_TAIL_MASKED) hipLaunchKernelGGL((conv_finish_tail_kernel<kTailMasked>), dim3(kAmaxBlocks), dim3(256), 0, st, f);
    else hipLaunchKernelGGL((conv_finish_tail_kernel<kTailDx>), dim3(grid_for(f.k.n4)), dim3(256), 0, st, f);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) return (int)e2;
    return tail_redo(tail, f, st);
}

// ---- the k-split's shares summed inside the workgroup (conv_local_kernel): wc_conv_local_supported, wc_conv_local_f16x3 ------------------
// the device's CU count; without a device (a predicate asked on a build machine) gfx950's 256
static int local_cus()
{
    static int cus = 0;
    if (cus > 0) return cus;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    return cus = n;
}

int wc_conv_local_supported(const wc_conv_geom* g)
{
    if (!wc_conv_supported(g)) return 0;            // whole tiles: no ragged grid
    if ((g->Cout % 128) != 0 || (g->Cout % 256) == 0 || (g->Cin % 64) != 0) return 0;
    if (conv_ksplit(g) != 4) return 0;              // four waves = four shares (eight wave-private double stages do not fit the LDS)
    const int64_t wgs = ((int64_t)g->N * g->H * g->W / 64) * g->nphase * (g->Cout / 64);
    return wgs <= local_cus() && wgs <= kAmaxBlocks;        // one workgroup (128 KiB of LDS) per CU; a pair of the reader's record each
}

int wc_conv_local_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* wimage, const float* wscale,
                        const float* bias, const float* res, const void* zero_line, const wc_conv_geom* g, int relu, float* y,
                        const wc_conv_tail* tail, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int kind = tail ? tail->kind : kTailNone;
    if (tail && kind == WC_CONV_TAIL_DX && !tail->out) return WC_ERR_NULL;
    if ((res && relu) || (tail && (res || relu))) return WC_ERR_ARG;        // (a tail brings its own residual; no ReLU in front of either)
    ConvArgs a;
    float* y_or_out = kind == WC_CONV_TAIL_DX ? tail->out : y;              // (DX: no fp32 copy of the convolution's own output)
    const int rc = conv_prepare(a, xhi, xlo, xscale, wimage, wscale, bias, zero_line, g, relu, y_or_out, nullptr, 0, false);
    if (rc != WC_OK) return rc;
    if (!wc_conv_local_supported(g)) return WC_ERR_SHAPE;
    FinishTailArgs f;
    if (tail) {
        const int rt = tail_prepare(f, tail, a, g, xscale, wscale, bias, y, nullptr);
        if (rt != WC_OK) return rt;
        if (f.colsum) return WC_ERR_SHAPE;          // (the partial rows' summation order belongs to the 512 x 256 grid)
    } else {
        memset(&f, 0, sizeof(f));
        f.k.cout = g->Cout; f.k.bias = bias; f.k.relu = relu; f.k.y = y; f.res = res;
    }
    constexpr int LDS = 4 * kLocalWaveBytes;
    const void* kernel = kind == WC_CONV_TAIL_SPLIT ? reinterpret_cast<const void*>(conv_local_kernel<kTailSplit>)
                       : kind == WC_CONV_TAIL_MASKED ? reinterpret_cast<const void*>(conv_local_kernel<kTailMasked>)
                       : kind == WC_CONV_TAIL_DX ? reinterpret_cast<const void*>(conv_local_kernel<kTailDx>)
                       : reinterpret_cast<const void*>(conv_local_kernel<kTailNone>);
    const hipError_t e = wc_set_max_lds(kernel, LDS);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)((int64_t)g->N * g->H * g->W / 64), (unsigned)(g->nphase * (g->Cout / 64)));
    if (kind == WC_CONV_TAIL_SPLIT) hipLaunchKernelGGL((conv_local_kernel<kTailSplit>), grid, dim3(256), LDS, st, a, f);
    else if (kind == WC_CONV_TAIL_MASKED) hipLaunchKernelGGL((conv_local_kernel<kTailMasked>), grid, dim3(256), LDS, st, a, f);
    else if (kind == WC_CONV_TAIL_DX) hipLaunchKernelGGL((conv_local_kernel<kTailDx>), grid, dim3(256), LDS, st, a, f);
    else hipLaunchKernelGGL((conv_local_kernel<kTailNone>), grid, dim3(256), LDS, st, a, f);
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) return (int)e2;
    return tail ? tail_redo(tail, f, st) : WC_OK;
}

int wc_conv_block_dx_f32(const float* dx1, const float* x, const float* other, int64_t N, int64_t H, int64_t W, int C, int down,
                         float* out, wc_stream_t stream)
{
    if (!dx1 || !x || !other || !out) return WC_ERR_NULL;
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || H > 0x7fffffff || W > 0x7fffffff) return WC_ERR_SHAPE;
    if (down && ((H & 1) || (W & 1))) return WC_ERR_SHAPE;
    const int64_t n4 = N * H * W * (C >> 2);
    hipStream_t st = (hipStream_t)stream;
    if (down) hipLaunchKernelGGL(conv_block_dx_kernel<true>, dim3(grid_for(n4)), dim3(256), 0, st, dx1, x, other, n4, C >> 2, (int)W, (int)H, out);
    else      hipLaunchKernelGGL(conv_block_dx_kernel<false>, dim3(grid_for(n4)), dim3(256), 0, st, dx1, x, other, n4, C >> 2, (int)W, (int)H, out);
    return (int)hipGetLastError();
}

static int wrw_splits(const wc_conv_geom* g, int* tile)
{
    // 256 x 256 tiles when there are enough of them (a 1x1 convolution has one slice: 128 x 128 tiles then)
    const bool wide = (g->Cin % 256 == 0) && (g->Cout % 256 == 0) && g->nphase * g->ntaps * (g->Cin / 256) * (g->Cout / 256) >= 4;
    *tile = wide ? 256 : ((g->Cin % 128) || (g->Cout % 128)) ? 64 : 128;     // (a 64-channel side: 64 x 64 tiles)
    if ((g->Cin % 64) || (g->Cout % 64)) *tile = 32;                          // (a 32-channel side: 32 x 32 tiles, conv_wrw_slim_kernel)
    const int tiles = g->nphase * g->ntaps * (g->Cin / *tile) * (g->Cout / *tile);
    const int64_t nchunks = (int64_t)g->N * g->H * g->W / 32;
    if (*tile == 32) {
        // a range is a WAVE here (four to a workgroup) and a partial sum is 4 KiB a slice: about 2048 waves over all tiles, in
        // multiples of 32 ranges = 8 workgroups (the XCD argument below), at most 256
        int64_t ranges = 2048 / (tiles < 1 ? 1 : tiles) / 32 * 32;
        if (ranges < 32) ranges = 32;
        if (ranges > 256) ranges = 256;
        if (ranges > nchunks) ranges = nchunks;
        return ranges < 1 ? 1 : (int)ranges;
    }
    // The workgroups of one pixel range (one per slice and tile) read the same activations: a split count that is a
    // multiple of 8 puts them on one XCD (workgroup id mod 8), i.e. behind one L2 -- measured 650 against 790 us at
    // 128 x 32 x 32 x 256 x 256 for 56 against 28 ranges.  About two workgroups per CU in all.
    int splits = kWrwTargetWgs / tiles / 8 * 8;
    if (splits < 8) splits = 8;
    if (splits > 64) splits = 64;                   // (the partial sums are splits x the weight size)
    if (splits > nchunks) splits = (int)nchunks;
    return splits < 1 ? 1 : splits;
}

int wc_conv_wrw_narrow_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int wc_conv_narrow64_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);
int wc_conv_narrow32_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize);

// the argument block and grid of the narrow forward (both entries below: one source for the tiling)
static dim3 narrow_fwd_args(NarrowFwdArgs& a, const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r,
                            int64_t stride_s, const float* bias, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu, float* y,
                            int nq = kNarrowNQ)
{
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cin = Cin; a.Cout = Cout; a.ks = ksize; a.nrow = ksize * ksize * Cin; a.relu = relu;
    a.sk = stride_k; a.sn = stride_n; a.sr = stride_r; a.ss = stride_s;
    magic_u31((unsigned)(H * W), &a.magHW, &a.shHW);
    magic_u31((unsigned)W, &a.magW, &a.shW);
    for (int m = 0; m < 32; ++m) {
        const int tap = m < a.nrow ? m / Cin : 0, c = m < a.nrow ? m % Cin : 0;
        a.tr[m] = (signed char)(tap / ksize); a.ts[m] = (signed char)(tap % ksize); a.tch[m] = (signed char)c;
        a.tdy[m] = (signed char)(tap / ksize - ksize / 2); a.tdx[m] = (signed char)(tap % ksize - ksize / 2);
    }
    a.M = N * H * W;
    a.ntiles = (int)((a.M + 31) / 32);
    a.tiles_per_wave = (a.ntiles + 1023) / 1024;           // x Cout / 64 workgroup columns: ~2 waves per SIMD at Cout = 128 (three, at 166 registers: 32.8 against 30.7 us)
    // (32-channel columns, wc_conv_fwd_narrow32_f32: a 32 -> 3 layer's data gradient has ONE column -- 4096 waves over the columns, four
    // per SIMD, to keep the stores of a pass that only writes in flight)
    if (nq == 1) a.tiles_per_wave = (int)(((int64_t)a.ntiles * (Cout / 32) + 4095) / 4096);
    if (a.tiles_per_wave < 1) a.tiles_per_wave = 1;
    const int nwg = (a.ntiles + 4 * a.tiles_per_wave - 1) / (4 * a.tiles_per_wave);
    return dim3(nwg, Cout / (32 * nq));
}

int wc_conv_fwd_narrow_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                           const float* bias, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu, float* y, wc_stream_t stream)
{
    if (!x || !w || !y) return WC_ERR_ARG;
    if (!wc_conv_narrow64_supported(N, H, W, Cin, Cout, ksize) || N * H * W * Cin >= ((int64_t)1 << 31)) return WC_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    NarrowFwdArgs a = {};
    const dim3 grid = narrow_fwd_args(a, x, w, stride_k, stride_n, stride_r, stride_s, bias, N, H, W, Cin, Cout, ksize, relu, y);
    const int ks2 = (a.nrow + 2) / 2;                      // k-steps: the taps' rows + the bias row, in pairs
    if (ks2 <= 2) hipLaunchKernelGGL(conv_fwd_narrow_kernel<2>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 5) hipLaunchKernelGGL(conv_fwd_narrow_kernel<5>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 10) hipLaunchKernelGGL(conv_fwd_narrow_kernel<10>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 14) hipLaunchKernelGGL(conv_fwd_narrow_kernel<14>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(conv_fwd_narrow_kernel<16>, grid, dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

// The same contract on the wider shape set (wc_conv_narrow32_supported).  Cout % 64 == 0: wc_conv_fwd_narrow_f32's launch.  Cout % 64 == 32:
// conv_fwd_narrow32_kernel, one 32-channel block per wave, on every column of the layer.
int wc_conv_fwd_narrow32_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                             const float* bias, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu, float* y, wc_stream_t stream)
{
    if (!x || !w || !y) return WC_ERR_ARG;
    // (the kernel's 32-bit element offset pc * Cin + off)
    if (!wc_conv_narrow32_supported(N, H, W, Cin, Cout, ksize) || N * H * W * Cin >= ((int64_t)1 << 31)) return WC_ERR_SHAPE;
    if ((Cout & 63) == 0) return wc_conv_fwd_narrow_f32(x, w, stride_k, stride_n, stride_r, stride_s, bias, N, H, W, Cin, Cout, ksize, relu, y, stream);
    hipStream_t st = (hipStream_t)stream;
    NarrowFwdArgs a = {};
    const dim3 grid = narrow_fwd_args(a, x, w, stride_k, stride_n, stride_r, stride_s, bias, N, H, W, Cin, Cout, ksize, relu, y, 1);
    const int ks2 = (a.nrow + 2) / 2;
    if (ks2 <= 2) hipLaunchKernelGGL(conv_fwd_narrow32_kernel<2>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 5) hipLaunchKernelGGL(conv_fwd_narrow32_kernel<5>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 10) hipLaunchKernelGGL(conv_fwd_narrow32_kernel<10>, grid, dim3(256), 0, st, a);
    else if (ks2 <= 14) hipLaunchKernelGGL(conv_fwd_narrow32_kernel<14>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(conv_fwd_narrow32_kernel<16>, grid, dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

// every workgroup of the split variant owns at least one pair of the reader's record: a grid of at most kAmaxBlocks workgroups
int wc_conv_fwd_narrow_split_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    if (!wc_conv_narrow64_supported(N, H, W, Cin, Cout, ksize) || N * H * W * Cin >= ((int64_t)1 << 31)) return 0;
    NarrowFwdArgs a = {};
    const dim3 grid = narrow_fwd_args(a, nullptr, nullptr, 0, 0, 0, 0, nullptr, N, H, W, Cin, Cout, ksize, 0, nullptr);
    return (int64_t)grid.x * grid.y <= kAmaxBlocks ? 1 : 0;
}

int wc_conv_fwd_narrow_split_f32(const float* x, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                 const float* bias, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize, int relu, float slope,
                                 float* y, void* hi, void* lo, float* scale, float* hist, int flags, wc_stream_t stream)
{
    if (!x || !w || !y || !hi || !lo || !scale || !hist || relu < 0 || relu > 2 || (flags & ~(WC_NARROW_SPLIT_NO_REDO | WC_NARROW_SPLIT_NT)))
        return WC_ERR_ARG;
    if (!wc_conv_fwd_narrow_split_supported(N, H, W, Cin, Cout, ksize)) return WC_ERR_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    NarrowFwdArgs a = {};
    const dim3 grid = narrow_fwd_args(a, x, w, stride_k, stride_n, stride_r, stride_s, bias, N, H, W, Cin, Cout, ksize, 0, y);
    NarrowSplitArgs s = {(_Float16*)hi, (_Float16*)lo, scale, hist, relu, slope, (flags & WC_NARROW_SPLIT_NT) ? 1 : 0};
    const int ks2 = (a.nrow + 2) / 2;
    if (ks2 <= 2) hipLaunchKernelGGL(conv_fwd_narrow_split_kernel<2>, grid, dim3(256), 0, st, a, s);
    else if (ks2 <= 5) hipLaunchKernelGGL(conv_fwd_narrow_split_kernel<5>, grid, dim3(256), 0, st, a, s);
    else if (ks2 <= 10) hipLaunchKernelGGL(conv_fwd_narrow_split_kernel<10>, grid, dim3(256), 0, st, a, s);
    else if (ks2 <= 14) hipLaunchKernelGGL(conv_fwd_narrow_split_kernel<14>, grid, dim3(256), 0, st, a, s);
    else hipLaunchKernelGGL(conv_fwd_narrow_split_kernel<16>, grid, dim3(256), 0, st, a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || (flags & WC_NARROW_SPLIT_NO_REDO)) return (int)e;
    // the gated second pass: split_hist's launch behind its own, on y
    const int64_t n4 = a.M * Cout / 4;
    const unsigned g2 = grid_for(n4) < 64u ? grid_for(n4) : 64u;
    hipLaunchKernelGGL(conv_split_redo_kernel, dim3(g2), dim3(256), 0, st, (const float*)y, n4, relu, (_Float16*)hi, (_Float16*)lo, scale, hist, slope);
    return (int)hipGetLastError();
}

static int64_t narrow_wrw_parts(int64_t M, int64_t* pix_per_wave)
{
    int64_t ppw = (M + 256 * 8 - 1) / (256 * 8);
    if (ppw < 16) ppw = 16;                          // at least one batch of eight pixel pairs per wave
    ppw = (ppw + 1) & ~(int64_t)1;
    *pix_per_wave = ppw;
    return (M + 8 * ppw - 1) / (8 * ppw);
}

int wc_conv_narrow64_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return 0;
    if (ksize * ksize * Cin >= 32 || (Cout & 63)) return 0;
    if (W < 2) return 0;                             // the multiply-shift division wants divisors >= 2 (conv_geom_ok's line)
    return N * H * W < ((int64_t)1 << 31) ? 1 : 0;
}

// wc_conv_narrow64_supported with Cout in 32s: the whole set of the narrow32 entries
int wc_conv_narrow32_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3)) return 0;
    if (ksize * ksize * Cin >= 32 || (Cout & 31)) return 0;
    if (W < 2) return 0;
    return N * H * W < ((int64_t)1 << 31) ? 1 : 0;
}

// (the ABI 7 predicate: multiples of 128 only; wc_conv_narrow64_supported is the whole set)
int wc_conv_wrw_narrow_supported(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    return ((Cout & 127) == 0 && wc_conv_narrow64_supported(N, H, W, Cin, Cout, ksize)) ? 1 : 0;
}

size_t wc_conv_wrw_narrow64_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    if (!wc_conv_narrow64_supported(N, H, W, Cin, Cout, ksize)) return 0;
    int64_t ppw;
    return (size_t)narrow_wrw_parts(N * H * W, &ppw) * ((Cout + 127) / 128) * 4096 * sizeof(float);
}

size_t wc_conv_wrw_narrow_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    return wc_conv_wrw_narrow_supported(N, H, W, Cin, Cout, ksize) ? wc_conv_wrw_narrow64_workspace_bytes(N, H, W, Cin, Cout, ksize) : 0;
}

// mask: nullptr = the plain kernel; else gy's shape, the ReLU's pre-activation applied as gy is read (conv_wrw_narrow_masked_kernel)
static int wrw_narrow64(const float* x, const float* gy, const float* mask, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                        float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db,
                        void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!x || !gy || !dw || !ws) return WC_ERR_ARG;
    if (!wc_conv_narrow64_supported(N, H, W, Cin, Cout, ksize)) return WC_ERR_SHAPE;
    if (ws_bytes < wc_conv_wrw_narrow64_workspace_bytes(N, H, W, Cin, Cout, ksize)) return WC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    NarrowWrwArgs a = {};
    a.x = x; a.gy = gy; a.partial = (float*)ws;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cin = Cin; a.Cout = Cout; a.ks = ksize; a.nrow = ksize * ksize * Cin;
    magic_u31((unsigned)(H * W), &a.magHW, &a.shHW);
    magic_u31((unsigned)W, &a.magW, &a.shW);
    a.M = N * H * W;
    const int nparts = (int)narrow_wrw_parts(a.M, &a.pix_per_wave);
    const int ngrp = (Cout + 127) / 128;
    constexpr int lds = 8 * 4096 * 4;
    hipError_t e = wc_set_max_lds(mask ? reinterpret_cast<const void*>(conv_wrw_narrow_masked_kernel)
                                       : reinterpret_cast<const void*>(conv_wrw_narrow_kernel), lds);
    if (e != hipSuccess) return (int)e;
    if (mask) hipLaunchKernelGGL(conv_wrw_narrow_masked_kernel, dim3(nparts, ngrp), dim3(512), lds, st, a, mask);
    else hipLaunchKernelGGL(conv_wrw_narrow_kernel, dim3(nparts, ngrp), dim3(512), lds, st, a);
    hipLaunchKernelGGL(conv_wrw_narrow_reduce_kernel, dim3(128, ngrp), dim3(256), 0, st, (const float*)ws, nparts, Cin, ksize, a.nrow,
                       dw, stride_k, stride_n, stride_r, stride_s, db, Cout);
    return (int)hipGetLastError();
}

int wc_conv_wrw_narrow64_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                             float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db,
                             void* ws, size_t ws_bytes, wc_stream_t stream)
{
    return wrw_narrow64(x, gy, nullptr, N, H, W, Cin, Cout, ksize, dw, stride_k, stride_n, stride_r, stride_s, db, ws, ws_bytes, stream);
}

int wc_conv_wrw_narrow_masked_f32(const float* x, const float* gy, const float* mask, int64_t N, int64_t H, int64_t W, int Cin, int Cout,
                                  int ksize, float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db,
                                  void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!mask) return WC_ERR_ARG;
    return wrw_narrow64(x, gy, mask, N, H, W, Cin, Cout, ksize, dw, stride_k, stride_n, stride_r, stride_s, db, ws, ws_bytes, stream);
}

// Cout % 64 == 0: wc_conv_wrw_narrow64_f32's size and launches.  Cout % 64 == 32: every group 32 wide, one partial of 1024 floats per
// (pixel range, group) -- the same bytes per channel.
size_t wc_conv_wrw_narrow32_workspace_bytes(int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize)
{
    if (!wc_conv_narrow32_supported(N, H, W, Cin, Cout, ksize)) return 0;
    if ((Cout & 63) == 0) return wc_conv_wrw_narrow64_workspace_bytes(N, H, W, Cin, Cout, ksize);
    int64_t ppw;
    return (size_t)narrow_wrw_parts(N * H * W, &ppw) * (Cout / 32) * 1024 * sizeof(float);
}

int wc_conv_wrw_narrow32_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                             float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db,
                             void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!x || !gy || !dw || !ws) return WC_ERR_ARG;
    if (!wc_conv_narrow32_supported(N, H, W, Cin, Cout, ksize)) return WC_ERR_SHAPE;
    if ((Cout & 63) == 0)
        return wrw_narrow64(x, gy, nullptr, N, H, W, Cin, Cout, ksize, dw, stride_k, stride_n, stride_r, stride_s, db, ws, ws_bytes, stream);
    if (ws_bytes < wc_conv_wrw_narrow32_workspace_bytes(N, H, W, Cin, Cout, ksize)) return WC_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    NarrowWrwArgs a = {};
    a.x = x; a.gy = gy; a.partial = (float*)ws;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cin = Cin; a.Cout = Cout; a.ks = ksize; a.nrow = ksize * ksize * Cin;
    magic_u31((unsigned)(H * W), &a.magHW, &a.shHW);
    magic_u31((unsigned)W, &a.magW, &a.shW);
    a.M = N * H * W;
    const int nparts = (int)narrow_wrw_parts(a.M, &a.pix_per_wave);
    const int ngrp = Cout / 32;
    hipLaunchKernelGGL(conv_wrw_narrow32_kernel, dim3(nparts, ngrp), dim3(512), 0, st, a);
    hipLaunchKernelGGL(conv_wrw_narrow32_reduce_kernel, dim3(32, ngrp), dim3(256), 0, st, (const float*)ws, nparts, Cin, ksize, a.nrow,
                       dw, stride_k, stride_n, stride_r, stride_s, db, Cout);
    return (int)hipGetLastError();
}

int wc_conv_wrw_narrow_f32(const float* x, const float* gy, int64_t N, int64_t H, int64_t W, int Cin, int Cout, int ksize,
                           float* dw, int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s, float* db,
                           void* ws, size_t ws_bytes, wc_stream_t stream)
{
    if (!x || !gy || !dw || !ws) return WC_ERR_ARG;
    if (!wc_conv_wrw_narrow_supported(N, H, W, Cin, Cout, ksize)) return WC_ERR_SHAPE;
    return wc_conv_wrw_narrow64_f32(x, gy, N, H, W, Cin, Cout, ksize, dw, stride_k, stride_n, stride_r, stride_s, db, ws, ws_bytes, stream);
}

// the band plan of the narrow-output convolution: false where the weight rows and ks image rows of Z do not fit the workgroup's LDS
static bool narrow_out_plan(NarrowOutArgs& a, int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize)
{
    if (N <= 0 || H <= 0 || W < 2 || Cw <= 0 || Cn <= 0 || (ksize != 1 && ksize != 3)) return false;     // (W >= 2: the multiply-shift division)
    if (ksize * ksize * Cn >= 32 || (Cw & 31)) return false;
    if (N * H * W >= ((int64_t)1 << 31)) return false;
    a.N = (int)N; a.H = (int)H; a.W = (int)W; a.Cw = Cw; a.Cn = Cn; a.ks = ksize;
    a.nrow = ksize * ksize * Cn;
    a.ld = a.nrow | 1;
    const int halo = 2 * (ksize / 2);
    const int64_t row_bytes = W * a.ld * (int64_t)sizeof(float);
    const int64_t fit = ((int64_t)kNarrowOutLds - (int64_t)Cw * 32 * (int64_t)sizeof(float)) / row_bytes - halo;   // output rows that fit
    if (fit < 1) return false;
    int64_t bands = (H + fit - 1) / fit;
    // a small batch: more, thinner bands (down to four rows behind a halo) until every CU has two workgroups
    const int64_t thin = ksize == 1 ? H : (H + 3) / 4;
    int64_t want = (512 + N - 1) / N;
    if (want > thin) want = thin;
    if (bands < want) bands = want;
    a.R = (int)((H + bands - 1) / bands);
    a.bands = (int)((H + a.R - 1) / a.R);
    if (N * a.bands >= ((int64_t)1 << 28)) return false;
    a.nwg = (int)(N * a.bands);
    a.per_xcd = (a.nwg + 7) / 8;
    magic_u31((unsigned)W, &a.magW, &a.shW);
    return true;
}

int wc_conv_narrow_out_supported(int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize)
{
    NarrowOutArgs a = {};
    return narrow_out_plan(a, N, H, W, Cw, Cn, ksize) ? 1 : 0;
}

int wc_conv_narrow_out_f32(const float* g, const float* mask, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r,
                           int64_t stride_s, int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize, float* out, wc_stream_t stream)
{
    if (!g || !w || !out) return WC_ERR_NULL;
    NarrowOutArgs a = {};
    if (!narrow_out_plan(a, N, H, W, Cw, Cn, ksize)) return WC_ERR_SHAPE;
    if (((uintptr_t)g | (uintptr_t)mask) & 15) return WC_ERR_ARG;              // 16-byte loads of the wide rows
    a.g = g; a.mask = mask; a.w = w; a.out = out;
    a.sk = stride_k; a.sn = stride_n; a.sr = stride_r; a.ss = stride_s;
    hipStream_t st = (hipStream_t)stream;
    const int rows = a.R + 2 * (ksize / 2);
    const size_t lds = ((size_t)Cw * 32 + (size_t)rows * a.W * a.ld) * sizeof(float);
    const void* kernel = mask ? reinterpret_cast<const void*>(conv_narrow_out_kernel<true>)
                              : reinterpret_cast<const void*>(conv_narrow_out_kernel<false>);
    hipError_t e = wc_set_max_lds(kernel, lds);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)(8 * a.per_xcd));
    if (mask) hipLaunchKernelGGL(conv_narrow_out_kernel<true>, grid, dim3(kNarrowOutThreads), lds, st, a);
    else hipLaunchKernelGGL(conv_narrow_out_kernel<false>, grid, dim3(kNarrowOutThreads), lds, st, a);
    return (int)hipGetLastError();
}

// wc_conv_narrow_out_f32 with bias[c] added to each output behind its tap sum; bias == nullptr: that entry itself
int wc_conv_narrow_out_bias_f32(const float* g, const float* mask, const float* w, int64_t stride_k, int64_t stride_n, int64_t stride_r,
                                int64_t stride_s, const float* bias, int64_t N, int64_t H, int64_t W, int Cw, int Cn, int ksize, float* out,
                                wc_stream_t stream)
{
    if (!bias) return wc_conv_narrow_out_f32(g, mask, w, stride_k, stride_n, stride_r, stride_s, N, H, W, Cw, Cn, ksize, out, stream);
    if (!g || !w || !out) return WC_ERR_NULL;
    NarrowOutArgs a = {};
    if (!narrow_out_plan(a, N, H, W, Cw, Cn, ksize)) return WC_ERR_SHAPE;
    if (((uintptr_t)g | (uintptr_t)mask) & 15) return WC_ERR_ARG;
    a.g = g; a.mask = mask; a.w = w; a.out = out; a.bias = bias;
    a.sk = stride_k; a.sn = stride_n; a.sr = stride_r; a.ss = stride_s;
    hipStream_t st = (hipStream_t)stream;
    const int rows = a.R + 2 * (ksize / 2);
    const size_t lds = ((size_t)Cw * 32 + (size_t)rows * a.W * a.ld) * sizeof(float);
    const void* kernel = mask ? reinterpret_cast<const void*>(conv_narrow_out_kernel<true, true>)
                              : reinterpret_cast<const void*>(conv_narrow_out_kernel<false, true>);
    hipError_t e = wc_set_max_lds(kernel, lds);
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)(8 * a.per_xcd));
    if (mask) hipLaunchKernelGGL((conv_narrow_out_kernel<true, true>), grid, dim3(kNarrowOutThreads), lds, st, a);
    else hipLaunchKernelGGL((conv_narrow_out_kernel<false, true>), grid, dim3(kNarrowOutThreads), lds, st, a);
    return (int)hipGetLastError();
}

size_t wc_conv_wrw_workspace_bytes(const wc_conv_geom* g)
{
    if (!g || g->Cin < 32 || g->Cout < 32) return 0;
    int tile;
    return (size_t)wrw_splits(g, &tile) * g->nphase * g->ntaps * g->Cin * g->Cout * 4;
}

int wc_conv_wrw_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* ghi, const void* glo, const float* gscale,
                      const void* zero_line, const wc_conv_geom* g, float* dw, int64_t stride_k, int64_t stride_n,
                      int64_t stride_r, int64_t stride_s, void* ws, size_t ws_bytes, wc_stream_t stream)
{
    return wc_conv_wrw_bias_f16x3(xhi, xlo, xscale, ghi, glo, gscale, zero_line, g, dw, stride_k, stride_n, stride_r, stride_s,
                                  nullptr, nullptr, ws, ws_bytes, stream);
}

// argument checks and both kernels' argument blocks of wc_conv_wrw_bias_f16x3 (shared with wc_conv_bwd_pair_f16x3)
struct WrwPlan { WrwArgs a; WrwReduceArgs r; int T, splits, tiles, extra; };

static int wrw_prepare(WrwPlan& p, const void* xhi, const void* xlo, const float* xscale, const void* ghi, const void* glo, const float* gscale,
                       const void* zero_line, const wc_conv_geom* g, float* dw, int64_t stride_k, int64_t stride_n,
                       int64_t stride_r, int64_t stride_s, const float* colsum_partials, float* db, void* ws, size_t ws_bytes)
{
    if (!xhi || !xlo || !xscale || !ghi || !glo || !gscale || !zero_line || !g || !dw || !ws) return WC_ERR_NULL;
    // (the set it always took, or the slim set: any side a multiple of 32 on whole tiles)
    if (!((wc_conv_ragged_supported(g) && !(g->Cin & 63)) || wc_conv_slim_supported(g)) || g->W < 2 || g->H * g->W < 2) return WC_ERR_SHAPE;
    if (ws_bytes < wc_conv_wrw_workspace_bytes(g)) return WC_ERR_WORKSPACE;
    if ((colsum_partials == nullptr) != (db == nullptr)) return WC_ERR_NULL;
    if (db && ((g->Cout & 3) || 256 % (g->Cout >> 2) != 0)) return WC_ERR_SHAPE;
    WrwArgs& a = p.a;
    WrwReduceArgs& r = p.r;
    int T;
    int splits = wrw_splits(g, &T);
    const int64_t M = (int64_t)g->N * g->H * g->W;
    const int nslice = g->nphase * g->ntaps;
    const int tiles = nslice * (g->Cin / T) * (g->Cout / T);
    const int nchunks = (int)(M / 32);
    WrwOperand X, G;
    X.hi = (const _Float16*)xhi; X.lo = (const _Float16*)xlo; X.Hp = g->Hin; X.Wp = g->Win; X.C = g->Cin; X.stride = g->in_stride;
    G.hi = (const _Float16*)ghi; G.lo = (const _Float16*)glo; G.Hp = g->Hout; G.Wp = g->Wout; G.C = g->Cout; G.stride = g->out_stride;
    r.nout = 0; r.coef = g->wcoef;
    for (int ph = 0; ph < kMaxPhase; ++ph)
        for (int t = 0; t < kMaxTaps; ++t) {
            X.dy[ph][t] = g->dy[ph][t]; X.dx[ph][t] = g->dx[ph][t];
            G.dy[ph][t] = g->off_y[ph]; G.dx[ph][t] = g->off_x[ph];
            if (ph >= g->nphase || t >= g->ntaps) continue;
            if (g->nsrc[ph][t] < 1 || g->nsrc[ph][t] > 4) return WC_ERR_ARG;
            for (int m = 0; m < g->nsrc[ph][t]; ++m) {          // source tap -> the slices built from it
                int o = 0;
                while (o < r.nout && (r.r[o] != g->wr[ph][t][m] || r.s[o] != g->ws[ph][t][m])) ++o;
                if (o == r.nout) {
                    if (r.nout == kMaxTaps) return WC_ERR_ARG;
                    r.r[o] = g->wr[ph][t][m]; r.s[o] = g->ws[ph][t][m]; r.cnt[o] = 0; ++r.nout;
                }
                if (r.cnt[o] == 4) return WC_ERR_ARG;
                r.slice[o][r.cnt[o]++] = (signed char)(ph * g->ntaps + t);
            }
        }
    // the lanes of a result tile run along its columns: put the weight's contiguous channel axis there
    const bool x_cols = stride_k == 1;
    a.A = x_cols ? G : X; a.B = x_cols ? X : G;
    a.zero = (const _Float16*)zero_line; a.partial = (float*)ws;
    a.N = g->N; a.H = g->H; a.W = g->W; a.ntaps = g->ntaps; a.nphase = g->nphase;
    magic_u31((unsigned)(g->H * g->W), &a.magHW, &a.shHW);
    magic_u31((unsigned)g->W, &a.magW, &a.shW);
    a.nchunks = nchunks; a.cps = (nchunks + splits - 1) / splits;
    splits = (nchunks + a.cps - 1) / a.cps;         // no empty ranges
    r.partial = (const float*)ws; r.splits = splits; r.nslice = nslice; r.Ca = a.A.C; r.Cb = a.B.C;
    r.xscale = xscale; r.gscale = gscale; r.dw = dw;
    r.sa = x_cols ? stride_n : stride_k; r.sb = x_cols ? stride_k : stride_n; r.sr = stride_r; r.ss = stride_s;
    r.colsum = colsum_partials; r.db = db; r.c4n = db ? g->Cout >> 2 : 0;
    r.main_blocks = grid_for((int64_t)r.nout * g->Cin * g->Cout);
    p.T = T; p.splits = splits; p.tiles = tiles; p.extra = db ? (r.c4n * 64 + 255) / 256 : 0;
    return WC_OK;
}

int wc_conv_wrw_bias_f16x3(const void* xhi, const void* xlo, const float* xscale, const void* ghi, const void* glo, const float* gscale,
                           const void* zero_line, const wc_conv_geom* g, float* dw, int64_t stride_k, int64_t stride_n,
                           int64_t stride_r, int64_t stride_s, const float* colsum_partials, float* db,
                           void* ws, size_t ws_bytes, wc_stream_t stream)
{
    hipStream_t st = (hipStream_t)stream;
    WrwPlan p;
    const int rc = wrw_prepare(p, xhi, xlo, xscale, ghi, glo, gscale, zero_line, g, dw, stride_k, stride_n, stride_r, stride_s,
                               colsum_partials, db, ws, ws_bytes);
    if (rc != WC_OK) return rc;
    const WrwArgs& a = p.a;
    const WrwReduceArgs& r = p.r;
    const int T = p.T;
    dim3 grid((unsigned)p.splits, (unsigned)p.tiles);
    hipError_t e = hipSuccess;
    if (T == 32) {
        constexpr int LDS = 4 * 2 * 8 * 1024;       // four waves, two stages of 8 KiB each
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_wrw_slim_kernel), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(conv_wrw_slim_kernel, dim3((unsigned)((p.splits + 3) / 4), (unsigned)p.tiles), dim3(256), LDS, st, a, p.splits);
    } else if (T == 256) {
        constexpr int LDS = 2 * (2 * 4 * 4 * 1024 + 2 * 4 * 4 * 1024);
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_wrw_kernel<4, 4>), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((conv_wrw_kernel<4, 4>), grid, dim3(256), LDS, st, a);
    } else if (T == 64) {
        constexpr int LDS = 2 * (2 * 1 * 4 * 1024 + 2 * 1 * 4 * 1024);
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_wrw_kernel<1, 1>), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((conv_wrw_kernel<1, 1>), grid, dim3(256), LDS, st, a);
    } else {
        constexpr int LDS = 2 * (2 * 2 * 4 * 1024 + 2 * 2 * 4 * 1024);
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_wrw_kernel<2, 2>), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((conv_wrw_kernel<2, 2>), grid, dim3(256), LDS, st, a);
    }
    hipLaunchKernelGGL(conv_wrw_reduce_kernel, dim3(r.main_blocks + p.extra), dim3(256), 0, st, r);
    return (int)hipGetLastError();
}

// ---- data gradient + weight gradient of one layer in two launches (conv_bwd_pair_kernel, conv_pair_reduce_kernel) -------------------------
// gd = the data-gradient geometry (what wc_conv_f16x3 is given for dx), gf = the forward geometry (what wc_conv_wrw_bias_f16x3 is given).
int wc_conv_bwd_pair_supported(const wc_conv_geom* gd, const wc_conv_geom* gf)
{
    if (!gd || !gf || !wc_conv_ragged_supported(gd) || !wc_conv_ragged_supported(gf) || (gf->Cin & 63) || gf->H * gf->W < 2) return 0;
    // one layer: the data gradient reads the planes the weight gradient takes as gy, and writes an x-shaped tensor
    if (gd->N != gf->N || gd->Cin != gf->Cout || gd->Cout != gf->Cin) return 0;
    if (gd->Hin != gf->Hout || gd->Win != gf->Wout || gd->Hout != gf->Hin || gd->Wout != gf->Win) return 0;
    // the critic's kinds -- 'same', 'down', 'down3': a dense forward whose data gradient reads gy at stride 1 (the up-sampling layers of
    // the generator, a phase forward with a strided data gradient, stay on the four launches: not costed)
    if (gf->nphase != 1 || gd->in_stride != 1) return 0;
    // the data gradient on <2, 2, KS>: 128-wide output tiles, not the 256-point tile
    if ((gd->Cout % 128) != 0 || (gd->Cout % 256) == 0 || conv_big_tile(gd, conv_ksplit(gd))) return 0;
    int tile;
    (void)wrw_splits(gf, &tile);
    return tile == 128 ? 1 : 0;
}

size_t wc_conv_bwd_pair_workspace_bytes(const wc_conv_geom* gd, const wc_conv_geom* gf)
{
    if (!gd || !gf) return 0;
    return wc_conv_workspace_bytes(gd) + wc_conv_wrw_workspace_bytes(gf);
}

// tail == nullptr: wc_conv_bwd_pair_f16x3; else the data gradient's finish goes on to the tail's work (MASKED or DX; dx unused by DX)
static int bwd_pair(const void* ghi, const void* glo, const float* gscale, const void* wimage, const float* wscale,
                    const void* zero_line, const wc_conv_geom* gd, float* dx, void* ws_dx, size_t ws_dx_bytes,
                    const void* xhi, const void* xlo, const float* xscale, const wc_conv_geom* gf, float* dw,
                    int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                    const float* colsum_partials, float* db, void* ws_dw, size_t ws_dw_bytes, const wc_conv_tail* tail, hipStream_t st)
{
    ConvArgs d;
    if (tail && tail->kind == WC_CONV_TAIL_DX && !tail->out) return WC_ERR_NULL;
    float* dx_or_out = (tail && tail->kind == WC_CONV_TAIL_DX) ? tail->out : dx;
    int rc = conv_prepare(d, ghi, glo, gscale, wimage, wscale, nullptr, zero_line, gd, 0, dx_or_out, ws_dx, ws_dx_bytes);
    if (rc != WC_OK) return rc;
    FinishTailArgs f;
    if (tail) {
        if (tail->kind != WC_CONV_TAIL_MASKED && tail->kind != WC_CONV_TAIL_DX) return WC_ERR_ARG;
        rc = tail_prepare(f, tail, d, gd, gscale, wscale, nullptr, dx, ws_dx);
        if (rc != WC_OK) return rc;
    }
    WrwPlan p;
    rc = wrw_prepare(p, xhi, xlo, xscale, ghi, glo, gscale, zero_line, gf, dw, stride_k, stride_n, stride_r, stride_s,
                     colsum_partials, db, ws_dw, ws_dw_bytes);
    if (rc != WC_OK) return rc;
    if (!wc_conv_bwd_pair_supported(gd, gf) || p.T != 128) return WC_ERR_SHAPE;
    constexpr int LDS = 2 * (2 * 2 * 4 * 1024 + 2 * 2 * 4 * 1024);
    const int64_t M = (int64_t)gd->N * gd->H * gd->W;
    const int gx = (int)conv_tiles(M), gy = gd->nphase * (gd->Cout / 128);          // launch_conv<2, 2>'s grid
    const int64_t conv_blocks = (int64_t)gx * gy * d.ksplit, wrw_off = (conv_blocks + 7) & ~(int64_t)7;
    const int64_t blocks = wrw_off + (int64_t)p.splits * p.tiles;
    if (blocks > 0x7fffffff) return WC_ERR_SHAPE;
    hipError_t e;
    if (M % 128) {          // a partial last tile in the data gradient's grid
        if (d.ksplit > 1) {
            e = wc_set_max_lds(reinterpret_cast<const void*>(conv_bwd_pair_ragged_kernel<true>), LDS);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL((conv_bwd_pair_ragged_kernel<true>), dim3((unsigned)blocks), dim3(256), LDS, st, d, p.a,
                               (int)conv_blocks, (int)wrw_off, p.splits, gx, gy);
        } else {
            e = wc_set_max_lds(reinterpret_cast<const void*>(conv_bwd_pair_ragged_kernel<false>), LDS);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL((conv_bwd_pair_ragged_kernel<false>), dim3((unsigned)blocks), dim3(256), LDS, st, d, p.a,
                               (int)conv_blocks, (int)wrw_off, p.splits, gx, gy);
        }
    } else if (d.ksplit > 1) {
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_bwd_pair_kernel<true>), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((conv_bwd_pair_kernel<true>), dim3((unsigned)blocks), dim3(256), LDS, st, d, p.a,
                           (int)conv_blocks, (int)wrw_off, p.splits, gx, gy);
    } else {
        e = wc_set_max_lds(reinterpret_cast<const void*>(conv_bwd_pair_kernel<false>), LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((conv_bwd_pair_kernel<false>), dim3((unsigned)blocks), dim3(256), LDS, st, d, p.a,
                           (int)conv_blocks, (int)wrw_off, p.splits, gx, gy);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int reduce_blocks = p.r.main_blocks + p.extra;
    if (tail) {                                     // (tail_prepare took the geometry: d.ksplit > 1)
        if (tail->kind == WC_CONV_TAIL_MASKED)
            hipLaunchKernelGGL((conv_pair_reduce_tail_kernel<kTailMasked>), dim3(reduce_blocks + kAmaxBlocks), dim3(256), 0, st, p.r, f, reduce_blocks);
        else
            hipLaunchKernelGGL((conv_pair_reduce_tail_kernel<kTailDx>), dim3(reduce_blocks + grid_for(f.k.n4)), dim3(256), 0, st, p.r, f, reduce_blocks);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        return tail_redo(tail, f, st);
    }
    if (d.ksplit > 1) {
        KsplitReduceArgs k;
        k.n4 = (int64_t)gd->N * gd->Hout * gd->Wout * gd->Cout / 4;
        k.partial = (const float*)ws_dx; k.ksplit = d.ksplit; k.cout = gd->Cout;
        k.xscale = gscale; k.wscale = wscale; k.bias = nullptr; k.relu = 0; k.y = dx;
        hipLaunchKernelGGL(conv_pair_reduce_kernel, dim3(reduce_blocks + grid_for(k.n4)), dim3(256), 0, st, p.r, k, reduce_blocks);
    } else {
        hipLaunchKernelGGL(conv_wrw_reduce_kernel, dim3(reduce_blocks), dim3(256), 0, st, p.r);
    }
    return (int)hipGetLastError();
}

int wc_conv_bwd_pair_f16x3(const void* ghi, const void* glo, const float* gscale, const void* wimage, const float* wscale,
                           const void* zero_line, const wc_conv_geom* gd, float* dx, void* ws_dx, size_t ws_dx_bytes,
                           const void* xhi, const void* xlo, const float* xscale, const wc_conv_geom* gf, float* dw,
                           int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                           const float* colsum_partials, float* db, void* ws_dw, size_t ws_dw_bytes, wc_stream_t stream)
{
    return bwd_pair(ghi, glo, gscale, wimage, wscale, zero_line, gd, dx, ws_dx, ws_dx_bytes, xhi, xlo, xscale, gf, dw,
                    stride_k, stride_n, stride_r, stride_s, colsum_partials, db, ws_dw, ws_dw_bytes, nullptr, (hipStream_t)stream);
}

int wc_conv_bwd_pair_tail_f16x3(const void* ghi, const void* glo, const float* gscale, const void* wimage, const float* wscale,
                                const void* zero_line, const wc_conv_geom* gd, float* dx, void* ws_dx, size_t ws_dx_bytes,
                                const void* xhi, const void* xlo, const float* xscale, const wc_conv_geom* gf, float* dw,
                                int64_t stride_k, int64_t stride_n, int64_t stride_r, int64_t stride_s,
                                const float* colsum_partials, float* db, void* ws_dw, size_t ws_dw_bytes,
                                const wc_conv_tail* tail, wc_stream_t stream)
{
    if (!tail) return WC_ERR_NULL;
    return bwd_pair(ghi, glo, gscale, wimage, wscale, zero_line, gd, dx, ws_dx, ws_dx_bytes, xhi, xlo, xscale, gf, dw,
                    stride_k, stride_n, stride_r, stride_s, colsum_partials, db, ws_dw, ws_dw_bytes, tail, (hipStream_t)stream);
}

}  // extern "C"
