"""Autograd function for the fused whitening + coloring transform.

Forward  (SURVEY.md rows a2/a3/a6-a9):  y_n = (x_n - mu) A_{slot(n)} + beta_{slot(n)},  A_k = W^T Gamma_k
Backward (row a10): one reduction (K4), the small float64 stage (K5), one two-stream apply (K6).

`process_group` turns on sync-WC: the additive moments (K1 output) and the backward reductions
(K4 output) are all-reduced over RCCL, so every replica whitens with the global-batch statistics.
Default (None) keeps per-replica statistics, which is the reference's behaviour on each GPU.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _state, ops

# Test hook (tests/test_producer_gpu.py): {'record': []} collects the one-bit ReLU masks the sites of a pass produce, {'replay': [...]} makes
# the sites of the next pass SAVE those instead of their own -- two routes whose K3 outputs differ in the last bit then run their backward
# on identical masks, and their gradients can be compared at rounding level instead of at the level of a few flipped ReLUs.
# The batch-norm sites use the same hook (generator._norm_relu): the fused route records `y > 0`, torch's route replays it as its ReLU
# (tests/test_std_gpu.py).
MASK_TAP = None


def _tap_mask(mask):
    if 'record' in MASK_TAP:
        MASK_TAP['record'].append(mask.clone())
        return mask
    return MASK_TAP['replay'].pop(0)


def _allreduce_(tensors, group):
    """Sum over the replicas, in place.  (General form: pack, reduce, unpack.  The WC path itself hands over tensors that are
    already views of one buffer -- ops.stats / ops.bwd_reduce with flat=True -- and all-reduces that buffer directly.)"""
    flat = torch.cat([t.reshape(-1) for t in tensors])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    off = 0
    for t in tensors:
        n = t.numel()
        t.copy_(flat[off:off + n].view_as(t))
        off += n


def _whiten(x, st, training, eps, momentum, ddof, moving_mean, moving_cov, group=None, groups=1, decomposition='cholesky'):
    """K1 + K2 of a site -> (mu, L, W, chan_scale), the statistics of the contiguous fp32 x (N, ..., C) or, where the residual add in
    front wrote pre-split planes, of the SplitTensor st (x is then its handle; the planes' own scales are the apply's input scales).
    Updates the moving statistics in place when training.  decomposition='zca': the eigen-stage (ops.zca) follows K2 on every route --
    W is then the symmetric U diag(lam^-1/2) U^T and the pair (U, lam) stands where L does."""
    C = x.shape[-1]
    M = x.numel() // C
    mm = moving_mean.view(-1) if moving_mean is not None else None
    pre = training and st is not None and st.moments is not None and st.moments[1] == groups   # the producer accumulated K1's partials
    if training and group is None and st is None:
        # per-replica statistics (the reference's behaviour): K1 and K2 as one call -- the moments never leave the workspace and the
        # K1 tail / K2 head run as one launch (wc_whiten_f32)
        out = ops.whiten(x.view(M, C), eps, momentum, ddof, mm, moving_cov, groups)
    elif training and group is None:
        out = (ops.whiten_presummed if pre else ops.whiten_split)(st, eps, momentum, ddof, mm, moving_cov, groups)
    else:
        s = xtx = None
        if training:
            # sync-WC: the additive moments of all replicas, ONE collective on the buffer K1 wrote them into (no pack / unpack
            # launches); every replica holds the same number of rows (fixed per-GPU batch): no host sync for the count
            s, xtx, buf = (ops.stats(x.view(M, C), flat=True) if st is None else
                           (ops.stats_presummed if pre else ops.stats_split)(st, flat=True))
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
            M *= dist.get_world_size(group)
        out = ops.factor(s, xtx, M, C, eps, momentum, ddof, training, mm, moving_cov, x.device, want_scale=st is None)
    if training:
        _touched(moving_mean, moving_cov)
    if decomposition == 'zca':
        U, lam, W = ops.zca(out[1], eps, groups)
        out = (out[0], (U, lam), W) + tuple(out[3:])
    return out if st is None else out + (st.scale,)


def _k3(x, st, mu, A, bias, slot, plan, folded, relu, want_mask, handoff=None):
    """K3 of a site -> (y, mask | None), from the fp32 x or from the SplitTensor st (x is then its handle; folded: `bias` is already
    beta + (center - mu) A, one launch).  want_mask: also the ReLU's one-bit gradient mask.  handoff: None, or the (gamma, beta) of the
    coloring when the output leaves as the next convolution's fp16 planes -- their scale record is built from those (not from the
    effective bias K3 adds), and y is then the NaN handle that carries the planes (`_wc_planes`: what conv.fast_conv_or_none looks for)."""
    rec = None if handoff is None else ops.out_scale(handoff[0], handoff[1], x.shape[-1], x.device)
    if st is not None:
        out = ops.apply_split(st, mu, A, bias, slot, plan=plan, relu=relu, folded=folded, want_mask=want_mask, oscale=rec)
    elif rec is not None:
        out = ops.apply_planes(x, mu, A, bias, slot, plan, rec, relu=relu, want_mask=want_mask)
    else:
        out = ops.apply(x, mu, A, bias, slot, plan=plan, relu=relu, want_mask=want_mask)
    if rec is None:
        return out if want_mask else (out, None)
    y = _nan_handle(x.shape, x.device)
    y._wc_planes = (out[0][0], out[0][1], rec)          # (hi, lo, scale record)
    return y, (out[2] if want_mask else None)


def backward_reads_planes(shape, has_slot):
    """Do K4 and K6 of a site whose input arrives as pre-split planes read x from those planes too (wc_bwd_*_xsplit_f32: the C = 256 and
    128 fast paths)?  Elsewhere they read the fp32 sum the producer then writes beside the planes.  (The fast paths need N*HW % 32 == 0:
    a ReLU'd site on them always keeps its mask as bits.)"""
    return ops.bwd_xsplit_supported(tuple(shape), has_slot)


def _bwd_reduce(x, xs, mu, gy, y, slot, Kc, relu, bits, share, flat):
    """K4 -> (R, gsum, flat buffer | None, scales | None, the gy K6 reads, K6's bit mask | None).  y: what the forward saved for a ReLU'd
    site, its one-bit mask (bits) or y itself; K4 applies the mask while it stages gy and hands the masked gradient on (no pass of its
    own).  share: the statistics path runs -- K4 samples the fp16 scales of (x - mu) and gy and K6 reuses them (three launches instead of
    six).  flat: R and gsum as views of one buffer (sync-WC's single all-reduce)."""
    rm = y if relu and bits else None
    if xs is not None:          # x lives in the producer's planes
        if rm is not None and gy.shape[-1] != 256:      # the planes forms of K4 / K6 apply the bits themselves at C = 256 only: one masking pass in front
            gy, rm = ops.relu_mask_bits(gy, rm), None
        out = ops.bwd_reduce_xsplit(xs, mu, gy, slot, Kc, relu_mask=rm, flat=flat)
        return out[0], out[1], out[2] if flat else None, out[-1], gy, rm
    # with the bits and a K6 that masks for itself (C = 256 fast paths) K4 writes no masked copy of the gradient at all
    bits_only = rm is not None and share and ops.bwd_bits_supported(x.shape, slot is not None)
    out = ops.bwd_reduce(x, mu, gy, slot, Kc, flat=flat, want_scales=share, relu_y=y if relu and not bits else None, relu_mask=rm,
                         write_masked=not bits_only)
    if relu and not bits_only:
        gy = out[-2] if share else out[-1]
    return out[0], out[1], out[2] if flat else None, out[-1] if share else None, gy, rm if bits_only else None


class WhitenColorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, slot, moving_mean, moving_cov, training, eps, momentum, ddof, process_group, relu=False,
                handoff=False, st=None, decomposition='cholesky', renorm=False):
        # x: (N, ..., C) float32 contiguous (NHWC); gamma (Kc,C,C)|None; beta (Kc,C)|None; slot int32 (N,)|None
        # handoff: the output leaves as the next convolution's fp16 planes (the K3 -> convolution hand-off below): y is a handle carrying them
        # st: x is a HANDLE whose data is this ops.SplitTensor (the residual add wrote the pre-split planes, split_handle below):
        #     K1 and K3 run on the planes (wc_whiten_split_f16x2, wc_apply_split_ex_f16x2), no conversion, no fp32 read
        C = x.shape[-1]
        M_local = x.numel() // C
        dev = x.device
        if st is None:
            x = x.contiguous()
        # decomposition='zca': `L` below is the eigen-stage's (U, lam); everything behind W is the Cholesky site's
        zca = decomposition == 'zca'
        # renorm (norm 'dr', training mode): the moving factor W_m first -- K2 below updates moving_cov in place and the renormalised
        # whitening is defined on the statistics from before the update
        renorm = bool(renorm) and bool(training)
        Wm = ops.renorm(moving_cov, None, eps)[0] if renorm else None
        mu, L, W, chan_scale = _whiten(x, st, training, eps, momentum, ddof, moving_mean, moving_cov, process_group, 1, decomposition)
        lam_t = ()
        if zca:
            L, lam_t = L[0], (L[1],)
        Wc = W                  # the matrix the coloring folds in
        if renorm:
            # W_eff = W_m sg(L) W: the value is W_m's, so the coloring takes W_m; C0 = W_m L stands where L does (K5 reads it, with W
            # and W_m).  Under sync-WC L is the factor of the all-reduced moments: every rank whitens with the same W_m (x - mu)
            L = ops.renorm(None, L, eps, Wm)[1]
            Wc, lam_t = Wm, (Wm,)
        g = gamma.contiguous() if gamma is not None else None
        b = beta.contiguous() if beta is not None else None
        bias = b
        if st is not None:      # ... and, on planes, the additive term beta + (center - mu) A from the same launch as the tables
            A, At, plan, bias = ops.color_split(Wc, g, st, mu, b)
        else:
            A, At, plan = ops.color(Wc, g, chan_scale)      # plan: the apply's fp16 tables, so K3 is one launch
        # relu: folded into K3's epilogue (row N2).  Its gradient mask is kept as ONE BIT per element (K3 writes it): the
        # backward neither re-reads y (K4: 134 MB at the headline site) nor keeps y alive for it
        bits = bool(relu) and M_local % 32 == 0
        y, mask = _k3(x, st, mu, A, bias, slot, plan, True, relu, bits, (g, b) if handoff else None)
        ctx.xsplit = None
        xs_t = ()
        if st is not None:
            # the backward: K4 / K6 read x from the same planes where they can; elsewhere from the fp32 sum the producer wrote beside
            # the planes (st.x32), or -- no such copy -- from one made here
            if not any(ctx.needs_input_grad[:3]):
                x = torch.empty(0, device=dev)
            elif backward_reads_planes(x.shape, slot is not None):
                ctx.xsplit = st.shape
                xs_t = (st.planes, st.center, st.scale)
                x = torch.empty(0, device=dev)
            else:
                x = st.x32 if st.x32 is not None else ops.unsplit(st)
        if MASK_TAP is not None and bits:
            mask = _tap_mask(mask)
        ctx.save_for_backward(x, mu, L, W, A, At, g if g is not None else torch.empty(0, device=dev),
                              slot if slot is not None else torch.empty(0, dtype=torch.int32, device=dev),
                              mask if bits else (y if relu else torch.empty(0, device=dev)), *xs_t, *lam_t)
        # (saved_tensors: the nine above, the planes' three where K4 / K6 read them, then ZCA's lam or renorm's W_m)
        ctx.zca, ctx.renorm, ctx.lam_at = zca, renorm, 9 + len(xs_t)
        ctx.relu = bool(relu)
        ctx.mask_bits = bits
        ctx.has_gamma = g is not None
        ctx.has_beta = b is not None
        ctx.has_slot = slot is not None
        ctx.training = bool(training)
        # the row count K2 used: every replica's under sync-WC
        ctx.M = M_local * dist.get_world_size(process_group) if (training and process_group is not None) else M_local
        ctx.eps, ctx.ddof, ctx.group = eps, ddof, process_group
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mu, L, W, A, At, g, slot, y = ctx.saved_tensors[:9]
        xs = None if ctx.xsplit is None else ops.SplitTensor(*ctx.saved_tensors[9:12], None, ctx.xsplit)     # x lives in the planes
        g = g if ctx.has_gamma else None
        slot = slot if ctx.has_slot else None
        gy = gy.contiguous()
        if ctx.zca:         # K5 of a ZCA site takes (U, lam) where the Cholesky site's takes L
            U, lam = L, ctx.saved_tensors[ctx.lam_at]

            def k5(R, gsum, W, L, *rest, **kw):
                return ops.bwd_factor_zca(R, gsum, W, U, lam, *rest, **kw)
        elif ctx.renorm:    # ... and a renorm site's takes W_m and C0 = W_m L (saved in L's place)
            Wm = ctx.saved_tensors[ctx.lam_at]

            def k5(R, gsum, W, C0, *rest, **kw):
                return ops.bwd_factor_renorm(R, gsum, W, Wm, C0, *rest, **kw)
        else:
            k5 = ops.bwd_factor
        need_x, need_g, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dgamma = dbeta = dx = S = gmean = scales = k6_mask = None
        stats_path = ctx.training and need_x
        want_g = ctx.has_gamma and need_g
        want_b = ctx.has_beta and need_b
        if want_g or want_b or stats_path:
            R, gsum, rbuf, scales, gy, k6_mask = _bwd_reduce(x, xs, mu, gy, y, slot, A.shape[0], ctx.relu, ctx.mask_bits, stats_path,
                                                             ctx.group is not None)
            if ctx.group is None:
                dgamma, dbeta, S, gmean = k5(R, gsum, W, L, g, A, ctx.M, ctx.eps, ctx.ddof, stats_path,
                                             want_dgamma=want_g, want_dbeta=want_b)
            else:
                # parameter gradients stay per-replica (the DDP-style average happens outside);
                # the statistics path needs the global reductions under sync-WC
                if want_g or want_b:
                    dgamma, dbeta, _, _ = k5(R, gsum, W, L, g, A, ctx.M, ctx.eps, ctx.ddof, False,
                                             want_dgamma=want_g, want_dbeta=want_b)
                if stats_path:
                    dist.all_reduce(rbuf, op=dist.ReduceOp.SUM, group=ctx.group)
                    _, _, S, gmean = k5(R, gsum, W, L, g, A, ctx.M, ctx.eps, ctx.ddof, True,
                                        want_dgamma=False, want_dbeta=False)
        elif ctx.relu:          # the fused activation's gradient: the mask in front of the unchanged backward
            if ctx.mask_bits:
                gy = ops.relu_mask_bits(gy, y)
            else:
                gy = torch.ops.aten.threshold_backward(gy, y, 0.0)      # gy where y > 0, else 0: ONE elementwise pass (where(y > 0, ...) took three launches)
        if need_x:
            if xs is not None and S is not None:
                dx = ops.bwd_apply_xsplit(gy, xs, mu, At, S, gmean, slot, scales, relu_mask=k6_mask)
            else:
                if xs is not None:          # (evaluation-mode site with a gradient: no statistics path, dx = masked gy At)
                    x = mu = scales = None
                    if k6_mask is not None:
                        gy, k6_mask = ops.relu_mask_bits(gy, k6_mask), None
                dx = ops.bwd_apply(gy, x, mu, At, S, gmean, slot, scales=scales, relu_mask=k6_mask)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------
# K3 -> convolution hand-off: the site's output as the next convolution's operand
# ---------------------------------------------------------------------------------------------
_NAN = {}


def _nan_handle(shape, dev):
    """The tensor that stands for y in the autograd graph when y itself leaves as fp16 planes: the right shape and dtype, no
    memory (one NaN element, stride 0) -- anything that reads it as data fails loudly instead of computing on zeros."""
    t = _NAN.get(str(dev))
    if t is None:
        t = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
        if not (t.is_cuda and torch.cuda.is_current_stream_capturing()):
            _NAN[str(dev)] = t
    return t.expand(tuple(shape))


def conv_handoff_supported(shape, relu, Ktables=1):
    """May a site of this NHWC output shape hand its output to the next convolution as planes? (relu'd sites only: that is what
    every convolution behind a WC site reads, generator.py:144-151)"""
    return bool(relu) and Ktables <= 1024 and ops.apply_planes_supported(tuple(shape))


def split_of(x):
    """The ops.SplitTensor a handle carries (the residual add of the block in front wrote the tensor as pre-split planes), or None."""
    return getattr(x, '_wc_split', None)


def materialize(x):
    """The fp32 tensor behind a handle (no autograd): a block output that travels as pre-split planes (`_wc_split`: ops.unsplit) or a site
    output that travels as the next convolution's planes (`_wc_planes`: (hi + lo) / scale); any other tensor is returned as it is.  For
    readers outside the generator's own wiring -- hooks, feature extraction, debugging -- which would otherwise compute on the handle's NaN."""
    st = getattr(x, '_wc_split', None)
    if st is not None:
        return ops.unsplit(st)
    pl = getattr(x, '_wc_planes', None)
    if pl is not None:
        hi, lo, rec = pl
        return ((hi.float() + lo.float()) / rec[0]).view(x.shape)
    return x


def split_handle(st, shape, dev):
    """A tensor that stands for a pre-split activation wherever a tensor object is needed (shape, device, autograd edge): the NaN
    handle of the K3 -> convolution hand-off, with the data attached as `_wc_split`."""
    h = _nan_handle(shape, dev)
    h._wc_split = st
    return h


class ResidualAddFunction(torch.autograd.Function):
    """out = h + upsample2x(s) (up) or h + s: the Add that ends a `resblock` (generator.py:142-146), csrc/wc_resadd.hip.
    box is None: the fp32 sum.  box a list: the sum leaves in the pre-split format for the next WC site (and the next shortcut
    convolution) -- the result is a handle and the SplitTensor lands in the box (with .x32 when a backward will read fp32)."""

    @staticmethod
    def forward(ctx, h, s, up, box, x32, stat_groups):
        h = h.contiguous(); s = s.contiguous()
        ctx.up = bool(up)
        if box is None:
            return ops.resadd(h, s, up)
        want32 = bool(x32) and any(ctx.needs_input_grad[:2])
        if stat_groups and ops.resadd_stats_supported(h.shape, up, stat_groups):
            st = ops.resadd_stats_split(h, s, up, stat_groups, want_x32=want32)      # ... and K1's partials from the same pass
        else:
            st = ops.resadd_split(h, s, up, want_x32=want32)
        box.append(st)
        return _nan_handle(h.shape, h.device)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return g, (ops.patch_sum(g) if ctx.up else g), None, None, None, None


def residual_add(h, s, up, planes=False, x32=True, stat_groups=0):
    """h + (upsample2x of) s.  planes=True (the readers of the sum all have a planes path: layers.WhiteningColoring.takes_split,
    generator.Conv2D.takes_split): a handle carrying the sum as pre-split planes (`split_of(handle)`).  x32=False: no reader's backward
    needs the fp32 sum either (layers.WhiteningColoring.backward_takes_split) -- else it is written beside the planes while a gradient
    is wanted.  stat_groups > 0: the WC site that reads the sum is in training mode with that many statistic groups -- the add's pass
    then accumulates that site's covariance partials as well (ops.resadd_stats_split: the site's K1 launch does not exist)."""
    if planes and ops.resadd_split_supported(h.shape):
        box = []
        out = ResidualAddFunction.apply(h, s, bool(up), box, bool(x32), int(stat_groups))
        out._wc_split = box[0]
        return out
    return ResidualAddFunction.apply(h, s, bool(up), None, False, 0)


_SLOT_BASE = {}


def _group_slot_base(N, groups, Kc, dev):
    """int32 (N,): group(n) * Kc, the table index of sample n before its class slot is added.  It depends on the shapes
    only, and building it took four elementwise launches per site and step (arange, //, *, cast: ~20 us of the grouped
    forward site), so it is kept per (N, groups, Kc, device) -- except while a graph is being recorded, whose private pool
    must not hand memory to later eager calls."""
    key = (N, groups, Kc, str(dev))
    t = _SLOT_BASE.get(key)
    if t is None:
        t = ((torch.arange(N, device=dev, dtype=torch.int32) // (N // groups)) * Kc).to(torch.int32).contiguous()
        if not (t.is_cuda and torch.cuda.is_current_stream_capturing()):
            _SLOT_BASE[key] = t
    return t


def whiten_color_grouped(x, groups, gamma=None, beta=None, slot=None, moving_mean=None, moving_cov=None,
                         eps=1e-3, momentum=0.99, ddof=1, relu=False, per_sample=False, planes=False, decomposition='cholesky'):
    """Training-mode forward of `groups` INDEPENDENT batches stacked along N (no autograd): each run of N/groups
    samples is whitened with its own batch statistics, exactly as `groups` separate calls would be, but the
    covariance / Cholesky / inverse problems of the groups are solved side by side in one set of launches.
    Used for the generator passes inside the critic updates (fixed generator weights, no graph).
    per_sample: gamma (N, C, C) / beta (N, C) hold one coloring table per SAMPLE (more classes than samples per batch,
    layers.WhiteningColoring.coloring_table); sample n of group g is coloured by W_g^T gamma[n]."""
    N, C = x.shape[0], x.shape[-1]
    if N % groups != 0:
        raise ValueError("N must be a multiple of groups")
    st = split_of(x)                    # the residual add in front wrote pre-split planes: K1 / K3 read those
    x = x.detach() if st is not None else x.detach().contiguous()
    dev = x.device
    mu, L, W, cs = _whiten(x, st, True, eps, momentum, ddof, moving_mean, moving_cov, None, groups, decomposition)
    g = gamma.detach().contiguous() if gamma is not None else None
    b = beta.detach().contiguous() if beta is not None else None
    if per_sample and (g is None or g.shape[0] != N):
        raise ValueError("per_sample needs one coloring table per sample")
    Kc = N // groups if per_sample else (1 if g is None else g.shape[0])
    A, At, plan = ops.color(W, g, cs, groups, per_group=per_sample)
    # on planes the common centre is the planes' own: the biases are then the additive terms of the split apply directly
    # (beta - (mu_g - st.center) A, folded)
    if st is not None:
        center, bias = st.center, ops.group_bias_centered(mu.view(groups, C), A, b, st.center, groups, Kc, per_group=per_sample)
    else:
        center, bias = ops.group_bias(mu.view(groups, C), A, b, groups, Kc, per_group=per_sample)
    if per_sample:
        full_slot = _group_slot_base(N, N, 1, dev)
    else:
        full_slot = _group_slot_base(N, groups, Kc, dev)
        if slot is not None:
            full_slot = (full_slot + slot.view(-1)).to(torch.int32).contiguous()
    # (the predicted scale of a hand-off follows from the coloring tables as given: every group's whitened batch has unit covariance)
    handoff = planes and conv_handoff_supported(x.shape, relu, 1 if g is None else g.shape[0])
    return _k3(x, st, center, A, bias, full_slot, plan, True, relu, False, (g, b) if handoff else None)[0]


def _touched(*tensors):
    """The HIP stages update the moving statistics through raw pointers: tell torch (version counters), so that whatever is
    cached per version -- the eval-mode plan below -- sees the update."""
    inc = getattr(torch.autograd.graph, 'increment_version', None)
    if inc is not None:
        for t in tensors:
            if t is not None:
                inc(t)


class EvalPlan:
    """Eval-mode cache: the moving statistics are constants between weight updates, so
    mu, W = chol((1-eps) moving_cov + eps I)^-1, A = W^T Gamma and the apply plan are computed once and reused --
    the reference redoes the Cholesky on every scorer.py call.  Invalidated by any in-place change of the inputs."""

    def __init__(self):
        self.key = None
        self.val = None

    def get(self, C, gamma, moving_mean, moving_cov, eps, dev, gamma_key=None, decomposition='cholesky'):
        # gamma is usually rebuilt from the coloring weights on every call: key on those weights (gamma_key) when given
        gk = gamma_key if gamma_key is not None else (None if gamma is None else (gamma.data_ptr(), gamma._version))
        key = (_state.replays, C, eps, moving_mean._version, moving_cov._version, moving_mean.data_ptr(), moving_cov.data_ptr(),
               None if gamma is None else tuple(gamma.shape), gk)
        if key != self.key:
            with torch.no_grad():
                mu, L, W, cs = ops.factor(None, None, 1, C, eps, 0.0, 1, False, moving_mean.view(-1), moving_cov, dev,
                                          want_scale=True)
                if decomposition == 'zca':          # (a layer has one decomposition: the key needs no entry for it)
                    W = ops.zca(L, eps)[2]
                g = gamma.detach().contiguous() if gamma is not None else None
                A, At, plan = ops.color(W, g, cs)
            self.key, self.val = key, (mu, A, At, plan)
        return self.val


def whiten_color_eval_cached(x, cache, gamma=None, beta=None, slot=None, moving_mean=None, moving_cov=None, eps=1e-3,
                             gamma_key=None, relu=False, planes=False, decomposition='cholesky'):
    """Inference forward (no autograd) through an EvalPlan: one K3 launch per call once the plan is warm."""
    mu, A, At, plan = cache.get(x.shape[-1], gamma, moving_mean, moving_cov, eps, x.device, gamma_key, decomposition)
    b = beta.detach().contiguous() if beta is not None else None
    st = split_of(x)
    handoff = planes and conv_handoff_supported(x.shape, relu, A.shape[0])
    g = gamma.detach().contiguous() if (gamma is not None and handoff) else None
    if st is None:
        x = x.detach().contiguous()
    # on planes: the cached A, with the tables for THIS tensor's scales and the additive term beta + (center - mu) A built
    # inside the call (three launches; the planes' scales come from a sample of the data, not from the cached statistics)
    return _k3(x, st, mu, A, b, slot, plan if st is None else None, False, relu, False, (g, b) if handoff else None)[0]


def whiten_color(x, gamma=None, beta=None, slot=None, moving_mean=None, moving_cov=None, training=True,
                 eps=1e-3, momentum=0.99, ddof=1, process_group=None, relu=False, planes=False, decomposition='cholesky', renorm=False):
    """y = coloring(whitening(x)) (relu=True: max(y, 0) from the same kernel).  x: (N, H, W, C) float32 on the GPU,
    C % 32 == 0 (see layers for padding).  planes=True (relu'd sites whose consumer is conv.fast_conv): where K3 can, the
    result is a HANDLE -- a NaN tensor of y's shape without memory that carries the autograd edge -- with the output itself
    attached as the convolution's fp16 planes (handle._wc_planes); else the plain tensor.
    decomposition: 'cholesky' (W = L^-1) or 'zca' (W = U diag(lam^-1/2) U^T of Sigma + eps I; C <= 256, ops.zca_supported).
    renorm (norm 'dr', Cholesky only): in training mode the whitening is W_m sg(L) W -- the value is that of the moving statistics as they
    were before this call, W_m (x - mu_batch), the gradient flows through the batch factor (ops.renorm, ops.bwd_factor_renorm); no effect
    in evaluation mode."""
    if decomposition not in ('cholesky', 'zca'):
        raise ValueError(f"unknown decomposition {decomposition!r}")
    if renorm and decomposition != 'cholesky':
        raise NotImplementedError("renorm is defined for decomposition='cholesky' only")
    if renorm and training and moving_cov is None:
        raise ValueError("renorm whitens with the moving statistics: moving_cov is required")
    handoff = planes and conv_handoff_supported(x.shape, relu, 1 if gamma is None else gamma.shape[0])
    return WhitenColorFunction.apply(x, gamma, beta, slot, moving_mean, moving_cov, bool(training),
                                     float(eps), float(momentum), int(ddof), process_group, bool(relu), bool(handoff), split_of(x),
                                     decomposition, bool(renorm))


_ROUTE = {}


def split_route_supported(shape, training, groups=1):
    """Can a WC site of this NHWC input shape read its input as pre-split planes (K1: wc_whiten_split_f16x2 in training mode, K3:
    wc_apply_split_ex_f16x2)?  Shapes only (cached: the producer asks on every pass)."""
    key = (tuple(shape), bool(training), int(groups))
    r = _ROUTE.get(key)
    if r is None:
        C = shape[-1]
        M = 1
        for d in shape[:-1]:
            M *= d
        r = ops.apply_split_supported(tuple(shape)) and ((not training) or ops.stats_split_supported(M, C, groups))
        _ROUTE[key] = r
    return r


# ---------------------------------------------------------------------------------------------
# Modular pieces: the same HIP kernels exposed as two differentiable ops, so that a C x C stage
# written in torch (ZCA's eigendecomposition, renorm's constant factor) can sit between them.
# ---------------------------------------------------------------------------------------------
class FactorMixFunction(torch.autograd.Function):
    """Tables of the soft-assignment coloring (generator.py:69-78): out[t] = base + sum_e alpha[idx[t], e] dictionary[e] through
    wc_factor_mix_f32 / wc_factor_mix_bwd_f32 -- only the tables the batch uses, one launch forward, two to three backward."""

    @staticmethod
    def forward(ctx, dictionary, alpha, idx, base):
        dictionary, alpha = dictionary.contiguous(), alpha.contiguous()
        base = None if base is None else base.contiguous()
        ctx.save_for_backward(dictionary, alpha, idx)
        ctx.has_base = base is not None
        return ops.factor_mix(dictionary, alpha, idx, base)

    @staticmethod
    def backward(ctx, dout):
        dictionary, alpha, idx = ctx.saved_tensors
        dd, da, db = ops.factor_mix_bwd(dictionary, alpha, idx, dout.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                        ctx.has_base and ctx.needs_input_grad[3])
        return dd, da, None, db


def factor_mix(dictionary, alpha, idx=None, base=None):
    return FactorMixFunction.apply(dictionary, alpha, idx, base)


class MomentsFunction(torch.autograd.Function):
    """(sum, xtx) = K1(x).  backward: dx[m] = gsum + x[m] (gxtx + gxtx^T)  -- one K3 launch."""

    @staticmethod
    def forward(ctx, x):
        C = x.shape[-1]
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.stats(x.view(-1, C))

    @staticmethod
    def backward(ctx, gs, gxtx):
        (x,) = ctx.saved_tensors
        C = x.shape[-1]
        A = (gxtx + gxtx.t()).to(torch.float32).reshape(1, C, C).contiguous()
        b = gs.to(torch.float32).reshape(1, C).contiguous()
        return ops.apply(x, None, A, b, None)


class AffineRowsFunction(torch.autograd.Function):
    """y[n] = (x[n] - mu) A[slot[n]] + b[slot[n]] with gradients to x, mu, A and b (K3 / K4 / K6)."""

    @staticmethod
    def forward(ctx, x, mu, A, b, slot):
        x = x.contiguous()
        A = A.contiguous()
        mu_c = mu.contiguous() if mu is not None else None
        b_c = b.contiguous() if b is not None else None
        ctx.save_for_backward(x, A, mu_c if mu_c is not None else torch.empty(0, device=x.device),
                              slot if slot is not None else torch.empty(0, dtype=torch.int32, device=x.device))
        ctx.has_mu, ctx.has_b, ctx.has_slot = mu is not None, b is not None, slot is not None
        return ops.apply(x, mu_c, A, b_c, slot)

    @staticmethod
    def backward(ctx, gy):
        x, A, mu, slot = ctx.saved_tensors
        mu = mu if ctx.has_mu else None
        slot = slot if ctx.has_slot else None
        gy = gy.contiguous()
        Kc = A.shape[0]
        need_x, need_mu, need_A, need_b = ctx.needs_input_grad[:4]
        dx = dmu = dA = db = None
        At = A.transpose(1, 2).contiguous()
        if need_x:
            dx = ops.bwd_apply(gy, None, None, At, None, None, slot)
        if need_A or need_b or need_mu:
            R, gsum = ops.bwd_reduce(x, mu, gy, slot, Kc)
            if need_A:
                dA = R.to(torch.float32)
            if need_b and ctx.has_b:
                db = gsum.to(torch.float32)
            if need_mu and ctx.has_mu:
                dmu = -torch.einsum('kj,kcj->c', gsum, A.to(torch.float64)).to(torch.float32)
        return dx, dmu, dA, db, None


def whiten_color_modular(x, gamma=None, beta=None, slot=None, moving_mean=None, moving_cov=None, training=True,
                         eps=1e-3, momentum=0.99, ddof=1, decomposition='zca'):
    """Unfused composition moments -> torch C x C stage -> affine, for decompositions without a fused kernel.

    decomposition='zca' (generator.py:24, commented alternative): W = U diag(S^-1/2) U^T of Sigma + eps I;
    torch.linalg.eigh supplies the (reportedly unstable) gradient, as tf.svd did upstream.
    """
    C = x.shape[-1]
    M = x.numel() // C
    if training:
        s, xtx = MomentsFunction.apply(x)
        mu64 = s / M
        sigma = (xtx - torch.outer(s, s) / M) / (M - ddof)
        sigma = 0.5 * (sigma + sigma.t())
        if moving_mean is not None:
            with torch.no_grad():
                moving_mean.mul_(momentum).add_((1 - momentum) * mu64.to(torch.float32).view_as(moving_mean))
                moving_cov.mul_(momentum).add_((1 - momentum) * sigma.to(torch.float32))
    else:
        mu64 = moving_mean.view(-1).to(torch.float64)
        sigma = moving_cov.to(torch.float64)
    eye = torch.eye(C, dtype=torch.float64, device=x.device)
    if decomposition == 'zca':
        S, U = torch.linalg.eigh(sigma + eps * eye)
        W = (U * S.rsqrt()) @ U.t()
    elif decomposition == 'cholesky':
        L = torch.linalg.cholesky((1 - eps) * sigma + eps * eye)
        W = torch.linalg.solve_triangular(L, eye, upper=False)
    else:
        raise ValueError(f"unknown decomposition {decomposition!r}")
    if gamma is None:
        A = W.t().unsqueeze(0)
    else:
        A = torch.matmul(W.t().unsqueeze(0), gamma.to(torch.float64))
    return AffineRowsFunction.apply(x, mu64.to(torch.float32), A.to(torch.float32), beta, slot)


# ---------------------------------------------------------------------------------------------
# norm 'b': batch standardisation + diagonal coloring (csrc/wc_std.hip).  gamma / beta are (Kc, C) VECTORS: no C x C table exists here.
# ---------------------------------------------------------------------------------------------
def _std_tables(x, gamma, beta, moving_mean, moving_variance, training, eps, momentum, ddof, groups=1):
    """moments -> factor of one site: (mu, w, a, b).  Evaluation mode reads the moving statistics (no pass over x)."""
    C = x.shape[-1]
    M = x.numel() // C
    s = sq = None
    if training:
        s, sq = ops.std_stats(x.view(M, C), groups)
    mu, w, a, b = ops.std_factor(s, sq, M // groups, C, eps, momentum, ddof, training, moving_mean, moving_variance, gamma, beta,
                                 x.device, groups)
    if training:
        _touched(moving_mean, moving_variance)
    return mu, w, a, b


class StandardizeColorFunction(torch.autograd.Function):
    """y = relu?(gamma[slot] (x - mu) / sqrt(var + eps) + beta[slot]) as moments -> factor -> apply; the backward is the closed form
    (reduce -> factor -> apply) with the ReLU's decision recomputed from x and the forward's tables: nothing but x, the tables and the
    (C,) statistics is kept."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slot, moving_mean, moving_variance, training, eps, momentum, ddof, relu):
        x = x.detach().contiguous()
        g = gamma.detach().contiguous() if gamma is not None else None
        b_ = beta.detach().contiguous() if beta is not None else None
        mu, w, a, b = _std_tables(x, g, b_, moving_mean, moving_variance, training, eps, momentum, ddof)
        y = ops.std_apply(x, a, b, slot, relu)
        ctx.save_for_backward(x, g, slot, mu, w, a, b)
        ctx.training, ctx.relu = training, relu
        ctx.has_beta = beta is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g, slot, mu, w, a, b = ctx.saved_tensors
        gy = gy.contiguous()
        Kc = a.shape[0]
        C = x.shape[-1]
        gsum, gxsum = ops.std_bwd_reduce(x, gy, a, b, slot, Kc, ctx.relu)
        dgamma, dbeta, q, r = ops.std_bwd_factor(gsum, gxsum, mu.view(-1), w.view(-1), g, x.numel() // C, ctx.training,
                                                 want_dgamma=g is not None and ctx.needs_input_grad[1],
                                                 want_dbeta=ctx.has_beta and ctx.needs_input_grad[2])
        dx = ops.std_bwd_apply(x, gy, a, b, q, r, slot, ctx.relu) if ctx.needs_input_grad[0] else None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def standardize_color(x, gamma=None, beta=None, slot=None, moving_mean=None, moving_variance=None, training=True,
                      eps=1e-3, momentum=0.99, ddof=0, relu=False):
    """Batch standardisation fused with a diagonal coloring and, with relu=True, the ReLU behind it.  x (N, ..., C) float32 on the GPU,
    C % 32 == 0; gamma, beta (Kc, C) or None (1 / 0); slot (N,) int32 picks a sample's row (None: row 0).  Training mode normalises
    with the batch's biased variance and updates the moving statistics in place (variance times M / (M - ddof): 0 Keras, 1 torch);
    evaluation mode normalises with the moving statistics: one apply launch behind one small table launch."""
    return StandardizeColorFunction.apply(x, gamma, beta, slot, moving_mean, moving_variance, bool(training), float(eps),
                                          float(momentum), int(ddof), bool(relu))


def standardize_color_grouped(x, groups, gamma=None, beta=None, slot=None, moving_mean=None, moving_variance=None,
                              eps=1e-3, momentum=0.99, ddof=0, relu=False):
    """Training-mode forward of `groups` independent batches stacked along N (no autograd), as whiten_color_grouped: every run of
    N / groups samples is standardised with its own statistics and the moving statistics take the groups' updates one after the other
    -- bit for bit what `groups` separate calls give."""
    N = x.shape[0]
    if N % groups != 0:
        raise ValueError("N must be a multiple of groups")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, gamma, beta)):
        raise RuntimeError("standardize_color_grouped() is a forward-only path: wrap the call in torch.no_grad()")
    x = x.detach().contiguous()
    g = gamma.detach().contiguous() if gamma is not None else None
    b_ = beta.detach().contiguous() if beta is not None else None
    mu, w, a, b = _std_tables(x, g, b_, moving_mean, moving_variance, True, eps, momentum, ddof, groups)
    Kc = a.shape[0] // groups
    full_slot = _group_slot_base(N, groups, Kc, x.device)
    if slot is not None and Kc > 1:
        full_slot = (full_slot + slot.view(-1)).to(torch.int32).contiguous()
    return ops.std_apply(x, a, b, full_slot, relu)
