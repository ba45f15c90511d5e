"""The ResNet critic's tail -- ReLU, global pooling, the adversarial head, the AC-GAN class head and its cross entropy -- as one autograd
node over the three entries of csrc/wc_tail.hip.

    f[n]      = s sum_hw relu(y[n, hw])              s = 1 (sum_pool) or 1 / HW
    out[n]    = f[n] . w_out + b_out
    logits[n] = W_cls f[n] + b_cls                   with a class head
    ce[n]     = logsumexp(logits[n]) - logits[n, labels[n]]        with labels

The backward is the closed form: dlogits = g_logits + g_ce (softmax - onehot), dy = 1[y > 0] s (g_out w_out + dlogits W_cls), the weight
gradients sums over n of dlogits (or g_out) times f.  One launch forward, two backward; no expanded gradient, no masked copy of y.

On a CPU tensor, in float64, or for a shape wc_critic_tail_supported turns down, the same map runs in torch ops (`torch_tail`): the form
the float64 tests compare against, as in penalty.py.

The projection head (`projection_tail`) is a second node over three entries of its own:

    out[n] = f[n] . (w_out + E[cls[n]]) + b_out

with dy = 1[y > 0] s g_out (w_out + E[cls]), dw_out = g_out^T f and the dense dE[k] = sum over the samples of class k, in order, of
g_out[n] f[n].  A label outside [0, K) gives a NaN out, drops E from that sample's dy and reaches no row of dE.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from .ops import _ptr, _stream

last_route = None       # after a call: 'hip' or 'torch'


def torch_tail(y, w_out, b_out, w_cls=None, b_cls=None, labels=None, sum_pool=True):
    f = F.relu(y)
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, w_out.reshape(1, -1), b_out)
    if w_cls is None:
        return out, None, None
    logits = F.linear(f, w_cls, b_cls)
    if labels is None:
        return out, logits, None
    K = logits.shape[1]
    lab = labels.reshape(-1).long()
    valid = (lab >= 0) & (lab < K)
    picked = logits.gather(1, lab.clamp(0, K - 1)[:, None])[:, 0]
    ce = torch.where(valid, torch.logsumexp(logits, dim=1) - picked, torch.full_like(picked, float('nan')))     # (the kernel's contract)
    return out, logits, ce


def _f32(t):
    return t is None or (t.is_cuda and t.dtype == torch.float32)


def _dense(t):
    """contiguous and 16-byte aligned (a view at an odd storage offset is copied)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def hip_forward(y, w_out, b_out, w_cls=None, b_cls=None, labels=None, sum_pool=True):
    """wc_critic_tail_fwd_f32 on dense fp32 tensors: y (N, H, W, C), w_out (C,), labels int32 (N,) -> (feat (N, C), out (N, 1),
    logits (N, K), lse (N,), ce (N,)); the last three None without a class head / without labels"""
    N, H, W, C = y.shape
    K = 0 if w_cls is None else w_cls.shape[0]
    dev = y.device
    feat = torch.empty(N, C, dtype=torch.float32, device=dev)
    out = torch.empty(N, 1, dtype=torch.float32, device=dev)
    logits = torch.empty(N, K, dtype=torch.float32, device=dev) if K else None
    lse = torch.empty(N, dtype=torch.float32, device=dev) if K else None
    ce = torch.empty(N, dtype=torch.float32, device=dev) if labels is not None else None
    _lib.check(_lib.load().wc_critic_tail_fwd_f32(_ptr(y), _ptr(w_out), _ptr(b_out), _ptr(w_cls), _ptr(b_cls), _ptr(labels), N, H * W, C, K,
                                                  int(bool(sum_pool)), _ptr(feat), _ptr(out), _ptr(logits), _ptr(lse), _ptr(ce), _stream()),
               "wc_critic_tail_fwd_f32")
    return feat, out, logits, lse, ce


def hip_backward(y, w_out, w_cls, g_out, g_logits, g_ce, logits, lse, labels, sum_pool=True):
    """wc_critic_tail_bwd_f32: g_out (N,), g_logits (N, K) or None, g_ce (N,) or None and the forward's logits, lse, labels
    -> (dlogits (N, K) or None, dy)"""
    N, H, W, C = y.shape
    K = 0 if w_cls is None else w_cls.shape[0]
    dlogits = torch.empty(N, K, dtype=torch.float32, device=y.device) if K else None
    dy = torch.empty_like(y)
    _lib.check(_lib.load().wc_critic_tail_bwd_f32(_ptr(y), _ptr(w_out), _ptr(w_cls), _ptr(g_out), _ptr(g_logits), _ptr(g_ce), _ptr(logits),
                                                  _ptr(lse), _ptr(labels), N, H * W, C, K, int(bool(sum_pool)), _ptr(dlogits), _ptr(dy),
                                                  _stream()), "wc_critic_tail_bwd_f32")
    return dlogits, dy


def hip_wgrad(feat, g_out, dlogits):
    """wc_critic_tail_wgrad_f32 -> (dw_out (C,), db_out (1,), dW_cls (K, C), db_cls (K,)); the last two None without a class head"""
    N, C = feat.shape
    K = 0 if dlogits is None else dlogits.shape[1]
    dev = feat.device
    dw_out = torch.empty(C, dtype=torch.float32, device=dev)
    db_out = torch.empty(1, dtype=torch.float32, device=dev)
    dW_cls = torch.empty(K, C, dtype=torch.float32, device=dev) if K else None
    db_cls = torch.empty(K, dtype=torch.float32, device=dev) if K else None
    _lib.check(_lib.load().wc_critic_tail_wgrad_f32(_ptr(feat), _ptr(g_out), _ptr(dlogits), N, C, K, _ptr(dw_out), _ptr(db_out), _ptr(dW_cls),
                                                    _ptr(db_cls), _stream()), "wc_critic_tail_wgrad_f32")
    return dw_out, db_out, dW_cls, db_cls


class _CriticTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, w_out, b_out, w_cls, b_cls, labels, sum_pool):
        y = _dense(y.detach())
        w_out_c = _dense(w_out.detach().reshape(-1))
        w_cls_c = None if w_cls is None else _dense(w_cls.detach())
        b_out_c = None if b_out is None else b_out.detach().contiguous()
        b_cls_c = None if b_cls is None else b_cls.detach().contiguous()
        lab = None if labels is None else labels.detach().reshape(-1).to(torch.int32).contiguous()
        feat, out, logits, lse, ce = hip_forward(y, w_out_c, b_out_c, w_cls_c, b_cls_c, lab, sum_pool)
        ctx.save_for_backward(y, w_out_c, w_cls_c, feat, logits, lse, lab)
        ctx.meta = (bool(sum_pool), tuple(w_out.shape), b_out is not None, b_cls is not None)
        ctx.set_materialize_grads(False)
        return out, logits, ce

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_logits, g_ce):
        y, w_out, w_cls, feat, logits, lse, lab = ctx.saved_tensors
        sum_pool, w_out_shape, has_b_out, has_b_cls = ctx.meta
        N = y.shape[0]
        g_out = torch.zeros(N, dtype=torch.float32, device=y.device) if g_out is None else g_out.reshape(N).to(torch.float32).contiguous()
        g_logits = None if g_logits is None else g_logits.to(torch.float32).contiguous()
        g_ce = None if g_ce is None else g_ce.reshape(N).to(torch.float32).contiguous()
        dlogits, dy = hip_backward(y, w_out, w_cls, g_out, g_logits, g_ce, logits, lse, lab, sum_pool)
        dw_out = db_out = dW_cls = db_cls = None
        if any(ctx.needs_input_grad[1:5]):
            dw_out, db_out, dW_cls, db_cls = hip_wgrad(feat, g_out, dlogits)
            dw_out = dw_out.view(w_out_shape)
        return (dy if ctx.needs_input_grad[0] else None, dw_out, db_out if has_b_out else None, dW_cls, db_cls if has_b_cls else None,
                None, None)


def hip_route(y, w_out, b_out=None, w_cls=None, b_cls=None):
    """whether critic_tail runs these tensors on the kernels"""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        return False
    if not all(_f32(t) for t in (w_out, b_out, w_cls, b_cls)):
        return False
    N, H, W, C = y.shape
    if w_out.numel() != C or (w_cls is not None and (w_cls.dim() != 2 or w_cls.shape[1] != C)):
        return False
    K = 0 if w_cls is None else w_cls.shape[0]
    return bool(_lib.load().wc_critic_tail_supported(N, H * W, C, K))


def critic_tail(y, w_out, b_out, w_cls=None, b_cls=None, labels=None, sum_pool=True):
    """y (N, H, W, C) NHWC, the last block's output BEFORE its ReLU; w_out (1, C) or (C,) -- a Linear's weight or the spectral-norm op's
    output --, w_cls (K, C), labels (N,) or (N, 1) integers.  -> (out (N, 1), logits (N, K) or None, ce (N,) or None); gradients go to y,
    both weights and both biases.  Labels without a class head are an error."""
    global last_route
    if labels is not None and w_cls is None:
        raise ValueError("critic_tail: labels need a class head (w_cls)")
    if hip_route(y, w_out, b_out, w_cls, b_cls):
        last_route = 'hip'
        return _CriticTail.apply(y, w_out, b_out, w_cls, b_cls, labels, bool(sum_pool))
    last_route = 'torch'
    return torch_tail(y, w_out, b_out, w_cls, b_cls, labels, sum_pool)


# ---------------------------------------------------------------------------------------------------------------------------------
# the projection head
# ---------------------------------------------------------------------------------------------------------------------------------
def torch_projection_tail(y, w_out, b_out, emb, cls, sum_pool=True):
    f = F.relu(y)
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, w_out.reshape(1, -1), b_out)
    K = emb.shape[0]
    idx = cls.reshape(-1).long()
    valid = ((idx >= 0) & (idx < K))[:, None]
    rows = torch.where(valid, F.embedding(idx.clamp(0, K - 1), emb), torch.zeros((), dtype=emb.dtype, device=emb.device))
    out = out + (rows * f).sum(dim=1, keepdim=True)
    # the kernel's contract: NaN for a label outside [0, K), whose gradient still reaches y, w_out and b_out through the adversarial head
    return out + torch.where(valid, torch.zeros_like(out), torch.full_like(out, float('nan'))).detach()


def hip_projection_forward(y, w_out, b_out, emb, cls, sum_pool=True):
    """wc_critic_proj_fwd_f32 on dense fp32 tensors: y (N, H, W, C), w_out (C,), emb (K, C), cls int32 (N,) -> (feat (N, C), out (N, 1))"""
    N, H, W, C = y.shape
    feat = torch.empty(N, C, dtype=torch.float32, device=y.device)
    out = torch.empty(N, 1, dtype=torch.float32, device=y.device)
    _lib.check(_lib.load().wc_critic_proj_fwd_f32(_ptr(y), _ptr(w_out), _ptr(b_out), _ptr(emb), _ptr(cls), N, H * W, C, emb.shape[0],
                                                  int(bool(sum_pool)), _ptr(feat), _ptr(out), _stream()), "wc_critic_proj_fwd_f32")
    return feat, out


def hip_projection_backward(y, w_out, emb, cls, g_out, sum_pool=True):
    """wc_critic_proj_bwd_f32: g_out (N,) -> dy"""
    N, H, W, C = y.shape
    dy = torch.empty_like(y)
    _lib.check(_lib.load().wc_critic_proj_bwd_f32(_ptr(y), _ptr(w_out), _ptr(emb), _ptr(cls), _ptr(g_out), N, H * W, C, emb.shape[0],
                                                  int(bool(sum_pool)), _ptr(dy), _stream()), "wc_critic_proj_bwd_f32")
    return dy


def hip_projection_wgrad(feat, g_out, cls, K):
    """wc_critic_proj_wgrad_f32 -> (dw_out (C,), db_out (1,), demb (K, C)); demb is written in full"""
    N, C = feat.shape
    dw_out = torch.empty(C, dtype=torch.float32, device=feat.device)
    db_out = torch.empty(1, dtype=torch.float32, device=feat.device)
    demb = torch.empty(K, C, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().wc_critic_proj_wgrad_f32(_ptr(feat), _ptr(g_out), _ptr(cls), N, C, K, _ptr(dw_out), _ptr(db_out), _ptr(demb),
                                                    _stream()), "wc_critic_proj_wgrad_f32")
    return dw_out, db_out, demb


class _ProjectionTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, w_out, b_out, emb, cls, sum_pool):
        y = _dense(y.detach())
        w_out_c = _dense(w_out.detach().reshape(-1))
        emb_c = _dense(emb.detach())
        b_out_c = None if b_out is None else b_out.detach().contiguous()
        idx = cls.detach().reshape(-1).to(torch.int32).contiguous()
        feat, out = hip_projection_forward(y, w_out_c, b_out_c, emb_c, idx, sum_pool)
        ctx.save_for_backward(y, w_out_c, emb_c, feat, idx)
        ctx.meta = (bool(sum_pool), tuple(w_out.shape), b_out is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        y, w_out, emb, feat, idx = ctx.saved_tensors
        sum_pool, w_out_shape, has_b_out = ctx.meta
        g_out = g_out.reshape(y.shape[0]).to(torch.float32).contiguous()
        dy = hip_projection_backward(y, w_out, emb, idx, g_out, sum_pool) if ctx.needs_input_grad[0] else None
        dw_out = db_out = demb = None
        if any(ctx.needs_input_grad[1:4]):
            dw_out, db_out, demb = hip_projection_wgrad(feat, g_out, idx, emb.shape[0])
            dw_out = dw_out.view(w_out_shape)
        return dy, dw_out, db_out if has_b_out else None, demb, None, None


def projection_route(y, w_out, b_out, emb, cls):
    """whether projection_tail runs these tensors on the kernels"""
    if not (torch.is_tensor(y) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4):
        return False
    if not (all(_f32(t) for t in (w_out, b_out, emb)) and emb is not None and emb.dim() == 2 and cls.is_cuda and not cls.is_floating_point()):
        return False
    N, H, W, C = y.shape
    if w_out.numel() != C or emb.shape[1] != C or cls.numel() != N:
        return False
    return bool(_lib.load().wc_critic_proj_supported(N, H * W, C, emb.shape[0]))


def projection_tail(y, w_out, b_out, emb, cls, sum_pool=True):
    """y (N, H, W, C) NHWC, the last block's output BEFORE its ReLU; w_out (1, C) or (C,) and emb (K, C) -- a layer's weight or the
    spectral-norm op's output --, cls (N,) or (N, 1) integers.  -> out (N, 1) = f . (w_out + emb[cls]) + b_out; gradients go to y, w_out,
    b_out and emb (dense, every row written)."""
    global last_route
    if projection_route(y, w_out, b_out, emb, cls):
        last_route = 'hip'
        return _ProjectionTail.apply(y, w_out, b_out, emb, cls, bool(sum_pool))
    last_route = 'torch'
    return torch_projection_tail(y, w_out, b_out, emb, cls, sum_pool)
