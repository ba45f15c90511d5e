"""Float64 restatement of the ResNet critic's tail and of its closed-form backward (csrc/wc_tail.hip); plain torch,
any device, not collected.

    f[n,c]     = s sum_hw relu(y[n,hw,c])              s = 1 (sum pooling) or 1 / HW (mean pooling)
    out[n]     = f[n] . w_out + b_out
    logit[n,k] = f[n] . W_cls[k] + b_cls[k]
    ce[n]      = lse[n] - logit[n, label[n]]           NaN for a label outside [0, K)

    dlogits[n,k] = g_logits[n,k] + g_ce[n] (softmax[n,k] - 1[k = label[n]])          (no class gradient for a label outside [0, K))
    dy[n,hw,c]   = y[n,hw,c] > 0 ? s (g_out[n] w_out[c] + sum_k dlogits[n,k] W_cls[k,c]) : 0
    dw_out = g_out^T f,  db_out = sum g_out,  dW_cls = dlogits^T f,  db_cls = sum_n dlogits
"""
import torch


def forward(y, w_out, b_out, w_cls=None, b_cls=None, labels=None, sum_pool=True):
    """y (N, H, W, C) -> dict(feat (N, C), out (N,), logits (N, K), lse (N,), ce (N,)); the last three only with their inputs.  Everything
    is converted to float64 first."""
    y = y.double()
    N, H, W, C = y.shape
    s = 1.0 if sum_pool else 1.0 / (H * W)
    r = dict(feat=s * y.clamp_min(0).reshape(N, H * W, C).sum(dim=1))
    r['out'] = r['feat'] @ w_out.double().reshape(C) + (0.0 if b_out is None else b_out.double().reshape(()))
    if w_cls is not None:
        r['logits'] = r['feat'] @ w_cls.double().t() + (0.0 if b_cls is None else b_cls.double())
        m = r['logits'].max(dim=1, keepdim=True).values
        r['lse'] = (m + (r['logits'] - m).exp().sum(dim=1, keepdim=True).log())[:, 0]
        if labels is not None:
            K = w_cls.shape[0]
            lab = labels.reshape(-1).long()
            valid = (lab >= 0) & (lab < K)
            picked = r['logits'].gather(1, lab.clamp(0, K - 1)[:, None])[:, 0]
            r['ce'] = torch.where(valid, r['lse'] - picked, torch.full_like(picked, float('nan')))
    return r


def backward(y, w_out, w_cls, fwd, g_out, g_logits=None, g_ce=None, labels=None, sum_pool=True):
    """the closed form from the forward's dict -> dict(dy, dw_out (C,), db_out (), dlogits, dW_cls, db_cls)"""
    y = y.double()
    N, H, W, C = y.shape
    s = 1.0 if sum_pool else 1.0 / (H * W)
    g_out = g_out.double().reshape(N)
    coef = g_out[:, None] * w_out.double().reshape(1, C)
    r = {}
    if w_cls is not None:
        K = w_cls.shape[0]
        d = torch.zeros(N, K, dtype=torch.float64, device=y.device) if g_logits is None else g_logits.double().clone()
        if g_ce is not None:
            lab = labels.reshape(-1).long()
            valid = (lab >= 0) & (lab < K)
            soft = (fwd['logits'] - fwd['lse'][:, None]).exp()
            onehot = torch.zeros_like(soft).scatter_(1, lab.clamp(0, K - 1)[:, None], 1.0)
            d = d + torch.where(valid[:, None], g_ce.double().reshape(N, 1) * (soft - onehot), torch.zeros_like(soft))
        r['dlogits'] = d
        coef = coef + d @ w_cls.double()
        r['dW_cls'] = d.t() @ fwd['feat']
        r['db_cls'] = d.sum(dim=0)
    r['dy'] = (y > 0).double() * (s * coef).reshape(N, 1, 1, C)
    r['dw_out'] = g_out @ fwd['feat']
    r['db_out'] = g_out.sum()
    return r


def rel(a, ref):
    """max |a - ref| over the reference's maximum (an all-zero reference: the absolute error)"""
    scale = float(ref.detach().abs().max()) if ref.numel() else 0.0
    return float((a.detach().double() - ref.detach().double()).abs().max()) / (scale if scale > 0 else 1.0) if ref.numel() else 0.0
