"""Float64 reference of the batch-standardisation site (norm 'b' + diagonal coloring + ReLU); numpy only, not collected.

Forward (training mode, per statistic group of M consecutive rows; x viewed as (rows, C), a sample is HW consecutive rows):

    mu = sum x / M            var = sum x^2 / M - mu^2  (biased)          w = 1 / sqrt(var + eps)
    moving_mean     <- momentum moving_mean     + (1 - momentum) mu
    moving_variance <- momentum moving_variance + (1 - momentum) var M / (M - ddof)
    y = gamma[slot] w (x - mu) + beta[slot],   relu: y = max(y, 0)

Evaluation mode takes mu, var from the moving statistics.  Backward, closed form (g' = gy where the mask holds):

    dbeta[k] = sum_{m in k} g'        dgamma[k] = w (sum_{m in k} g' x - mu dbeta[k])
    m1 = sum_k gamma[k] dbeta[k] / M  m2 = sum_k gamma[k] dgamma[k] / M
    dx = gamma[slot] w g' - w^2 m2 x + w (w mu m2 - m1)
"""
import numpy as np


def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    N, C = x.shape[0], x.shape[-1]
    return x.reshape(N, -1, C), N, C


def _tables(gamma, beta, C):
    g = np.ones((1, C)) if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(-1, C)
    b = np.zeros((1, C)) if beta is None else np.asarray(beta, dtype=np.float64).reshape(-1, C)
    K = max(g.shape[0], b.shape[0])
    return np.broadcast_to(g, (K, C)), np.broadcast_to(b, (K, C))


def forward(x, gamma=None, beta=None, slot=None, moving_mean=None, moving_variance=None, training=True, eps=1e-3, momentum=0.99,
            ddof=0, relu=False, groups=1):
    """-> (y, cache): y in x's shape (float64); cache holds mu, w (groups, C), the updated moving statistics and what backward needs."""
    x3, N, C = _rows(x)
    g, b = _tables(gamma, beta, C)
    sl = np.zeros(N, dtype=np.int64) if slot is None else np.asarray(slot).reshape(-1).astype(np.int64)
    mm = None if moving_mean is None else np.asarray(moving_mean, dtype=np.float64).reshape(C).copy()
    mv = None if moving_variance is None else np.asarray(moving_variance, dtype=np.float64).reshape(C).copy()
    assert N % groups == 0
    per = N // groups
    y = np.empty_like(x3)
    mus, ws = [], []
    for gi in range(groups):
        xs = x3[gi * per:(gi + 1) * per]
        if training:
            M = xs.shape[0] * xs.shape[1]
            mu = xs.sum((0, 1)) / M
            var = (xs * xs).sum((0, 1)) / M - mu * mu
            if mm is not None:
                mm = momentum * mm + (1.0 - momentum) * mu
                mv = momentum * mv + (1.0 - momentum) * var * M / (M - ddof)
        else:
            mu, var = mm, mv
        w = 1.0 / np.sqrt(var + eps)
        k = sl[gi * per:(gi + 1) * per]
        y[gi * per:(gi + 1) * per] = (g[k] * w)[:, None, :] * (xs - mu) + b[k][:, None, :]
        mus.append(mu)
        ws.append(w)
    pre = y
    if relu:
        y = np.maximum(pre, 0.0)
    cache = dict(x=x3, gamma=g, slot=sl, mu=np.stack(mus), w=np.stack(ws), pre=pre, relu=relu, training=training,
                 moving_mean=mm, moving_variance=mv, shape=np.asarray(x).shape)
    return y.reshape(np.asarray(x).shape), cache


def backward(gy, cache, mask=None):
    """-> (dx, dgamma (K, C), dbeta (K, C)) of one statistic group.  mask (x's shape, bool): where the ReLU passed -- given, it
    replaces the reference's own `pre > 0` (a value within rounding of zero may fall on either side in another precision)."""
    x3, g, sl = cache['x'], cache['gamma'], cache['slot']
    assert cache['mu'].shape[0] == 1, "the backward is defined for one statistic group"
    mu, w = cache['mu'][0], cache['w'][0]
    N, HW, C = x3.shape
    K = g.shape[0]
    gp = np.asarray(gy, dtype=np.float64).reshape(N, HW, C)
    if cache['relu']:
        m = (cache['pre'] > 0) if mask is None else np.asarray(mask).reshape(N, HW, C)
        gp = np.where(m, gp, 0.0)
    gs_n = gp.sum(1)                         # per sample
    gx_n = (gp * x3).sum(1)
    gsum = np.zeros((K, C))
    gxsum = np.zeros((K, C))
    np.add.at(gsum, sl, gs_n)
    np.add.at(gxsum, sl, gx_n)
    dbeta = gsum
    dgamma = w * (gxsum - mu * gsum)
    M = N * HW
    if cache['training']:
        m1 = (g * dbeta).sum(0) / M
        m2 = (g * dgamma).sum(0) / M
        q = -w * w * m2
        r = w * (w * mu * m2 - m1)
    else:
        q = r = np.zeros(C)
    dx = (g[sl] * w)[:, None, :] * gp + q * x3 + r
    return dx.reshape(cache['shape']), dgamma, dbeta


def rel(a, ref):
    """max-abs error over max-abs reference: the project's contract."""
    a = np.asarray(a, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))
