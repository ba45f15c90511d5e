"""Float64 restatement of the projection critic's tail and of its closed-form backward (csrc/wc_tail.hip); plain
torch, any device, not collected.

    f[n,c]     = s sum_hw relu(y[n,hw,c])              s = 1 (sum pooling) or 1 / HW (mean pooling)
    out[n]     = f[n] . (w_out + E[cls[n]]) + b_out    NaN for a label outside [0, K)

    dy[n,hw,c] = y[n,hw,c] > 0 ? s g_out[n] (w_out[c] + E[cls[n],c]) : 0            (a label outside [0, K): the w_out term alone)
    dw_out = g_out^T f,  db_out = sum g_out,  dE[k] = sum_{n : cls[n] = k} g_out[n] f[n]       (a label outside [0, K): no row)
"""
import torch

from tail_reference import rel      # noqa: F401  (the tests' measure: max |a - ref| over the reference's maximum)


def _rows(E, cls):
    """(E[cls[n]] with a zero row for a label outside [0, K), which labels are valid, the clamped index)"""
    K = E.shape[0]
    idx = cls.reshape(-1).long()
    valid = (idx >= 0) & (idx < K)
    safe = idx.clamp(0, K - 1)
    return torch.where(valid[:, None], E.double()[safe], torch.zeros((), dtype=torch.float64, device=E.device)), valid, safe


def forward(y, w_out, b_out, E, cls, sum_pool=True):
    """y (N, H, W, C), E (K, C), cls (N,) or (N, 1) -> dict(feat (N, C), out (N,)).  Everything is converted to float64 first."""
    y = y.double()
    N, H, W, C = y.shape
    s = 1.0 if sum_pool else 1.0 / (H * W)
    feat = s * y.clamp_min(0).reshape(N, H * W, C).sum(dim=1)
    rows, valid, _ = _rows(E, cls)
    out = (feat * (w_out.double().reshape(1, C) + rows)).sum(dim=1) + (0.0 if b_out is None else b_out.double().reshape(()))
    return dict(feat=feat, out=torch.where(valid, out, torch.full_like(out, float('nan'))))


def backward(y, w_out, E, cls, fwd, g_out, sum_pool=True):
    """the closed form from the forward's dict -> dict(dy, dw_out (C,), db_out (), dE (K, C))"""
    y = y.double()
    N, H, W, C = y.shape
    s = 1.0 if sum_pool else 1.0 / (H * W)
    g = g_out.double().reshape(N)
    rows, valid, safe = _rows(E, cls)
    coef = g[:, None] * (w_out.double().reshape(1, C) + rows)
    contrib = torch.where(valid[:, None], g[:, None] * fwd['feat'], torch.zeros((), dtype=torch.float64, device=y.device))
    dE = torch.zeros(E.shape[0], C, dtype=torch.float64, device=y.device).index_add_(0, safe, contrib)
    return dict(dy=(y > 0).double() * (s * coef).reshape(N, 1, 1, C), dw_out=g @ fwd['feat'], db_out=g.sum(), dE=dE)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows the GPU test compares and the CPU test measures its sensitivity on: fp32 inputs, made on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 4, 1), (3, 36, 132, 7), (8, 64, 128, 10), (128, 64, 256, 10), (128, 64, 256, 100), (5, 144, 256, 100), (4, 64, 1024, 200),
          (6, 64, 1024, 1024)]             # (N, HW, C, K)
GRID = {1: (1, 1), 36: (6, 6), 64: (8, 8), 144: (12, 12)}


def case(N, HW, C, K, sum_pool, seed, pattern='random'):
    """w_out and the table sized so that out is of order one.  pattern: 'random' (the first label 0, the last K - 1), 'equal' (every sample
    of one class: one row of dE sums N terms) or 'distinct' (K >= N: no two samples share a row)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    H, W = GRID[HW]
    size = (0.4 * HW if sum_pool else 0.4) * C ** 0.5
    c = dict(y=rn(N, H, W, C), w_out=rn(C) / size, b_out=0.1 * rn(1), emb=rn(K, C) / size, g_out=rn(N))
    if pattern == 'random':
        cls = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
        cls[0], cls[-1] = 0, K - 1
    elif pattern == 'equal':
        cls = torch.full((N,), int(torch.randint(0, K, (1,), generator=g)), dtype=torch.int32)
    else:
        assert pattern == 'distinct' and K >= N
        cls = torch.randperm(K, generator=g)[:N].to(torch.int32)
    c['cls'] = cls
    return c


def rows(shape):
    """(label, case, sum_pool) of one shape: every label pattern that fits and both poolings; one row without a bias and one whose first
    sample is negative throughout"""
    N, HW, C, K = shape
    out = []
    for i, pattern in enumerate(('random', 'equal') + (('distinct',) if K >= N else ())):
        for sum_pool in (True, False):
            out.append((f"{pattern} {'sum' if sum_pool else 'mean'}", case(N, HW, C, K, sum_pool, 100 + 10 * i + sum_pool, pattern), sum_pool))
    c = case(N, HW, C, K, True, 7)
    c['b_out'] = None
    out.append(("random sum no bias", c, True))
    c = case(N, HW, C, K, False, 8)
    c['y'][0] = -c['y'][0].abs()
    out.append(("random mean sample 0 negative", c, False))
    return out


def reference(c, sum_pool):
    fwd = forward(c['y'], c['w_out'], c['b_out'], c['emb'], c['cls'], sum_pool)
    return dict(fwd, **backward(c['y'], c['w_out'], c['emb'], c['cls'], fwd, c['g_out'], sum_pool))
