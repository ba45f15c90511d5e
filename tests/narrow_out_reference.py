"""Float64 direct sums for the narrow-OUTPUT convolution (wc_conv_narrow_out_f32, csrc/wc_conv.hip) in NumPy, its rows and their inputs
(not collected: no test_ prefix).  tests/test_narrow_out.py holds this file to torch's float64 autograd and shows that it tells the
kernel's possible faults apart; tests/test_narrow_out_gpu.py holds the kernel to it.

The map, p = k // 2, g the wide NHWC tensor (Cw channels), c < Cn:

    data gradient  (w (Cw, Cn, k, k), the layer whose gradient it is)   out[n, y, x, c] = sum m(g)[n, y - (r - p), x - (s - p), o] w[o, c, r, s]
    forward        (v (Cn, Cw, k, k), a layer with few outputs)          out[n, y, x, c] = sum m(g)[n, y + (r - p), x + (s - p), o] v[c, o, r, s]

m(g) = g, or with a mask h of g's shape threshold_backward(g, h, 0) = where(h <= 0, 0, g).  Positions outside the image contribute zero."""
from __future__ import annotations

import collections
import functools

import numpy as np

BOUND = 1e-5            # max |error| / max |reference|: the narrow kernels' data-gradient bound (tests/test_narrow_edges_gpu.py)

Row = collections.namedtuple('Row', 'name N H W Cw Cn k')

ROWS = [
    Row('3x5x7-64-3-k3', 3, 5, 7, 64, 3, 3),            # M = 105: a partial last tile, tiles across image and row borders
    Row('2x1x2-32-1-k3', 2, 1, 2, 32, 1, 3),            # H = 1, the smallest W
    Row('2x6x8-64-3-k1', 2, 6, 8, 64, 3, 1),
    Row('1x4x4-192-1-k3', 1, 4, 4, 192, 1, 3),          # several k-chunks
    Row('2x8x8-256-3-k3', 2, 8, 8, 256, 3, 3),
    Row('4x64x64-64-3-k3', 4, 64, 64, 64, 3, 3),        # several workgroups per image and tiles per wave
    Row('1x3x720-32-1-k3', 1, 3, 720, 32, 1, 3),        # the widest grid the predicate takes: one output row per workgroup, halos either side
]
WIDEST = ROWS[-1]
POISON_ROWS = ('3x5x7-64-3-k3', '2x1x2-32-1-k3', '1x4x4-192-1-k3')

# every recipe's image-layer grids (H = W), at Cn 3 (1 for the MNIST recipes' 28 and 14) and the widths the critics' first blocks have
RECIPE_GRIDS = (128, 64, 48, 32, 28, 24, 16, 14)
RECIPE_WIDTHS = (64, 128, 256)


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def inputs(row):
    """-> g, h (N, H, W, Cw), w (Cw, Cn, k, k), v (Cn, Cw, k, k): float32.  h holds exact zeros and -0.0 (both masked out)."""
    rng = np.random.default_rng([row.N, row.H, row.W, row.Cw, row.Cn, row.k])
    shape = (row.N, row.H, row.W, row.Cw)
    g = rng.standard_normal(shape).astype(np.float32)
    h = rng.standard_normal(shape).astype(np.float32)
    pick = rng.random(shape)
    h[pick < 0.05] = 0.0
    h[(pick >= 0.05) & (pick < 0.10)] = -0.0
    w = (0.2 * rng.standard_normal((row.Cw, row.Cn, row.k, row.k))).astype(np.float32)
    v = (0.2 * rng.standard_normal((row.Cn, row.Cw, row.k, row.k))).astype(np.float32)
    return g, h, w, v


def masked(g, h):
    """threshold_backward(g, h, 0) in float64"""
    return np.where(h <= 0, 0.0, g.astype(np.float64))


def narrow_out(g, w, mask=None, forward=False):
    """The map of the module docstring in float64: w (Cw, Cn, k, k), or with forward=True (Cn, Cw, k, k)."""
    g64 = g.astype(np.float64) if mask is None else masked(g, mask)
    w64 = w.astype(np.float64)
    if forward:
        w64 = w64.transpose(1, 0, 2, 3)              # -> [o, c, r, s]
    N, H, W, _ = g64.shape
    k = w64.shape[2]
    p = k // 2
    gp = np.pad(g64, ((0, 0), (p, p), (p, p), (0, 0)))
    out = np.zeros((N, H, W, w64.shape[1]))
    for r in range(k):
        for s in range(k):
            dy, dx = (r - p, s - p) if forward else (-(r - p), -(s - p))
            out += np.einsum('nyxo,oc->nyxc', gp[:, p + dy:p + dy + H, p + dx:p + dx + W, :], w64[:, :, r, s])
    return out


def rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """{'dx', 'dx_masked', 'y', 'y_masked'} of a row in float64, computed once and shared (read-only)"""
    row = by_name(name)
    g, h, w, v = inputs(row)
    out = dict(dx=narrow_out(g, w), dx_masked=narrow_out(g, w, h), y=narrow_out(g, v, forward=True), y_masked=narrow_out(g, v, h, forward=True))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- what a faulty kernel would compute (float64; tests/test_narrow_out.py: each is far outside the bound on the rows above) ---------------
def faulty(g, w, mask, fault, band=1):
    """The data gradient as the kernel's design would compute it with one fault:
    'halo'        a workgroup owns `band` output rows and leaves out the products of the rows above and below its band
    'unmirrored'  the taps are read in the forward's direction
    'mask_after'  the mask's first Cn channels applied to the sums instead of to g
    'partial'     the products of the last, partial 32-pixel tile (N*H*W % 32 pixels) are never written"""
    if fault == 'unmirrored':
        return narrow_out(g, np.ascontiguousarray(w.transpose(1, 0, 2, 3)), mask, forward=True)
    if fault == 'mask_after':
        return narrow_out(g, w) * np.where(mask[..., :w.shape[1]] <= 0, 0.0, 1.0)
    g64 = g.astype(np.float64) if mask is None else masked(g, mask)
    N, H, W, Cw = g64.shape
    if fault == 'partial':
        flat = g64.reshape(-1, Cw).copy()
        M = flat.shape[0]
        if M % 32:
            flat[M - M % 32:] = 0.0
        return narrow_out(flat.reshape(g64.shape), w)
    if fault == 'halo':
        out = np.zeros((N, H, W, w.shape[1]))
        for y0 in range(0, H, band):
            part = np.zeros_like(g64)
            part[:, y0:y0 + band] = g64[:, y0:y0 + band]
            out[:, y0:y0 + band] = narrow_out(part, w)[:, y0:y0 + band]
        return out
    raise ValueError(fault)
