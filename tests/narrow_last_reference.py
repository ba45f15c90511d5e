"""The generator's last layer on the narrow kernels (conv._NarrowLastConv): the row table, the rows' inputs and
their float64 references for tests/test_narrow_last.py (no GPU) and tests/test_narrow_last_gpu.py (not collected: no test_ prefix).

A row `NxHxW-Cw-Cn-k` is the layer x (N, H, W, Cw) -> y (N, H, W, Cn) with w (Cn, Cw, k, k) and a bias b (Cn,):

    y    wc_conv_narrow_out_bias_f32, the taps mirrored      narrow_out_reference.narrow_out(x, w, forward=True) + b
    dx   wc_conv_fwd_narrow32_f32, mirrored                  narrow_reference.forward(gy, w, mirrored=True)
    dW   wc_conv_wrw_narrow32_f32, the operands exchanged    narrow_reference.exchanged_gradient(x, gy, k)
    db   the column sums of gy

The float64 sums are those two helpers' (imported, not restated), and so are the bounds: BOUND = 1e-5 for y, Y_BOUND = 1e-5 for dx,
DW_BOUND = 2e-6 for dW and db, each max |error| over max |reference| of the tensor.  In the narrow kernels' own terms the wide side Cw is
their `Cout` and Cn their `Cin`."""
import collections
import functools
import zlib

import numpy as np

import narrow_out_reference as NO
import narrow_reference as NR

BOUND, Y_BOUND, DW_BOUND = NO.BOUND, NR.Y_BOUND, NR.DW_BOUND

# nparts: pixel ranges of the weight gradient (narrow_reference.plan's, a literal here); groups: channel groups of the weight gradient --
# Cw / 32 groups of 32 where Cw % 64 == 32 (every group of such a layer is 32 wide), ceil(Cw / 128) groups of 128 where Cw % 64 == 0
Row = collections.namedtuple('Row', 'name N H W Cw Cn k nparts groups edge')

ROWS = [
    Row('2x5x7-32-3-k3', 2, 5, 7, 32, 3, 3, 1, 1, 'M = 70: a partial 32-pixel tile, a partial batch of pixel pairs, one 32-group'),
    Row('1x2x2-32-1-k3', 1, 2, 2, 32, 1, 3, 1, 1, 'W = 2, the smallest width the multiply-shift division takes; M = 4'),
    Row('3x4x6-96-3-k3', 3, 4, 6, 96, 3, 3, 1, 3, 'three 32-groups'),
    Row('2x8x8-160-2-k1', 2, 8, 8, 160, 2, 1, 1, 5, 'k = 1; five 32-groups; whole tiles'),
    Row('1x33x3-32-3-k3', 1, 33, 3, 32, 3, 3, 1, 1, 'nine bands of four rows behind a halo, the last band one row'),
    Row('5x16x16-32-3-k3', 5, 16, 16, 32, 3, 3, 10, 1, 'M = 1280: ten partials through the reduce'),
    Row('2x128x128-32-3-k3', 2, 128, 128, 32, 3, 3, 256, 1, "the recipe's grid: bands of three rows, 43 per image, the last with two; 256 partials"),
    Row('2x64x64-64-3-k3', 2, 64, 64, 64, 3, 3, 64, 1, 'a 64-multiple width: the bits of the entries that were there'),
]
POISON_ROWS = ('2x5x7-32-3-k3', '1x2x2-32-1-k3', '2x8x8-160-2-k1')          # rows 1, 2 and 4
OLD_BITS_ROW = '2x64x64-64-3-k3'

# declined by every narrow predicate, as (N, H, W, Cn, Cw, k): W = 1, ksize = 5, ksize^2 * Cn >= 32 (k = 3: Cn = 4; k = 1: Cn = 32), Cw = 48
DECLINED = [(2, 5, 1, 3, 32, 3), (2, 5, 1, 3, 128, 3), (2, 5, 7, 1, 128, 5), (2, 5, 7, 4, 128, 3), (2, 5, 7, 32, 128, 1), (2, 5, 7, 3, 48, 3),
            (2, 5, 7, 3, 48, 1)]


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def name_of(N, H, W, Cw, Cn, k):
    return f"{N}x{H}x{W}-{Cw}-{Cn}-k{k}"


def inputs(row):
    """float32 x (N, H, W, Cw), w (Cn, Cw, k, k), b (Cn,), gy (N, H, W, Cn).  The bias is 0.5-sigma beside outputs of about unit size:
    a dropped bias is far above the bounds."""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    x = (rng.standard_normal((row.N, row.H, row.W, row.Cw)) * 0.8 + 0.1).astype(np.float32)
    w = (rng.standard_normal((row.Cn, row.Cw, row.k, row.k)) / np.sqrt(row.Cw * row.k * row.k)).astype(np.float32)
    b = (rng.standard_normal(row.Cn) * 0.5 + 0.25).astype(np.float32)
    gy = rng.standard_normal((row.N, row.H, row.W, row.Cn)).astype(np.float32)
    return x, w, b, gy


@functools.lru_cache(maxsize=None)
def reference(name):
    """{'y0' (no bias), 'y', 'dx', 'dw', 'db'} of a row in float64, computed once and shared (read-only)"""
    row = by_name(name)
    x, w, b, gy = inputs(row)
    y0 = NO.narrow_out(x, w, forward=True)
    out = dict(y0=y0, y=y0 + b.astype(np.float64), dx=NR.forward(gy, w, None, mirrored=True), dw=NR.exchanged_gradient(x, gy, row.k),
               db=gy.astype(np.float64).sum(axis=(0, 1, 2)))
    for a in out.values():
        a.setflags(write=False)
    return out


rel = NR.rel


# ---- what a faulty route would compute (float64): tests/test_narrow_last.py shows each far outside the bounds on a row of the table ---------
def faulty(row, fault):
    """-> (name of the reference it belongs to, the faulty tensor):
    'unmirrored'  the forward's taps read in the data gradient's direction
    'no_bias'     the bias left out of y
    'remainder'   the last 32-channel group of the wide side never computed: dW's last 32 input channels and dx's last 32 channels zero
    'partial'     the first pixel range's partial (8 waves x 16 pixels) missing from the weight gradient's reduce"""
    x, w, b, gy = inputs(row)
    ref = reference(row.name)
    if fault == 'unmirrored':
        return 'y', NO.narrow_out(x, np.ascontiguousarray(w.transpose(1, 0, 2, 3)), forward=False) + b.astype(np.float64)
    if fault == 'no_bias':
        return 'y', ref['y0']
    if fault == 'remainder':
        dw = ref['dw'].copy()
        dw[:, -32:] = 0.0
        return 'dw', dw
    if fault == 'remainder_dx':
        dx = ref['dx'].copy()
        dx[..., -32:] = 0.0
        return 'dx', dx
    if fault == 'partial':
        M = row.N * row.H * row.W
        keep = np.arange(128, M)
        dwt, _ = NR.gradients_of(NR.product_rows(gy, x, row.k, pixels=keep), row.Cn, row.k)
        return 'dw', dwt.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1].copy()
    raise ValueError(fault)
