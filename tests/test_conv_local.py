"""CPU tests of the host side of the k-split summed inside the workgroup (csrc/wc_conv.hip: wc_conv_local_supported, wc_conv_local_f16x3):
which geometries the predicate takes, what the entry refuses, and what conv.py records -- no kernel is launched (every refusal comes
before anything is dereferenced; without a device the predicate counts gfx950's 256 CUs)."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


class _W:
    def __init__(self, *shape):
        self.shape = shape


def _geoms(kind, N, H, W, ci, co, k=3):
    from wc_gan_amd import conv as C
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, _W(co, ci, k, k))
    return gf, gd


ONE = ctypes.c_void_p(16)

# kind, (N, H, W), Cin, Cout, taken, why
TABLE = [
    ('same', (128, 8, 8), 128, 128, True, "the critic's SAME blocks: k-split 4, 256 tiles of 64 x 64"),
    ('down3', (128, 16, 16), 128, 128, True, "the DOWN block's conv2: 16 taps, 64 iterations, 16 per share"),
    ('same', (256, 4, 8), 128, 128, True, "two images per tile, H != W"),
    ('same', (32, 16, 16), 128, 128, True, "a quarter image per tile"),
    ('same', (128, 8, 8), 192, 128, True, "54 iterations: shares of 13, 14, 13, 14 that start mid-tap"),
    ('same', (4, 8, 8), 128, 128, False, "batch 4: k-split 8"),
    ('same', (72, 8, 8), 128, 128, False, "36 tiles: k-split 8"),
    ('same', (128, 8, 8), 128, 256, False, "Cout 256: the 256-wide tiles' k-split"),
    ('same', (129, 8, 8), 128, 128, False, "a ragged grid: 8256 points are no whole tiles"),
    ('same', (168, 8, 8), 128, 128, False, "M = 10752: k-split 4, but a grid of 336 exceeds the CUs"),
    ('same', (128, 8, 8), 160, 128, False, "Cin is no multiple of 64"),
    ('same', (128, 16, 16), 128, 128, False, "no k-split at all"),
]


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"{r[0]}-{'x'.join(map(str, r[1]))}-{r[2]}-{r[3]}")
def test_the_predicate_takes_four_shares_on_whole_tiles_that_fit_the_chip(lib, row):
    kind, (N, H, W), ci, co, want, why = row
    gf, _ = _geoms(kind, N, H, W, ci, co)
    p = ctypes.addressof(gf)
    assert lib.wc_conv_local_supported(p) == (1 if want else 0), why
    if want:
        # a taken geometry is one the two-launch entries take with FOUR shares: their workspace is 4 outputs, their predicates say yes
        out_bytes = gf.N * gf.Hout * gf.Wout * gf.Cout * 4
        assert lib.wc_conv_workspace_bytes(p) == 4 * out_bytes and lib.wc_conv_res_supported(p) == 1 and lib.wc_conv_tail_supported(p) == 1
        assert (gf.N * gf.H * gf.W // 64) * gf.nphase * (gf.Cout // 64) <= 256


def test_the_refused_rows_are_refused_for_the_reason_they_name(lib):
    ws = lambda g: lib.wc_conv_workspace_bytes(ctypes.addressof(g))
    out = lambda g: g.N * g.Hout * g.Wout * g.Cout * 4
    g4, _ = _geoms('same', 4, 8, 8, 128, 128)
    g72, _ = _geoms('same', 72, 8, 8, 128, 128)
    assert ws(g4) == 8 * out(g4) and ws(g72) == 8 * out(g72)
    big, _ = _geoms('same', 168, 8, 8, 128, 128)
    assert ws(big) == 4 * out(big) and lib.wc_conv_supported(ctypes.addressof(big)) == 1       # four shares, whole tiles: only the grid is too large
    ragged, _ = _geoms('same', 129, 8, 8, 128, 128)
    assert lib.wc_conv_supported(ctypes.addressof(ragged)) == 0 and lib.wc_conv_ragged_supported(ctypes.addressof(ragged)) == 1
    assert lib.wc_conv_local_supported(None) == 0


def test_the_data_gradient_geometries(lib):
    _, gd = _geoms('same', 128, 8, 8, 128, 128)
    assert lib.wc_conv_local_supported(ctypes.addressof(gd)) == 1
    _, gd = _geoms('down3', 128, 16, 16, 128, 128)              # four phases at 8x8: 256 tiles of 128 points, no k-split
    assert lib.wc_conv_local_supported(ctypes.addressof(gd)) == 0


def test_the_plan_records_both_directions():
    from wc_gan_amd import conv as C
    for kind, shape, fwd, bwd in (('same', (128, 8, 8, 128), True, True), ('down3', (128, 16, 16, 128), True, False),
                                  ('same', (128, 16, 16, 128), False, False), ('same', (2, 8, 8, 128), False, False)):
        p = C._plan(kind, C._Shape(shape), C._Shape((128, 128, 3, 3)))
        assert p and p.ok and p.local is fwd and p.bwd_local is bwd, (kind, shape)
    assert C.LOCAL_KSPLIT in (True, False)


def _tail(kind, **fields):
    from wc_gan_amd import _lib
    t = _lib.ConvTail()
    t.kind = kind
    for k in ('res', 'mask', 'other', 'out', 'hi', 'lo', 'scale', 'hist'):
        setattr(t, k, fields.get(k, 16))
    t.colsum_partials = fields.get('colsum_partials', None)
    t.C = fields.get('C', 128)
    t.redo = fields.get('redo', 0)
    return t


def test_the_entry_checks_its_arguments(lib):
    from wc_gan_amd import _lib
    gf, _ = _geoms('same', 128, 8, 8, 128, 128)
    pf = ctypes.addressof(gf)

    def call(tail=None, xhi=ONE, wimage=ONE, y=ONE, g=pf, res=None, relu=0, zero=ONE):
        return lib.wc_conv_local_f16x3(xhi, ONE, ONE, wimage, ONE, None, res, zero, g, relu, y, ctypes.addressof(tail) if tail else None, None)
    assert call(xhi=None) == -5 and call(wimage=None) == -5 and call(y=None) == -5 and call(g=None) == -5 and call(zero=None) == -5
    assert call(res=ONE, relu=1) == -5                          # no ReLU behind a residual
    split = _tail(_lib.TAIL_SPLIT)
    assert call(split, res=ONE) == -5 and call(split, relu=1) == -5        # a tail brings its own residual, and has no ReLU in front
    for missing in ('hi', 'lo', 'scale', 'hist'):
        assert call(_tail(_lib.TAIL_SPLIT, **{missing: None})) == -1, missing
        assert call(_tail(_lib.TAIL_MASKED, **{missing: None})) == -1, missing
    assert call(_tail(_lib.TAIL_MASKED, mask=None)) == -1
    assert call(_tail(_lib.TAIL_MASKED, colsum_partials=16)) == -2         # the partial rows belong to the 512-workgroup finish
    assert call(_tail(_lib.TAIL_MASKED, colsum_partials=16, C=64)) == -2
    for missing in ('mask', 'other', 'out'):
        assert call(_tail(_lib.TAIL_DX, **{missing: None}), y=None) == -1, missing
    assert call(_tail(_lib.TAIL_DX, out=16, mask=16, other=32), y=None) == -5     # out aliases the mask
    assert call(_tail(0)) == -5 and call(_tail(4)) == -5
    # every geometry the predicate refuses: WC_ERR_SHAPE, with and without a tail
    for kind, (N, H, W), ci, co, want, why in TABLE:
        if not want:
            g, _ = _geoms(kind, N, H, W, ci, co)
            assert call(g=ctypes.addressof(g)) == -2, why
            assert call(split, g=ctypes.addressof(g)) == -2, why
