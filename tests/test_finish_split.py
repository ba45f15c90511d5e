"""CPU tests of the host side of the k-split finishes with a tail (csrc/wc_conv.hip: wc_conv_tail_supported, wc_conv_tail_f16x3,
wc_conv_bwd_pair_tail_f16x3; csrc/wc_gp.hip: wc_conv_split_redo_masked_f32): which geometries take a tail, what the entries refuse, and what
conv.py decides from shapes and records alone -- no kernel is launched (every refusal comes before anything is dereferenced)."""
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


def _geoms(kind, N, H, W, ci, co, k):
    from wc_gan_amd import conv as C
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, _W(co, ci, k, k))
    return gf, gd


ONE = ctypes.c_void_p(16)
BIG = 1 << 30


def _tail(kind, **fields):
    from wc_gan_amd import _lib
    t = _lib.ConvTail()
    t.kind = kind
    for k in ('res', 'mask', 'other', 'out', 'hi', 'lo', 'scale', 'hist', 'colsum_partials'):
        setattr(t, k, fields.get(k, 16))
    t.C = fields.get('C', 128)
    t.redo = fields.get('redo', 0)
    return t


# the CIFAR critic at batch 128: (layer, kind, H, the forward finish takes a tail, the data gradient's finish takes one)
CRITIC = [('2.conv1', 'same', 8, True, True), ('2.conv2', 'same', 8, True, True), ('1.conv2', 'down3', 16, True, False),
          ('1.conv1', 'same', 16, False, False)]


@pytest.mark.parametrize("layer", CRITIC, ids=lambda c: c[0])
def test_a_tail_goes_where_the_tap_loop_is_shared(lib, layer):
    _, kind, H, fwd, bwd = layer
    gf, gd = _geoms(kind, 128, H, H, 128, 128, 3)
    for g, want in ((gf, fwd), (gd, bwd)):
        p = ctypes.addressof(g)
        assert lib.wc_conv_tail_supported(p) == (1 if want else 0)
        assert bool(lib.wc_conv_tail_supported(p)) == (lib.wc_conv_workspace_bytes(p) > 0 and lib.wc_conv_res_supported(p) == 1)
    assert lib.wc_conv_tail_supported(None) == 0


def test_the_plan_records_both_tails():
    from wc_gan_amd import conv as C
    for kind, shape, fwd, bwd in (('same', (128, 8, 8, 128), True, True), ('down3', (128, 16, 16, 128), True, False),
                                  ('same', (128, 16, 16, 128), False, False), ('same', (2, 8, 8, 128), True, True)):
        p = C._plan(kind, C._Shape(shape), C._Shape((128, 128, 3, 3)))
        assert p and p.ok and p.tail is fwd and p.bwd_tail is bwd, (kind, shape)


def test_the_forward_entry_checks_its_arguments(lib):
    from wc_gan_amd import _lib
    gf, _ = _geoms('same', 128, 8, 8, 128, 128, 3)
    pf = ctypes.addressof(gf)
    ws = lib.wc_conv_workspace_bytes(pf)
    assert ws > 0

    def call(tail, xhi=ONE, wimage=ONE, y=ONE, work=ONE, nbytes=BIG, g=pf):
        return lib.wc_conv_tail_f16x3(xhi, ONE, ONE, wimage, ONE, None, ONE, g, y, work, nbytes, ctypes.addressof(tail) if tail else None, None)
    split = _tail(_lib.TAIL_SPLIT)
    assert call(None) == -1
    assert call(split, xhi=None) == -5 and call(split, wimage=None) == -5 and call(split, y=None) == -5 and call(split, g=None) == -5
    assert call(split, nbytes=ws - 1) == -4 and call(split, work=None) == -4
    for missing in ('hi', 'lo', 'scale', 'hist'):
        assert call(_tail(_lib.TAIL_SPLIT, **{missing: None})) == -1, missing
        assert call(_tail(_lib.TAIL_MASKED, **{missing: None})) == -1, missing
    assert call(_tail(_lib.TAIL_MASKED, mask=None)) == -1
    assert call(_tail(_lib.TAIL_MASKED, C=64)) == -2 and call(_tail(_lib.TAIL_MASKED, C=0)) == -2      # the partial rows are Cout wide
    for missing in ('mask', 'other', 'out'):
        assert call(_tail(_lib.TAIL_DX, **{missing: None}), y=None) == -1, missing
    assert call(_tail(_lib.TAIL_DX, out=16, mask=16, other=32), y=None) == -5                          # out aliases the mask
    assert call(_tail(0)) == -5 and call(_tail(4)) == -5
    # a geometry without a shared tap loop: there is no finish launch to give a tail to
    g16, _ = _geoms('same', 128, 16, 16, 128, 128, 3)
    assert lib.wc_conv_workspace_bytes(ctypes.addressof(g16)) == 0
    assert call(split, g=ctypes.addressof(g16), work=None, nbytes=0) == -2
    # a width the finish's 128-wide tiles do not take
    g64, _ = _geoms('down', 128, 8, 8, 128, 64, 4)
    assert call(split, g=ctypes.addressof(g64)) == -2


def test_the_pair_entry_checks_its_tail(lib):
    from wc_gan_amd import _lib
    gf, gd = _geoms('same', 128, 8, 8, 128, 128, 3)
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)

    def call(tail, dx=ONE, gd_=pd, gf_=pf, ws_dx=ONE, ws_dx_bytes=BIG, dw=ONE):
        return lib.wc_conv_bwd_pair_tail_f16x3(ONE, ONE, ONE, ONE, ONE, ONE, gd_, dx, ws_dx, ws_dx_bytes,
                                               ONE, ONE, ONE, gf_, dw, 1, 128, 3 * 128 * 128, 128 * 128, None, None, ONE, BIG,
                                               ctypes.addressof(tail) if tail else None, None)
    masked, dx = _tail(_lib.TAIL_MASKED), _tail(_lib.TAIL_DX, out=48, other=32)
    assert call(None) == -1
    assert call(_tail(_lib.TAIL_SPLIT)) == -5                   # the forward's tail: not behind a data gradient
    assert call(masked, dx=None) == -5                          # MASKED writes the data gradient in fp32 as well
    assert call(_tail(_lib.TAIL_MASKED, mask=None)) == -1 and call(_tail(_lib.TAIL_DX, out=None)) == -1
    assert call(masked, dw=None) == -1                          # the weight gradient's own checks still run
    assert call(masked, ws_dx_bytes=8) == -4
    # the 16x16 layers' data gradient finishes in the tiles' epilogue: no tail, whatever the pair predicate says
    gf16, gd16 = _geoms('same', 128, 16, 16, 128, 128, 3)
    assert lib.wc_conv_bwd_pair_supported(ctypes.addressof(gd16), ctypes.addressof(gf16)) == 1
    for t in (masked, dx):
        assert call(t, gd_=ctypes.addressof(gd16), gf_=ctypes.addressof(gf16), ws_dx=None, ws_dx_bytes=0) == -2


def test_the_gated_pass_alone_checks_its_arguments(lib):
    def call(t=ONE, a=ONE, n=1024, slope=0.0, hi=ONE, lo=ONE, scale=ONE, hist=ONE):
        return lib.wc_conv_split_redo_masked_f32(t, a, n, slope, hi, lo, scale, hist, None)
    for k in ('t', 'a', 'hi', 'lo', 'scale', 'hist'):
        assert call(**{k: None}) == -5, k
    assert call(n=0) == -5 and call(n=1022) == -5 and call(slope=1.5) == -5 and call(slope=-0.1) == -5


def test_the_readers_record_is_used_only_when_seeded_and_in_training_mode():
    import torch
    from wc_gan_amd import conv as C

    class Site:
        training = True
    s = Site()
    cpu = torch.device('cpu')
    assert C._reader_record(None, 'x', cpu) is None
    assert C._reader_record(s, 'x', cpu) is None and '_wc_split_hist' not in s.__dict__        # never creates a record
    rec = [torch.zeros(C.HIST_FLOATS), False]
    s._wc_split_hist = {'x': rec}
    assert C._reader_record(s, 'x', cpu) is None                # there, not seeded: the first call measures
    rec[1] = True
    assert C._reader_record(s, 'x', cpu) is rec and C._reader_record(s, 'g', cpu) is None
    assert C._reader_record(s, 'x', torch.device('meta')) is None                              # the layer moved
    s.training = False
    assert C._reader_record(s, 'x', cpu) is None                # eval mode measures every tensor
    s.training = True
    old, C.SPLIT_HIST = C.SPLIT_HIST, False
    try:
        assert C._reader_record(s, 'x', cpu) is None
    finally:
        C.SPLIT_HIST = old


def test_the_flags_default_to_on():
    from wc_gan_amd import conv as C
    assert C.FUSED_FINISH is True and C.FUSED_FINISH_F1 and C.FUSED_FINISH_F2 and C.FUSED_FINISH_B1 and C.FUSED_FINISH_B2
