"""CPU tests of the pair entry's host side (csrc/wc_conv.hip: wc_conv_bwd_pair_supported / _workspace_bytes / _f16x3): which layers take
the one-grid backward, what it asks for as workspace, and what it refuses -- no kernel is launched (the library loads without a device)."""
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
    """(forward geometry, data-gradient geometry) of conv.py's layer `kind` on an (N, H, W, ci) input"""
    from wc_gan_amd import conv as C
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, _W(co, ci, k, k))
    return gf, gd


# the CIFAR critic at batch 128 (discriminator.py: blocks 1-3 behind the image block), 128 -> 128
CRITIC = [
    ('2.conv1', 'same', 8, 8, 3), ('2.conv2', 'same', 8, 8, 3), ('3.conv1', 'same', 8, 8, 3), ('3.conv2', 'same', 8, 8, 3),
    ('1.conv1', 'same', 16, 16, 3), ('1.conv2', 'down3', 16, 16, 3), ('1.shortcut', 'same', 8, 8, 1),
]


@pytest.mark.parametrize("layer", CRITIC, ids=lambda c: c[0])
def test_the_critics_128_channel_layers_take_the_pair(lib, layer):
    _, kind, H, W, k = layer
    gf, gd = _geoms(kind, 128, H, W, 128, 128, k)
    assert lib.wc_conv_bwd_pair_supported(ctypes.addressof(gd), ctypes.addressof(gf)) == 1


OTHERS = [
    ('a 64-channel input side', 'down', 128, 16, 16, 64, 128, 4),
    ('a 64-channel output side', 'down', 128, 16, 16, 128, 64, 4),
    ('256 -> 256: the wide weight-gradient tile', 'same', 128, 8, 8, 256, 256, 3),
    ('a data gradient on <4,2>', 'same', 64, 32, 32, 128, 128, 3),
    ('an up-sampling layer', 'up3', 128, 8, 8, 128, 128, 3),
    ("'up' with the 4x4 weight", 'up', 128, 8, 8, 128, 128, 4),
]


@pytest.mark.parametrize("layer", OTHERS, ids=lambda c: c[0])
def test_everything_else_stays_on_the_two_entries(lib, layer):
    _, kind, N, H, W, ci, co, k = layer
    from wc_gan_amd import conv as C
    w = _W(ci, co, k, k) if kind == 'up' else _W(co, ci, k, k)
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, w)
    assert lib.wc_conv_supported(ctypes.addressof(gf)) == 1 and lib.wc_conv_supported(ctypes.addressof(gd)) == 1
    assert lib.wc_conv_bwd_pair_supported(ctypes.addressof(gd), ctypes.addressof(gf)) == 0


def test_the_predicate_wants_the_two_geometries_of_one_layer(lib):
    gf, gd = _geoms('same', 128, 8, 8, 128, 128, 3)
    gf16, gd16 = _geoms('same', 128, 16, 16, 128, 128, 3)
    assert lib.wc_conv_bwd_pair_supported(None, ctypes.addressof(gf)) == 0 and lib.wc_conv_bwd_pair_supported(ctypes.addressof(gd), None) == 0
    assert lib.wc_conv_bwd_pair_supported(ctypes.addressof(gd16), ctypes.addressof(gf)) == 0


def test_the_sizer_is_the_sum_of_the_two_sizers(lib):
    seen_ksplit = seen_plain = False
    for _, kind, H, W, k in CRITIC:
        gf, gd = _geoms(kind, 128, H, W, 128, 128, k)
        dx_ws, dw_ws = lib.wc_conv_workspace_bytes(ctypes.addressof(gd)), lib.wc_conv_wrw_workspace_bytes(ctypes.addressof(gf))
        assert dw_ws > 0
        assert lib.wc_conv_bwd_pair_workspace_bytes(ctypes.addressof(gd), ctypes.addressof(gf)) == dx_ws + dw_ws
        seen_ksplit |= dx_ws > 0
        seen_plain |= dx_ws == 0
    assert seen_ksplit and seen_plain           # the 8x8 'same' layers k-split their data gradient, the others do not
    assert lib.wc_conv_bwd_pair_workspace_bytes(None, None) == 0


def test_the_entry_returns_the_two_entries_codes(lib):
    """null pointers: wc_conv_f16x3's WC_ERR_ARG for the data gradient's operands, wc_conv_wrw_bias_f16x3's WC_ERR_NULL for the weight
    gradient's; a short workspace: WC_ERR_WORKSPACE from either; a layer outside the predicate: WC_ERR_SHAPE.  Every call is rejected
    before anything is dereferenced or launched."""
    one = ctypes.c_void_p(16)
    big = 1 << 30
    gf, gd = _geoms('same', 128, 8, 8, 128, 128, 3)          # k-split data gradient: both workspaces are needed
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)
    dx_ws, dw_ws = lib.wc_conv_workspace_bytes(pd), lib.wc_conv_wrw_workspace_bytes(pf)
    assert dx_ws > 0 and dw_ws > 0

    def call(ghi=one, wimage=one, dx=one, ws_dx=one, ws_dx_bytes=big, xhi=one, dw=one, colsum=None, db=None, ws_dw=one, ws_dw_bytes=big,
             gd_=pd, gf_=pf):
        return lib.wc_conv_bwd_pair_f16x3(ghi, one, one, wimage, one, one, gd_, dx, ws_dx, ws_dx_bytes,
                                          xhi, one, one, gf_, dw, 1, 128, 3 * 128 * 128, 128 * 128, colsum, db, ws_dw, ws_dw_bytes, None)
    assert call(ghi=None) == -5 and call(wimage=None) == -5 and call(dx=None) == -5 and call(gd_=None) == -5
    assert call(xhi=None) == -1 and call(dw=None) == -1 and call(ws_dw=None) == -1 and call(gf_=None) == -1
    assert call(colsum=one) == -1 and call(db=one) == -1                    # the bias gradient's operands: both or neither
    assert call(ws_dx_bytes=dx_ws - 1) == -4 and call(ws_dx=None) == -4
    assert call(ws_dw_bytes=dw_ws - 1) == -4
    gf2, gd2 = _geoms('same', 128, 8, 8, 256, 256, 3)
    assert call(gd_=ctypes.addressof(gd2), gf_=ctypes.addressof(gf2)) == -2
    gf3, gd3 = _geoms('up3', 128, 8, 8, 128, 128, 3)
    assert call(gd_=ctypes.addressof(gd3), gf_=ctypes.addressof(gf3)) == -2


def test_the_plan_records_the_pair():
    from wc_gan_amd import conv as C

    class _X:
        pass
    for kind, shape, wshape, want in (('same', (128, 8, 8, 128), (128, 128, 3, 3), True), ('down3', (128, 16, 16, 128), (128, 128, 3, 3), True),
                                      ('up3', (128, 8, 8, 128), (128, 128, 3, 3), False), ('same', (128, 8, 8, 256), (256, 256, 3, 3), False)):
        x, w = _X(), _X()
        x.shape, w.shape = shape, wshape
        p = C._plan(kind, x, w)
        assert p and p.ok and p.pair is want, (kind, shape)
