"""Host-side tests of the critic blocks' glue entries: argument checks of the new and extended C-ABI entries -- every
call below is rejected before a kernel is launched -- and the shapes the fused block takes."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


ONE = ctypes.c_void_p(16)       # never dereferenced


def _geom(kind, N, H, W, cin=128, cout=128, k=3):
    from wc_gan_amd import conv as C
    p = C._Plan(kind, N, H, W, (cout, cin, k, k))
    return p


def test_masked_split_entries_check_the_column_sum_arguments(lib):
    n = 2 * 8 * 8 * 128
    for C_bad in (0, 130, 24, 384):         # not a multiple of 4, or C / 4 does not divide 256 (conv._colsum_ok), or n % C != 0
        assert lib.wc_conv_split_hist_masked_f32(ONE, ONE, n, 0.0, ONE, ONE, ONE, ONE, C_bad, ONE, 0, None) == -2, C_bad
        assert lib.wc_conv_split_masked_f32(ONE, ONE, n, 0.0, ONE, ONE, ONE, ONE, ONE, C_bad, None) == -2, C_bad
    from wc_gan_amd import conv as C
    assert not C._colsum_ok(130) and not C._colsum_ok(24) and not C._colsum_ok(384) and C._colsum_ok(128) and C._colsum_ok(64)
    assert lib.wc_conv_split_hist_masked_f32(ONE, ONE, 4 * 97, 0.0, ONE, ONE, ONE, ONE, 128, ONE, 0, None) == -2     # n is no multiple of C
    # the checks that were there: pointers, the slope's range, n % 4
    assert lib.wc_conv_split_hist_masked_f32(None, ONE, n, 0.0, ONE, ONE, ONE, None, 0, ONE, 0, None) == -5
    assert lib.wc_conv_split_hist_masked_f32(ONE, None, n, 0.0, ONE, ONE, ONE, None, 0, ONE, 0, None) == -5
    assert lib.wc_conv_split_hist_masked_f32(ONE, ONE, n, 0.0, ONE, ONE, ONE, None, 0, None, 0, None) == -5
    assert lib.wc_conv_split_hist_masked_f32(ONE, ONE, n, 1.5, ONE, ONE, ONE, None, 0, ONE, 0, None) == -5
    assert lib.wc_conv_split_hist_masked_f32(ONE, ONE, n + 2, 0.0, ONE, ONE, ONE, None, 0, ONE, 0, None) == -5
    assert lib.wc_conv_split_masked_f32(ONE, ONE, n, 0.0, ONE, ONE, ONE, None, None, 0, None) == -5


def test_residual_entry_checks_its_arguments(lib):
    ks = _geom('same', 2, 8, 8)             # the k-split finish
    direct = _geom('same', 256, 8, 8)       # 128 output tiles: the tiles' own epilogue
    wide = _geom('same', 2, 8, 8, 256, 256)
    narrow = _geom('down', 2, 8, 8, 64, 64, 4)
    assert ks.ok and direct.ok and wide.ok
    assert lib.wc_conv_res_supported(ks.fwd_ptr) == 1 and lib.wc_conv_workspace_bytes(ks.fwd_ptr) > 0
    assert lib.wc_conv_res_supported(direct.fwd_ptr) == 0 and lib.wc_conv_workspace_bytes(direct.fwd_ptr) == 0
    assert lib.wc_conv_res_supported(wide.fwd_ptr) == 1
    assert lib.wc_conv_res_supported(narrow.fwd_ptr) == 0 and lib.wc_conv_res_supported(None) == 0
    assert (ks.res, direct.res, wide.res) == (True, False, True)
    big = 1 << 30
    args = lambda g, res=ONE, ws=ONE, nbytes=big, y=ONE: (ONE, ONE, ONE, ONE, ONE, None, res, ONE, g, y, ws, nbytes, None)
    assert lib.wc_conv_res_f16x3(*args(ks.fwd_ptr, res=None)) == -5
    assert lib.wc_conv_res_f16x3(*args(ks.fwd_ptr, y=None)) == -5
    assert lib.wc_conv_res_f16x3(*args(None)) == -5
    assert lib.wc_conv_res_f16x3(*args(direct.fwd_ptr)) == -2           # no shared tap loop: the caller adds
    assert lib.wc_conv_res_f16x3(*args(narrow.fwd_ptr)) == -2
    assert lib.wc_conv_res_f16x3(*args(ks.fwd_ptr, ws=None, nbytes=0)) == -4
    assert lib.wc_conv_res_f16x3(*args(ks.fwd_ptr, nbytes=16)) == -4


def test_block_input_gradient_entry_checks_its_arguments(lib):
    f = lib.wc_conv_block_dx_f32
    assert f(None, ONE, ONE, 2, 8, 8, 128, 0, ONE, None) == -1
    assert f(ONE, None, ONE, 2, 8, 8, 128, 0, ONE, None) == -1
    assert f(ONE, ONE, None, 2, 8, 8, 128, 1, ONE, None) == -1
    assert f(ONE, ONE, ONE, 2, 8, 8, 128, 0, None, None) == -1
    assert f(ONE, ONE, ONE, 0, 8, 8, 128, 0, ONE, None) == -2
    assert f(ONE, ONE, ONE, 2, 8, 8, 130, 0, ONE, None) == -2           # float4 per lane
    assert f(ONE, ONE, ONE, 2, 7, 8, 128, 1, ONE, None) == -2           # the pooled form halves the grid
    assert f(ONE, ONE, ONE, 2, 8, 7, 128, 1, ONE, None) == -2


def test_the_shapes_the_fused_block_takes():
    from wc_gan_amd import conv as C
    w3, w1 = (128, 128, 3, 3), (128, 128, 1, 1)
    # the CIFAR-10 and STL-10 critics' blocks behind the first, at the step's batch and at the tests'
    for shape, ws, down in (((128, 16, 16, 128), w1, True), ((128, 8, 8, 128), None, False), ((128, 24, 24, 128), w1, True),
                            ((128, 12, 12, 128), None, False), ((4, 16, 16, 128), w1, True), ((2, 8, 8, 128), None, False)):
        plans = C.critic_block_plans(shape, w3, w3, ws, down)
        assert plans is not None and (plans[2] is None) == (ws is None), shape
        # conv2 finishes through the k-split reduction, which takes the residual, up to 96 output tiles: 128 x 12 x 12 has 144
        assert plans[1].res == (shape[1] not in (24, 12)), shape
    assert C.critic_block_plans((128, 16, 16, 256), (256, 256, 3, 3), (256, 256, 3, 3), (256, 256, 1, 1), True) is not None
    # what falls through to the separate nodes
    assert C.critic_block_plans((128, 16, 16, 64), (64, 64, 3, 3), (64, 64, 3, 3), (64, 64, 1, 1), True) is None      # 64-wide toy blocks
    assert C.critic_block_plans((128, 16, 16, 384), (384, 384, 3, 3), (384, 384, 3, 3), None, False) is None          # 96 does not divide 256
    assert C.critic_block_plans((1, 8, 8, 128), w3, w3, None, False) is None                                           # 64 grid points: no tile
    assert C.critic_block_plans((128, 15, 15, 128), w3, w3, w1, True) is None                                          # an odd grid cannot halve
    assert C.critic_block_plans((128, 8, 8, 128), w3, w3, None, True) is None                                          # DOWN has a shortcut
    assert C.critic_block_plans((128, 8, 8, 128), w3, (256, 128, 3, 3), None, False) is None                           # widths differ: no identity
    assert C.critic_block_plans((128, 8, 8, 128), (128, 128, 1, 1), w3, None, False) is None                           # conv1 is 3x3
    assert C.critic_block_plans((128, 8, 8, 128), w3, w3, (128, 128, 3, 3), False) is None                             # the shortcut is 1x1
    assert C.critic_block_plans((128, 8, 128), w3, w3, None, False) is None


def test_the_block_falls_through_off_the_fused_route():
    import torch
    from functools import partial
    from wc_gan_amd import conv as C
    from wc_gan_amd import generator as G
    from wc_gan_amd.discriminator import ResBlockDown
    conv_layer = partial(G.Conv2D, spectral=False)
    make = lambda norm=('n', 'n'), first=False, conv=conv_layer: ResBlockDown(128, 128, 'SAME', 'D.2', G.create_norm(*norm), conv, is_first=first)
    blk = make()
    assert C.FUSED_BLOCK is True and C.FUSED_MASKED_SPLIT and C.FUSED_RESIDUAL and C.FUSED_BLOCK_DX
    # the module's own part of the predicate (ResBlockDown._fusable, what _fused_plans asks first)
    assert blk._fusable()
    assert not make(first=True)._fusable()                                      # block 0 reads images
    assert not make(norm=('b', 'ucs'))._fusable()                               # a norm at the sites
    assert not make(norm=('n', 'ucs'))._fusable()                               # no normalisation, but coloring branches
    assert not make(conv=partial(G.Conv2D, spectral=False)).double()._fusable() # fp64 weights
    for name, mod in (('FUSED_BLOCK', C), ('FAST_CONV', G)):                    # either switch off
        old = getattr(mod, name)
        setattr(mod, name, False)
        try:
            assert not blk._fusable()
        finally:
            setattr(mod, name, old)
    assert blk._fusable()
    # the input's part: a CPU tensor, a non-fp32 tensor, a 3-d tensor never reach the node
    x = torch.zeros(2, 8, 8, 128)
    assert blk._fused_plans(x) is None and blk._fused_plans(x.double()) is None and blk._fused_plans(x[0]) is None
    y = blk(x, None)                                                            # the present code, on the CPU
    assert y.shape == (2, 8, 8, 128)
