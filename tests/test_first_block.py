"""CPU tests of the host side of the critic's first block on the HIP route (csrc/wc_conv.hip: wc_conv_fwd_narrow_split_supported,
wc_conv_fwd_narrow_split_f32, wc_conv_wrw_narrow_masked_f32; conv.first_block_route, discriminator.ResBlockDown._first_plan_of): which
shapes the split variant of the narrow forward takes, what the entries refuse, and what the route decides from shapes, records and
switches alone -- no kernel is launched (every refusal comes before anything is dereferenced)."""
import ctypes
import os
from functools import partial

import pytest


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


ONE = ctypes.c_void_p(16)
BIG = 1 << 30


def _grid(N, H, W, cout):
    """workgroups of the narrow forward: 4 waves of tiles_per_wave 32-pixel tiles each, one column per 64 output channels"""
    ntiles = (N * H * W + 31) // 32
    tpw = max(1, (ntiles + 1023) // 1024)
    return ((ntiles + 4 * tpw - 1) // (4 * tpw)) * (cout // 64)


# (N, H, W, Cin, Cout, k): the CIFAR critic's block 0 fills the record exactly; the GPU tests' shapes; the largest grids on either side of 512
TAKEN = [(128, 32, 32, 3, 128, 3), (2, 5, 5, 3, 64, 3), (3, 8, 8, 3, 128, 3), (2, 12, 12, 3, 128, 3), (2, 5, 5, 1, 64, 3), (3, 8, 8, 3, 64, 1),
         (9, 64, 64, 3, 128, 3), (64, 32, 32, 3, 128, 3), (32, 32, 32, 3, 128, 3), (512, 32, 32, 3, 128, 3)]
REFUSED = [(32, 32, 32, 3, 192, 3), (128, 32, 32, 3, 192, 3), (128, 32, 32, 3, 256, 3)]


def test_the_split_variant_takes_grids_of_at_most_512_workgroups(lib):
    for c in TAKEN:
        N, H, W, ci, co, k = c
        assert _grid(N, H, W, co) <= 512 and lib.wc_conv_fwd_narrow_split_supported(*c) == 1, c
    for c in REFUSED:
        N, H, W, ci, co, k = c
        assert _grid(N, H, W, co) > 512 and lib.wc_conv_narrow64_supported(*c) == 1 and lib.wc_conv_fwd_narrow_split_supported(*c) == 0, c
    assert _grid(32, 32, 32, 192) == 768 and _grid(128, 32, 32, 128) == 512
    # never more than the plain entry takes
    for c in ((2, 8, 8, 4, 128, 3), (2, 8, 8, 3, 96, 3), (2, 8, 8, 3, 128, 5), (0, 8, 8, 3, 128, 3)):
        assert lib.wc_conv_narrow64_supported(*c) == 0 and lib.wc_conv_fwd_narrow_split_supported(*c) == 0, c


def test_the_forward_entry_checks_its_arguments(lib):
    def call(x=ONE, w=ONE, y=ONE, hi=ONE, lo=ONE, scale=ONE, hist=ONE, relu=1, flags=0, shape=(3, 8, 8, 3, 128, 3)):
        N, H, W, ci, co, k = shape
        return lib.wc_conv_fwd_narrow_split_f32(x, w, 1, 27, 9, 3, None, N, H, W, ci, co, k, relu, 0.0, y, hi, lo, scale, hist, flags, None)
    for missing in ('x', 'w', 'y', 'hi', 'lo', 'scale', 'hist'):
        assert call(**{missing: None}) == -5, missing
    assert call(relu=3) == -5 and call(relu=-1) == -5
    assert call(flags=1) == -5 and call(flags=8) == -5          # (1: split_hist's seeding call -- the record here is already seeded)
    # G = 768 workgroups: refused with WC_ERR_SHAPE before anything is dereferenced -- the caller runs the two launches
    assert call(shape=(32, 32, 32, 3, 192, 3)) == -2
    assert call(shape=(2, 8, 8, 4, 128, 3)) == -2


def test_the_masked_weight_gradient_checks_its_arguments(lib):
    shape = (3, 8, 8, 3, 128, 3)
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(*shape)
    assert nb > 0

    def call(x=ONE, gy=ONE, mask=ONE, dw=ONE, ws=ONE, nbytes=BIG, shape=shape):
        N, H, W, ci, co, k = shape
        return lib.wc_conv_wrw_narrow_masked_f32(x, gy, mask, N, H, W, ci, co, k, dw, 1, 27, 9, 3, None, ws, nbytes, None)
    for missing in ('x', 'gy', 'mask', 'dw', 'ws'):
        assert call(**{missing: None}) == -5, missing
    assert call(nbytes=nb - 1) == -4
    assert call(shape=(2, 8, 8, 4, 128, 3)) == -2


def test_the_route_falls_back_on_shapes_records_and_its_switch():
    from wc_gan_amd import conv as C
    rec = [None, True]              # (first_block_route only asks whether _reader_record gave one)
    cifar, wide = ((128, 32, 32, 3), (128, 3, 3, 3)), ((32, 32, 32, 3), (192, 3, 3, 3))
    assert C.narrow_split_supported(*cifar) and not C.narrow_split_supported(*wide)
    assert C.narrow_shapes_supported(*wide)                     # the narrow kernels themselves take it: the two launches run
    assert C.first_block_route(*cifar, rec) == 'planes'
    assert C.first_block_route(*wide, rec) == 'two'             # G = 768
    assert C.first_block_route(*cifar, None) == 'two'           # the first call, eval mode, a capture that meets an unseeded site
    old, C.FIRST_BLOCK_PLANES = C.FIRST_BLOCK_PLANES, False
    try:
        assert C.first_block_route(*cifar, rec) == 'two'
    finally:
        C.FIRST_BLOCK_PLANES = old


def _block(in_ch=3, resample='DOWN', is_first=True, norm='n'):
    from wc_gan_amd.discriminator import ResBlockDown
    from wc_gan_amd.generator import Conv2D, create_norm
    return ResBlockDown(in_ch, 128, resample, 'D.0', create_norm(norm, 'n'), partial(Conv2D), is_first=is_first)


def test_the_flags_default_to_on_and_are_independent_of_the_other_blocks_switches():
    from wc_gan_amd import conv as C
    assert C.FIRST_BLOCK is True and C.FIRST_BLOCK_PLANES is True and C.FIRST_BLOCK_MASK is True
    blk = _block()
    shape = (128, 32, 32, 3)
    assert blk._first_plan_of(shape) is not None and not blk._fusable()
    flags = ('FUSED_BLOCK', 'FUSED_FINISH', 'FUSED_FINISH_F1', 'FUSED_MASKED_SPLIT', 'FUSED_RESIDUAL', 'FUSED_BLOCK_DX')
    old = {k: getattr(C, k) for k in flags}
    try:
        for k in flags:
            setattr(C, k, False)
        assert C.FIRST_BLOCK and C.FIRST_BLOCK_PLANES and C.FIRST_BLOCK_MASK
        assert blk._first_plan_of(shape) is not None
        assert C.first_block_route(shape, (128, 3, 3, 3), [None, True]) == 'planes'
    finally:
        for k, v in old.items():
            setattr(C, k, v)
    # ... and the other way round: the blocks behind the first keep their route when this one is off
    behind = _block(in_ch=128, resample='SAME', is_first=False)
    old, C.FIRST_BLOCK = C.FIRST_BLOCK, False
    try:
        assert blk._first_plan_of(shape) is None
        assert behind._fusable() and behind.takes_input_planes((128, 8, 8, 128))
    finally:
        C.FIRST_BLOCK = old


def test_which_blocks_take_the_route():
    import torch
    blk = _block()
    assert blk._first_plan_of((128, 32, 32, 3)).ok and blk._first_plan_of((2, 16, 16, 3)).ok
    assert blk._first_plan_of((2, 8, 8, 3)) is None             # conv2 on 32 output pixels: a partial tile, for layers marked ragged_conv only
    assert blk._first_plan_of((2, 15, 16, 3)) is None           # a DOWN block halves the grid
    assert blk._first_plan(torch.zeros(2, 16, 16, 3)) is None   # not on the GPU
    assert _block(resample='SAME')._first_plan_of((2, 8, 8, 3)).ok
    assert _block(is_first=False)._first_plan_of((128, 32, 32, 3)) is None
    assert _block(in_ch=128)._first_plan_of((128, 32, 32, 128)) is None         # conv1 is a block convolution there
    assert _block(in_ch=4)._first_plan_of((128, 32, 32, 4)) is None             # 36 rows: not a narrow layer
    assert _block(norm='b')._first_plan_of((128, 32, 32, 3)) is None            # a norm at the second site: not wired
