"""CPU tests behind tests/test_narrow_last_gpu.py (the generator's last layer on the narrow kernels): the row table
against the library's predicates and workspace sizes, the entries' argument checks, conv.narrow_last_supported, the recipe helper, the
mark on a CPU generator, and the sensitivity of the GPU tests' bounds to the faults the rows are there for.  No kernel is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import narrow_last_reference as R
import narrow_out_reference as NO

WC_ERR_NULL, WC_ERR_SHAPE, WC_ERR_WORKSPACE, WC_ERR_ARG = -1, -2, -4, -5


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _geom(row):
    """the narrow kernels' own argument order: (N, H, W, Cin = the layer's few outputs, Cout = its wide side, ksize)"""
    return (row.N, row.H, row.W, row.Cn, row.Cw, row.k)


def test_the_table_holds_the_rows_the_issue_names():
    assert [r.name for r in R.ROWS] == ['2x5x7-32-3-k3', '1x2x2-32-1-k3', '3x4x6-96-3-k3', '2x8x8-160-2-k1', '1x33x3-32-3-k3', '5x16x16-32-3-k3',
                                        '2x128x128-32-3-k3', '2x64x64-64-3-k3']
    for r in R.ROWS:
        assert r.name == R.name_of(r.N, r.H, r.W, r.Cw, r.Cn, r.k)
    assert tuple(R.ROWS[i].name for i in (0, 1, 3)) == R.POISON_ROWS and R.ROWS[-1].name == R.OLD_BITS_ROW
    assert {r.Cw % 64 for r in R.ROWS} == {0, 32} and {r.k for r in R.ROWS} == {1, 3} and min(r.W for r in R.ROWS) == 2


@pytest.mark.parametrize("name", [r.name for r in R.ROWS])
def test_the_predicates_and_the_workspace_on_the_table(name, lib):
    row = R.by_name(name)
    g = _geom(row)
    assert lib.wc_conv_narrow32_supported(*g) == 1
    assert lib.wc_conv_narrow64_supported(*g) == (0 if row.Cw % 64 == 32 else 1)
    assert lib.wc_conv_wrw_narrow_supported(*g) == (0 if row.Cw % 128 else 1)
    assert lib.wc_conv_fwd_narrow_split_supported(*g) in ((0,) if row.Cw % 64 else (0, 1))
    nb = lib.wc_conv_wrw_narrow32_workspace_bytes(*g)
    assert nb > 0
    if row.Cw % 64 == 0:
        assert nb == lib.wc_conv_wrw_narrow64_workspace_bytes(*g) == row.nparts * row.groups * 4096 * 4
    else:
        # the entries that were there size nothing for such a row; here: one partial of 1024 floats per pixel range and 32-group
        assert lib.wc_conv_wrw_narrow64_workspace_bytes(*g) == 0 and lib.wc_conv_wrw_narrow_workspace_bytes(*g) == 0
        assert row.groups == row.Cw // 32 and nb == row.nparts * row.groups * 1024 * 4
    # the forward's predicate takes the row in the layer's own orientation
    assert lib.wc_conv_narrow_out_supported(row.N, row.H, row.W, row.Cw, row.Cn, row.k) == 1


def test_every_narrow_predicate_declines_what_it_declined(lib):
    every = (lib.wc_conv_narrow32_supported, lib.wc_conv_wrw_narrow32_workspace_bytes, lib.wc_conv_narrow64_supported,
             lib.wc_conv_wrw_narrow_supported, lib.wc_conv_fwd_narrow_split_supported, lib.wc_conv_wrw_narrow64_workspace_bytes,
             lib.wc_conv_wrw_narrow_workspace_bytes)
    for g in R.DECLINED:
        assert [int(f(*g) != 0) for f in every] == [0] * len(every), g
    # the superset: multiples of 32 taken, the entries that were there as they were
    for cw, want32, want64, want128 in ((32, 1, 0, 0), (64, 1, 1, 0), (96, 1, 0, 0), (128, 1, 1, 1), (160, 1, 0, 0), (48, 0, 0, 0), (16, 0, 0, 0)):
        g = (2, 5, 7, 3, cw, 3)
        assert (lib.wc_conv_narrow32_supported(*g), lib.wc_conv_narrow64_supported(*g), lib.wc_conv_wrw_narrow_supported(*g)) == \
            (want32, want64, want128), cw
    assert lib.wc_conv_narrow32_supported(1, 1, 2 ** 31 - 1, 1, 32, 1) == 1 and lib.wc_conv_narrow32_supported(1, 2, 2 ** 30, 1, 32, 1) == 0
    for g in ((0, 5, 7, 3, 32, 3), (2, 0, 7, 3, 32, 3), (2, 5, 0, 3, 32, 3), (2, 5, 7, 0, 32, 3), (2, 5, 7, 3, 0, 3)):
        assert lib.wc_conv_narrow32_supported(*g) == 0


def test_the_entries_check_their_arguments_before_touching_memory(lib):
    one = ctypes.c_void_p(16)
    row = R.ROWS[0]
    g = _geom(row)
    nb = lib.wc_conv_wrw_narrow32_workspace_bytes(*g)
    wrw = lambda x, gy, dw, ws, n, geom=g: lib.wc_conv_wrw_narrow32_f32(x, gy, *geom, dw, 1, 1, 1, 1, None, ws, n, None)
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert wrw(*args, nb) == WC_ERR_ARG
    assert wrw(one, one, one, one, nb - 1) == WC_ERR_WORKSPACE and wrw(one, one, one, one, 0) == WC_ERR_WORKSPACE
    fwd = lambda x, w, y, geom=g: lib.wc_conv_fwd_narrow32_f32(x, w, 1, 1, 1, 1, None, *geom, 0, y, None)
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert fwd(*args) == WC_ERR_ARG
    for d in R.DECLINED:
        assert wrw(one, one, one, one, 1 << 30, d) == WC_ERR_SHAPE and fwd(one, one, one, d) == WC_ERR_SHAPE, d
    # the forward's 32-bit element offset: N*H*W*Cin < 2^31 (the predicate alone takes this grid)
    big = (1, 2 ** 15, 2 ** 14, 4, 32, 1)
    assert lib.wc_conv_narrow32_supported(*big) == 1 and fwd(one, one, one, big) == WC_ERR_SHAPE
    out = lambda gp, w, o, bias, shape: lib.wc_conv_narrow_out_bias_f32(gp, None, w, 1, 1, 1, 1, bias, *shape, o, None)
    shape = (row.N, row.H, row.W, row.Cw, row.Cn, row.k)
    for bias in (None, one):
        for args in ((None, one, one), (one, None, one), (one, one, None)):
            assert out(*args, bias, shape) == WC_ERR_NULL
        assert out(one, one, one, bias, (2, 4, 4, 48, 3, 3)) == WC_ERR_SHAPE and out(one, one, one, bias, (2, 4, 1, 32, 3, 3)) == WC_ERR_SHAPE
        assert out(ctypes.c_void_p(20), one, one, bias, shape) == WC_ERR_ARG            # g on a 16-byte boundary


def test_narrow_last_supported_is_the_two_library_predicates(lib):
    from wc_gan_amd import conv as C
    for row in R.ROWS:
        xs, ws = (row.N, row.H, row.W, row.Cw), (row.Cn, row.Cw, row.k, row.k)
        both = lib.wc_conv_narrow_out_supported(row.N, row.H, row.W, row.Cw, row.Cn, row.k) and lib.wc_conv_narrow32_supported(*_geom(row))
        assert C.narrow_last_supported(xs, ws) == bool(both) is True
    for N, H, W, cn, cw, k in R.DECLINED:
        assert not C.narrow_last_supported((N, H, W, cw), (cn, cw, k, k))
    assert not C.narrow_last_supported((2, 5, 7, 32), (5, 32, 1, 1))             # more than four outputs: not a last layer
    assert not C.narrow_last_supported((2, 5, 7, 64), (3, 32, 3, 3))             # the input's channels are not the weight's
    assert not C.narrow_last_supported((2, 5, 7, 32), (3, 32, 3, 1))
    assert not C.narrow_last_supported((1, 3, NO.WIDEST.W + 1, 32), (1, 32, 3, 3))   # the forward's LDS band does not fit: the predicate of that kernel
    assert lib.wc_conv_narrow32_supported(1, 3, NO.WIDEST.W + 1, 1, 32, 3) == 1


def test_narrow_last_config_copies_and_marks_the_generator_only():
    from wc_gan_amd import train as T
    entry = T.IMAGENET_CONFIGS['imagenet_cond_sa']
    import copy
    before = copy.deepcopy(entry)
    on, off = T.narrow_last_config(entry), T.narrow_last_config(entry, False)
    assert entry == before and 'narrow_last' not in entry['generator']
    assert on['generator']['narrow_last'] is True and off['generator']['narrow_last'] is False
    for out in (on, off):
        assert out is not entry and out['generator'] is not entry['generator']
        assert {k: v for k, v in out['generator'].items() if k != 'narrow_last'} == entry['generator']
        assert {k: v for k, v in out.items() if k != 'generator'} == {k: v for k, v in entry.items() if k != 'generator'}
    assert isinstance(T.IMAGENET_NARROW_LAST_SHIPS, bool)
    ship = T.narrow_last_config(T.slim_blocks_config(entry, T.IMAGENET_SLIM_BLOCKS_SHIPS), T.IMAGENET_NARROW_LAST_SHIPS)
    assert ship['generator']['narrow_last'] is T.IMAGENET_NARROW_LAST_SHIPS and ship['discriminator']['slim_blocks'] is T.IMAGENET_SLIM_BLOCKS_SHIPS
    assert entry == before


@pytest.mark.parametrize("arch", ['res', 'dcgan'])
def test_the_mark_is_on_the_last_layer_only_and_changes_nothing_on_the_cpu(arch):
    from wc_gan_amd.generator import Conv2D, make_generator
    kw = dict(block_sizes=(32, 32), resamples=('UP', 'UP'), first_block_shape=(2, 2, 32), arch=arch, block_norm='b', block_after_norm='ucs',
              last_norm='b', last_after_norm='ucs')
    nets = []
    for mark in (True, False):
        torch.manual_seed(11)
        nets.append(make_generator(narrow_last=mark, **kw))
    G, P = nets
    marked = [n for n, m in G.named_modules() if isinstance(m, Conv2D) and m.narrow_last]
    assert marked == ['final_conv'] and G.final_conv.layer_name == 'Generator.Final'
    assert not any(m.narrow_last for m in P.modules() if isinstance(m, Conv2D))
    assert not make_generator(**kw).final_conv.narrow_last
    torch.manual_seed(5)
    z = torch.randn(4, 128)
    outs = []
    for net in nets:
        img = net(z)
        grads = torch.autograd.grad((img * torch.linspace(-1, 1, img.numel()).view_as(img)).sum(), list(net.parameters()))
        outs.append([img.detach()] + list(grads))
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_a_marked_layer_keeps_its_route_where_the_node_does_not_apply():
    from wc_gan_amd.generator import Conv2D
    torch.manual_seed(2)
    layer = Conv2D(32, 3, (3, 3), narrow_last=True)
    assert layer.narrow_last and not Conv2D(32, 3, (3, 3)).narrow_last
    x = torch.randn(2, 5, 7, 32)
    assert not layer._narrow_last_route(x)                               # on the CPU
    plain = Conv2D(32, 3, (3, 3))
    plain.load_state_dict(layer.state_dict())
    assert torch.equal(layer(x), plain(x))


FAULTS = [('unmirrored', '2x5x7-32-3-k3'), ('unmirrored', '2x128x128-32-3-k3'), ('no_bias', '2x5x7-32-3-k3'), ('no_bias', '2x8x8-160-2-k1'),
          ('remainder', '3x4x6-96-3-k3'), ('remainder', '2x8x8-160-2-k1'), ('remainder_dx', '3x4x6-96-3-k3'),
          ('remainder_dx', '2x8x8-160-2-k1'), ('partial', '5x16x16-32-3-k3'), ('partial', '2x128x128-32-3-k3')]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_the_bounds_see_the_faults_the_rows_are_there_for(fault, name):
    """un-mirrored taps, a dropped bias, a missing remainder group and one partial missing from the reduce are each more than 1e-2 of the
    tensor's maximum off on a row of the table -- a thousand times the bounds of the GPU tests"""
    row = R.by_name(name)
    key, wrong = R.faulty(row, fault)
    err = R.rel(wrong, R.reference(name)[key])
    assert err > 1e-2 >= 1000 * max(R.BOUND, R.Y_BOUND, R.DW_BOUND), (fault, name, err)


def test_the_reference_is_torchs_float64_convolution_and_its_autograd():
    """the two imported helpers, combined as the GPU tests combine them, against torch.nn.functional.conv2d in float64"""
    import torch.nn.functional as F
    for name in ('2x5x7-32-3-k3', '1x2x2-32-1-k3', '3x4x6-96-3-k3', '2x8x8-160-2-k1'):
        row = R.by_name(name)
        x, w, b, gy = R.inputs(row)
        ref = R.reference(name)
        xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b))
        y = F.conv2d(xt.permute(0, 3, 1, 2), wt, bt, padding=row.k // 2).permute(0, 2, 3, 1)
        dx, dw, db = torch.autograd.grad(y, (xt, wt, bt), torch.from_numpy(gy).double())
        for key, t in (('y', y.detach()), ('dx', dx), ('dw', dw), ('db', db)):
            assert ref[key].shape == tuple(t.shape) and R.rel(ref[key], t.numpy()) < 1e-12, (name, key)
