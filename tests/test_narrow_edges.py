"""CPU tests behind tests/test_narrow_edges_gpu.py (the narrow convolution kernels of csrc/wc_conv.hip at every k-step, tile and range
edge): the row table's literals against the restated host plan, the restated plan against what the library says (predicates, the
weight gradient's workspace, the split variant's gate), the multiply-shift division at the table's divisors -- and why a divisor of 1
is declined --, the NumPy float64 direct sums against torch.nn.functional.conv2d and its autograd, and the sensitivity of the GPU
tests' bounds to the defects the rows are there for.  No kernel is launched."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import narrow_reference as R


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


_NAMES = [r.name for r in R.ALL_ROWS]


def test_the_table_holds_the_rows_the_edges_ask_for():
    assert len(set(_NAMES)) == len(_NAMES)
    ks = R.tagged('kstep')
    assert sorted(r.Cin for r in ks if r.k == 1) == [1, 2, 3, 4, 9, 10, 19, 20, 27, 28, 31] and sorted(r.Cin for r in ks if r.k == 3) == [1, 2, 3]
    assert all(r.shape == (2, 5, 7) and r.Cout == 64 for r in ks)
    # both sides of every class gate, the full table, the bias row with and without a tap in its k-step
    assert {(r.nrow, r.inst) for r in ks} >= {(3, 2), (4, 5), (9, 5), (10, 10), (19, 10), (20, 14), (27, 14), (28, 16), (31, 16)}
    assert {r.nrow % 2 for r in ks} == {0, 1}
    assert {(r.Cout, r.nrow) for r in R.tagged('group')} == {(o, n) for o in (128, 192, 256) for n in (27, 31)}
    px = R.tagged('pixel')
    assert [r.M for r in px if r.Cout == 64] == [2, 31, 33, 128, 129, 1024, 1152, 15360, 15488, 16384, 16512, 32768, 32800]
    assert sorted(r.M for r in px if r.Cout == 192) == [33, 16385]
    assert all(r.Cin == 3 and r.k == 3 for r in px)
    assert {r.nparts for r in px} >= {1, 2, 8, 9, 120, 121, 128, 129, 228, 256} and {r.tpw for r in px} == {1, 2} and {r.ppw for r in px} == {16, 18}
    assert {r.ntiles for r in px} >= {1, 2, 1024, 1025}
    sh = R.tagged('shape')
    assert {r.shape for r in sh} == {(3, 6, 10), (2, 7, 7), (2, 14, 28), (4, 2, 3), (3, 1, 9)}
    assert {r.fmt for r in sh} == {'channels_last', 'contiguous'} and {r.bias for r in sh} == {True, False}
    assert {r.Cin for r in R.MIRROR_ROWS} == {1, 3} and {r.Cout for r in R.MIRROR_ROWS} == {64, 128, 192, 256}
    assert {r.shape for r in R.MIRROR_ROWS} >= {(3, 6, 10), (2, 7, 7), (2, 14, 28), (4, 2, 3)} and any(r.M < 32 for r in R.MIRROR_ROWS)
    assert max(r.M * r.Cout for r in R.ALL_ROWS) <= 32800 * 256          # the largest tensor a GPU test allocates


@pytest.mark.parametrize("name", _NAMES)
def test_the_restated_plan_equals_the_rows_literals(name, lib):
    row = R.by_name(name)
    assert R.plan(*row.geom) == row.literals()
    assert R.supported(*row.geom) and lib.wc_conv_narrow64_supported(*row.geom) == 1
    # nparts as the library sizes the partial sums: nparts x ngrp x 4096 floats
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(*row.geom)
    assert nb % (16384 * row.ngrp) == 0 and nb // (16384 * row.ngrp) == row.nparts
    assert lib.wc_conv_wrw_narrow_supported(*row.geom) == (1 if row.Cout % 128 == 0 else 0)
    assert lib.wc_conv_wrw_narrow_workspace_bytes(*row.geom) == (nb if row.Cout % 128 == 0 else 0)
    # the reduce kernel reads every partial once
    assert 16 * row.reduce[0] + row.reduce[1] == row.nparts
    # two tiles per wave and the lifted pixels-per-wave floor come with the sizes the issue names
    assert row.tpw == (1 if row.ntiles <= 1024 else 2) and (row.ppw == 16) == (row.M <= 32768)


def test_the_split_variants_gate_is_the_restated_grid(lib):
    for row in R.ALL_ROWS:
        want = row.grid[0] * row.grid[1] <= R.SPLIT_BLOCKS
        assert R.split_supported(*row.geom) == want and lib.wc_conv_fwd_narrow_split_supported(*row.geom) == int(want), row
        if row.split is not None:
            assert row.split == want, row
    g = {r.name: r for r in R.GATE_ROWS}
    # the largest accepted and the smallest declined M either side of grid = 512 -- and the gate is not monotone in M
    assert g['M32768-o128'].grid == (256, 2) and g['M32768-o128'].split and g['M32769-o128'].split
    assert g['M21760-o192'].split and not g['M21761-o192'].split and g['M21761-o192'].M == g['M21760-o192'].M + 1
    assert not g['M32768-o192'].split and g['M32769-o192'].split and g['M43520-o192'].split and not g['M43521-o192'].split
    for M, cout, want in ((21760, 192, 1), (21761, 192, 0), (32768, 192, 0), (32769, 192, 1), (43520, 192, 1), (43521, 192, 0), (32768, 128, 1),
                          (32769, 128, 1), (65536, 128, 1), (65537, 128, 1)):
        assert lib.wc_conv_fwd_narrow_split_supported(1, 1, M, 3, cout, 3) == want == int(R.split_supported(1, 1, M, 3, cout, 3)), (M, cout)


def test_the_predicates_set(lib):
    every = (lib.wc_conv_narrow64_supported, lib.wc_conv_wrw_narrow_supported, lib.wc_conv_fwd_narrow_split_supported,
             lib.wc_conv_wrw_narrow64_workspace_bytes, lib.wc_conv_wrw_narrow_workspace_bytes)

    def taken(*g):
        got = [int(f(*g) != 0) for f in every]
        assert len(set(got)) == 1, (g, got)
        assert bool(got[0]) == R.supported(*g), g
        return bool(got[0])
    # k*k*Cin = 31 taken, 32 declined
    assert taken(2, 5, 7, 31, 128, 1) and not taken(2, 5, 7, 32, 128, 1)
    assert taken(2, 5, 7, 3, 128, 3) and not taken(2, 5, 7, 4, 128, 3)
    # k in (1, 3)
    for k in (0, 2, 4, 5, 7):
        assert not taken(2, 5, 7, 1, 128, k)
    # Cout in 64s; the ABI-7 entry in 128s
    for cout in (1, 3, 32, 96, 100, 160):
        assert not taken(2, 5, 7, 3, cout, 3)
    for cout in (64, 192, 320):
        g = (2, 5, 7, 3, cout, 3)
        assert lib.wc_conv_narrow64_supported(*g) == 1 and lib.wc_conv_wrw_narrow64_workspace_bytes(*g) > 0
        assert lib.wc_conv_wrw_narrow_supported(*g) == 0 and lib.wc_conv_wrw_narrow_workspace_bytes(*g) == 0
    for g in ((0, 5, 7, 3, 128, 3), (2, 0, 7, 3, 128, 3), (2, 5, 0, 3, 128, 3), (2, 5, 7, 0, 128, 3), (2, 5, 7, 3, 0, 3)):
        assert not taken(*g)
    assert taken(1, 1, 2, 3, 128, 3) and taken(1, 1, 2 ** 31 - 1, 1, 128, 1) and not taken(1, 2, 2 ** 30, 1, 128, 1)
    # a one-pixel-wide image: the multiply-shift division wants divisors >= 2 (conv_geom_ok's line)
    for g in R.W1_GEOMS:
        assert not taken(*g), g
        assert lib.wc_conv_narrow64_supported(g[0], g[2], max(2, g[1]), *g[3:]) == 1, g           # (the same image lying down is taken)


def test_the_entries_refuse_a_one_pixel_wide_image_before_touching_memory(lib):
    import ctypes
    one = ctypes.c_void_p(16)
    for g in R.W1_GEOMS:
        N, H, W, ci, co, k = g
        assert lib.wc_conv_fwd_narrow_f32(one, one, 1, 1, 1, 1, None, N, H, W, ci, co, k, 0, one, None) == -2
        assert lib.wc_conv_fwd_narrow_split_f32(one, one, 1, 1, 1, 1, None, N, H, W, ci, co, k, 1, 0.0, one, one, one, one, one, 0, None) == -2
        for f in (lib.wc_conv_wrw_narrow64_f32, lib.wc_conv_wrw_narrow_f32):
            assert f(one, one, N, H, W, ci, co, k, one, 1, 1, 1, 1, None, one, 1 << 30, None) == -2
        assert lib.wc_conv_wrw_narrow_masked_f32(one, one, one, N, H, W, ci, co, k, one, 1, 1, 1, 1, None, one, 1 << 30, None) == -2


def test_the_multiply_shift_division_is_exact_at_the_tables_divisors_and_not_for_one():
    divisors = sorted({d for r in R.ALL_ROWS for d in (r.shape[1] * r.shape[2], r.shape[2])})
    assert min(divisors) == 2
    for d in divisors:
        mag, sh = R.magic_u31(d)
        assert mag < 2 ** 32 and sh < 32
        Ms = {r.M for r in R.ALL_ROWS if d in (r.shape[1] * r.shape[2], r.shape[2])}
        for m in sorted({0, d - 1, d, 2 * d - 1, 2 ** 31 - 1} | {M - 1 for M in Ms} | {k * d + e for k in (1, 7, 2 ** 31 // d - 1) for e in (-1, 0)}):
            if 0 <= m < 2 ** 31:
                assert R.mulshift(m, mag, sh) == m // d, (d, m)
    rng = np.random.default_rng(5)
    for d in divisors:
        mag, sh = R.magic_u31(d)
        for m in rng.integers(0, 2 ** 31, 200).tolist():
            assert R.mulshift(m, mag, sh) == m // d, (d, m)
    # d = 1: mag = 2^31 and a shift count of 0xFFFFFFFF, of which the hardware takes five bits -- the quotient is 0 for every m
    assert R.magic_u31(1) == (2 ** 31, 0xFFFFFFFF)
    assert all(R.mulshift(m, *R.magic_u31(1)) == 0 for m in (0, 1, 2, 31, 2 ** 31 - 1))


# ---- the direct sums against torch in float64 ----------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _torch_reference(x, w, b, gy, k, mask=None):
    xt, wt = _t(x).permute(0, 3, 1, 2).requires_grad_(True), _t(w).requires_grad_(True)
    bt = None if b is None else _t(b).requires_grad_(True)
    y = F.conv2d(xt, wt, bt, padding=k // 2)
    g = _t(gy)
    if mask is not None:
        g = torch.ops.aten.threshold_backward(g, torch.from_numpy(mask).double(), 0)
    grads = torch.autograd.grad(y, (xt, wt) + (() if bt is None else (bt,)), g.permute(0, 3, 1, 2))
    return (y.permute(0, 2, 3, 1).detach().numpy(), grads[0].permute(0, 2, 3, 1).numpy(), grads[1].numpy(), g.sum((0, 1, 2)).numpy())


@pytest.mark.parametrize("name", [r.name for r in R.SMALL_ROWS])
def test_the_direct_sums_equal_torch_in_float64(name):
    row = R.by_name(name)
    x, w, b, gy, h = R.inputs(row)
    ref = R.reference(name)
    y, _, dw, db = _torch_reference(x, w, b, gy, row.k)
    assert R.rel(ref['y'], y) < 1e-12 and R.rel(ref['relu'], np.maximum(y, 0)) < 1e-12
    assert R.rel(ref['dw'], dw) < 1e-12 and R.rel(ref['db'], db) < 1e-12
    assert ref['dw'].shape == w.shape and ref['y'].shape == gy.shape
    _, _, mdw, mdb = _torch_reference(x, w, b, gy, row.k, mask=h)
    assert R.rel(ref['mdw'], mdw) < 1e-12 and R.rel(ref['mdb'], mdb) < 1e-12
    assert np.isnan(h).any() and (h < 0).any() and R.rel(ref['mdw'], dw) > 1e-2        # the mask takes a visible part away


@pytest.mark.parametrize("name", [r.name for r in R.MIRROR_ROWS])
def test_the_mirrored_and_exchanged_sums_equal_torchs_gradients_in_float64(name):
    row = R.by_name(name)
    x, w, gy = R.mirror_inputs(row)
    ref = R.mirror_reference(name)
    _, dx, dw, _ = _torch_reference(x, w, None, gy, row.k)
    assert ref['dx'].shape == x.shape and ref['dw'].shape == w.shape
    assert R.rel(ref['dx'], dx) < 1e-12 and R.rel(ref['dw'], dw) < 1e-12


# ---- what the GPU tests' bounds see --------------------------------------------------------------------------------------------------
def test_a_dropped_bias_row_is_seen():
    for row in R.tagged('kstep') + R.tagged('group'):
        x, w, b, gy, _ = R.inputs(row)
        assert R.rel(R.forward(x, w, None), R.reference(row.name)['y']) > 1e-2, row
        D = R.product_rows(x, gy, row.k)
        assert np.abs(D[-1]).max() > 1e-2 * np.abs(D).max(), row           # db is no small row of the product


def test_unmirrored_taps_are_seen():
    for row in R.MIRROR_ROWS:
        x, w, gy = R.mirror_inputs(row)
        ref = R.mirror_reference(row.name)
        straight = R.forward(gy, np.ascontiguousarray(w.transpose(1, 0, 2, 3)), None)
        assert R.rel(straight, ref['dx']) > 1e-2, row
        dwt, _ = R.gradients_of(R.product_rows(gy, x, row.k), gy.shape[3], row.k)
        assert R.rel(dwt.transpose(1, 0, 2, 3), ref['dw']) > 1e-2, row


def test_an_unwritten_last_partial_tile_is_seen():
    rows = [r for r in R.SMALL_ROWS if r.M % 32] + [R.by_name('M32800'), R.by_name('M16385-o192')]
    assert {r.name for r in R.tagged('partial')} <= {r.name for r in rows}
    for row in rows:
        y = R.reference(row.name)['y'].reshape(row.M, row.Cout)
        bad = y.copy()
        bad[32 * (row.ntiles - 1):] = 0.0
        assert R.rel(bad, y) > 1e-2, row


def test_one_partial_missing_from_the_reduce_is_seen():
    rows = [r for r in R.tagged('pixel') if r.nparts >= 2]
    assert {r.nparts for r in rows} >= {2, 8, 9, 120, 121, 128, 129, 228, 256}
    for row in rows:
        x, _, _, gy, _ = R.inputs(row)
        D = R.product_rows(x, gy, row.k)
        span = 8 * row.ppw
        for part, floor in ((row.nparts // 2, 1e-2), (row.nparts - 1, 100 * R.DW_BOUND)):        # a full partial; the last, as short as one pixel
            px = np.arange(part * span, min(row.M, (part + 1) * span))
            assert R.rel(D - R.product_rows(x, gy, row.k, pixels=px), D) > floor, (row, part)


def test_the_idle_half_group_written_for_192_outputs_is_seen():
    """Cout = 192: the second group's upper 64 channels do not exist; its lanes hold sums of the group's first channels.  Written, they
    would land 64 channels further on -- in the next input channel's (or tap's) weights, or behind the tensor."""
    for row in R.tagged('o192'):
        x, _, _, gy, _ = R.inputs(row)
        D = R.product_rows(x, gy, row.k)
        wide = np.zeros((D.shape[0], 256))
        wide[:, :192] = D
        bad = wide.copy()
        bad[:, 192:] = D[:, 128:192]
        assert np.abs(bad - wide).max() > 1e-2 * np.abs(D).max(), row
