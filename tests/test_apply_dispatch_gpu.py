"""K3, the fused apply (wc_apply_act_f32, wc_apply_mask_f32, wc_apply_planes_f32, wc_apply_split_ex_f16x2) and K6, the backward apply
(wc_bwd_apply_scaled_f32, wc_bwd_apply_bits_f32, wc_bwd_apply_xsplit_f32) at every pipeline class, tile order and slot edge, against
float64 numpy of the same expression.  These kernels are DMA rings whose hand-counted waits depend on how many tiles a workgroup owns;
the workloads' shapes give every workgroup 8 or 16 tiles.  The rows, the class each one is there for, the launch arithmetic that labels
them and the conditions on their inputs are in test_apply_dispatch.py (CPU); here each row runs through wc_gan_amd.ops:

  affine_ring_kernel    ops.apply(plan=) plain and ReLU'd, + the bit mask, + the planes form (the grid is read off the per-workgroup maxima)
  apply_split_kernel    ops.apply_split on the planes ops.split wrote (the reference: float64 on the values the planes hold exactly)
  onepass_ring_kernel   ops.bwd_apply(scales=), relu_mask=, ops.bwd_apply_xsplit at C = 256
  affine_f16x3_kernel   the accumulating pass of a two-pass K6; ops.bwd_apply_xsplit at C = 128 with a slot table
  rows_gemm_kernel      fast=False and the shapes the fast path declines

Bounds: 3e-6 of the reference's maximum (test_fast_gpu.py, test_split_gpu.py), 2^-20 max|y| for planes against the fp32 output and bit
equality for masks (test_handoff_gpu.py).

`PYTHONPATH=. python tests/test_apply_dispatch_gpu.py` prints every row's class and measured errors (profiles/apply_dispatch_parity.txt)."""
import numpy as np
import pytest
import torch

from test_apply_dispatch import (ACC_ROWS, GEMM_ROWS, K3_TOL, ONEPASS_ROWS, RING, RING_ROWS, ROWS, SPLIT_ROWS, XSPLIT128_ROWS, fast_affine_supported,
                                 k3_inputs, k6_inputs, k6_ref, label, nhwc, onepass_supported, plan_acc, plan_onepass, plan_ring, plan_rows,
                                 plan_split, row_id)
from test_conv_dispatch_gpu import _kernel_names
from test_fast_gpu import _mask_ref, _ref_apply
from test_site_dispatch_gpu import _site_row, dev, rel
from test_split_gpu import _planes64

pytestmark = pytest.mark.gpu
SITE_TOL = 1e-4         # the site's contract (test_configs_gpu.py)
MAXIMA_AT = 2 + 1024    # the per-workgroup maxima inside ops.out_scale's record (csrc/wc_fast.hip, FastArgs::oamax)


def _st(d, Kc):
    return dev(d['slot'], torch.int32) if Kc > 1 else None


def _check_kernel(fn, kernel):
    """the kernel of one profiled call, by name"""
    names = _kernel_names(fn)
    if not names:
        pytest.skip("this profiler build reports no device kernel names: the kernel was not checked (the plan and parity assertions ran)")
    assert any(kernel + '<' in n or kernel + '(' in n for n in names), (kernel, names)


def _tables(ops, d, xd, mud):
    """-> (A, plan): the apply's fp16 tables of d['A'] (ops.color with W = I) for power-of-two channel scales that put max |x - mu| of
    a channel into [8, 16) -- where the library's own sampled scales put it"""
    C = xd.shape[-1]
    e = torch.frexp((xd.view(-1, C) - mud).abs().amax(0))[1]
    cs = torch.ldexp(torch.ones(C, device="cuda"), 4 - e)
    A, _At, plan = ops.color(torch.eye(C, dtype=torch.float64, device="cuda"), dev(d['A']), cs)
    return A, plan


def _whitened_tables(d):
    """d['A'] in units of the channels' standard deviations: the coloring out_scale() predicts the output range from"""
    mag = d['mu'].astype(np.float64) / 3
    return dev(d['A'] * mag[None, :, None])


def _poisoned_record(ops, d, C):
    rec = ops.out_scale(_whitened_tables(d), dev(d['b']), C, "cuda")
    rec[MAXIMA_AT:] = -1.0          # no maximum is negative: what the kernel writes can be counted
    return rec


def _planes_errs(planes, rec, y):
    s = float(rec[0])
    back = (planes[0].double() + planes[1].double()) / s
    return dict(scale_pow2=bool(s > 0 and np.log2(s) == int(np.log2(s))), planes=float((back - y.double()).abs().max()) / float(y.abs().max()),
                maxima=int((rec[MAXIMA_AT:] != -1.0).sum()))


# ---- affine_ring_kernel<C, SLOT, MASK, PL> ----------------------------------------------------------------------------------------
def _ring_row(ops, shape, Kc):
    """-> errors of every epilogue the shape supports, plain and ReLU'd, and what a profiled call needs"""
    N, HW, C = nhwc(shape)
    p = plan_ring(shape, Kc > 1)
    d = k3_inputs(shape, Kc, p['T'])
    xd, mud, bd, st = dev(d['x']), dev(d['mu']), dev(d['b']), _st(d, Kc)
    A, plan = _tables(ops, d, xd, mud)
    ref = _ref_apply(d['x'], d['mu'], A.cpu().numpy(), d['b'], d['slot'])
    flat = lambda t: t.cpu().numpy().reshape(ref.shape)
    errs = dict(y=rel(flat(ops.apply(xd, mud, A, bd, st, plan=plan)), ref))
    errs['y_relu'] = rel(flat(ops.apply(xd, mud, A, bd, st, plan=plan, relu=True)), np.maximum(ref, 0))
    if N * HW % 32 == 0:
        y, mask = ops.apply(xd, mud, A, bd, st, plan=plan, relu=True, want_mask=True)
        errs['y_mask'] = rel(flat(y), np.maximum(ref, 0))
        errs['mask_exact'] = bool(np.array_equal(mask.cpu().numpy().view(np.uint32), _mask_ref(y.cpu().numpy().reshape(-1, C))))
        errs['planes_form'] = ops.apply_planes_supported(shape)
        if errs['planes_form']:
            planes, rec, pmask = ops.apply_planes(xd, mud, A, bd, st, plan, _poisoned_record(ops, d, C), relu=True, want_mask=True)
            errs.update(_planes_errs(planes, rec, y), masks_equal=torch.equal(mask, pmask))
    return errs, p, lambda: ops.apply(xd, mud, A, bd, st, plan=plan)


def _assert_k3(errs, p):
    for k in ('y', 'y_relu', 'y_mask'):
        assert errs.get(k, 0.0) < K3_TOL, errs
    assert errs.get('mask_exact', True), errs
    if errs.get('planes_form') or 'planes' in errs:
        assert errs['scale_pow2'] and errs['planes'] <= 2.0 ** -20 and errs['masks_equal'], errs
        assert errs['maxima'] == p['grid'], (errs, p['grid'])           # one maximum per workgroup: the restated grid is the launch's


RING_PROFILED = {((65, 16, 16, 256), 3), ((257, 8, 4, 256), 3), ((161, 16, 16, 64), 3)}


@pytest.mark.parametrize("row", RING_ROWS, ids=row_id)
def test_k3_on_fp32_at_each_tile_count_and_slot_edge(row):
    from wc_gan_amd import ops
    shape, Kc, want = row
    errs, p, call = _ring_row(ops, shape, Kc)
    print("apply dispatch K3", row_id(row), label(p), errs)
    assert label(p) == want
    assert errs.get('planes_form', False) == (p['kernel'] == RING and shape[-1] in (128, 256)), errs
    _assert_k3(errs, p)
    if (shape, Kc) in RING_PROFILED:
        _check_kernel(call, p['kernel'])


# ---- apply_split_kernel<C, SLOT, MASK, PL> ----------------------------------------------------------------------------------------
def _split_row(ops, shape, Kc):
    N, HW, C = nhwc(shape)
    p = plan_split(shape, Kc > 1)
    d = k3_inputs(shape, Kc, p['T'])
    mud, Ad, bd, st = dev(d['mu']), dev(d['A']), dev(d['b']), _st(d, Kc)
    xs = ops.split(dev(d['x']))
    ref = _ref_apply(_planes64(xs).reshape(shape), d['mu'], d['A'], d['b'], d['slot'])
    flat = lambda t: t.cpu().numpy().reshape(ref.shape)
    errs = dict(flag=int(xs.flag[0]), y=rel(flat(ops.apply_split(xs, mud, Ad, bd, st)), ref))
    errs['y_relu'] = rel(flat(ops.apply_split(xs, mud, Ad, bd, st, relu=True)), np.maximum(ref, 0))
    if N * HW % 32 == 0:
        y, mask = ops.apply_split(xs, mud, Ad, bd, st, relu=True, want_mask=True)
        errs['y_mask'] = rel(flat(y), np.maximum(ref, 0))
        errs['mask_exact'] = bool(np.array_equal(mask.cpu().numpy().view(np.uint32), _mask_ref(y.cpu().numpy().reshape(-1, C))))
        planes, rec, pmask = ops.apply_split(xs, mud, Ad, bd, st, relu=True, want_mask=True, oscale=_poisoned_record(ops, d, C))
        errs.update(_planes_errs(planes, rec, y), masks_equal=torch.equal(mask, pmask))
    return errs, p, lambda: ops.apply_split(xs, mud, Ad, bd, st)


@pytest.mark.parametrize("row", SPLIT_ROWS, ids=row_id)
def test_k3_on_planes_at_each_tile_count_and_slot_edge(row):
    from wc_gan_amd import ops
    shape, Kc, want = row
    assert ops.apply_split_supported(shape)
    errs, p, call = _split_row(ops, shape, Kc)
    print("apply dispatch K3 planes", row_id(row), label(p), errs)
    assert label(p) == want and errs['flag'] == 0
    _assert_k3(errs, p)
    if (shape, Kc) == ((193, 16, 16, 256), 3):
        _check_kernel(call, p['kernel'])


# ---- K6 --------------------------------------------------------------------------------------------------------------------------
def _k6_args(d, Kc):
    return dict(gy=dev(d['gy']), x=dev(d['x']), mu=dev(d['mu']), At=dev(d['At']), S=dev(d['S']), gm=dev(d['gm']), st=_st(d, Kc))


def _k6_ref(d, shape, gy=None, x=None):
    N, HW, C = nhwc(shape)
    return k6_ref(d['gy'] if gy is None else gy, d['x'] if x is None else x, d['mu'], d['At'], d['S'], d['gm'], np.repeat(d['slot'], HW))


def _xsplit(ops, d, a, Kc, shape):
    """K6 on the planes of the same x (scales from K4 on the planes) -> its error against float64 on what the planes hold"""
    xs = ops.split(a['x'])
    sc = ops.bwd_reduce_xsplit(xs, a['mu'], a['gy'], a['st'], Kc)[-1]
    dx = ops.bwd_apply_xsplit(a['gy'], xs, a['mu'], a['At'], a['S'], a['gm'], a['st'], sc)
    ref = _k6_ref(d, shape, x=_planes64(xs))
    return int(xs.flag[0]), rel(dx.cpu().numpy().reshape(ref.shape), ref)


def _onepass_row(ops, shape, Kc, forms):
    N, HW, C = nhwc(shape)
    p = plan_onepass(shape, Kc > 1)
    d = k6_inputs(shape, Kc, p['T'])
    a = _k6_args(d, Kc)
    ref = _k6_ref(d, shape)
    scales = ops.bwd_reduce(a['x'], a['mu'], a['gy'], a['st'], Kc, want_scales=True)[-1]
    call = lambda: ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], scales=scales)
    errs = dict(scaled=rel(call().cpu().numpy().reshape(ref.shape), ref))
    errs['bits_form'], errs['xsplit_form'] = ops.bwd_bits_supported(shape, Kc > 1), ops.bwd_xsplit_supported(shape, Kc > 1)
    if forms:
        y = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
        y[0, 0, 0, :8] = 0.0; y[0, 0, 1, :8] = -0.0; y[1, 2, 3, 4] = np.nan          # the edges of `y > 0`
        mask = dev(_mask_ref(y.reshape(-1, C)).view(np.int32), torch.int32)
        sc = ops.bwd_reduce(a['x'], a['mu'], a['gy'], a['st'], Kc, want_scales=True, relu_mask=mask, write_masked=False)[-1]
        dxb = ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], scales=sc, relu_mask=mask)
        refb = _k6_ref(d, shape, gy=np.where(~(y <= 0), d['gy'], np.float32(0)))
        errs['bits'] = rel(dxb.cpu().numpy().reshape(refb.shape), refb)
        errs['flag'], errs['xsplit'] = _xsplit(ops, d, a, Kc, shape)
    return errs, p, call


@pytest.mark.parametrize("row", ONEPASS_ROWS, ids=row_id)
def test_k6_in_one_pass_at_each_tile_count_and_slot_edge(row):
    from wc_gan_amd import ops
    shape, Kc, want, forms = row
    assert onepass_supported(shape)             # the route: bwd_apply_impl takes the one-pass kernel exactly here (the CPU file pins it)
    errs, p, call = _onepass_row(ops, shape, Kc, forms)
    print("apply dispatch K6 one pass", row_id(row), label(p), errs)
    assert label(p) == want
    assert errs['bits_form'] == forms and errs['xsplit_form'] == forms, errs
    assert errs['scaled'] < K3_TOL and errs.get('bits', 0.0) < K3_TOL and errs.get('xsplit', 0.0) < K3_TOL and errs.get('flag', 0) == 0, errs
    if (shape, Kc) in {((65, 8, 8, 256), 3), ((128, 6, 6, 256), 3)}:
        _check_kernel(call, p['kernel'])


def _acc_row(ops, shape, Kc, with_scales):
    p = plan_acc(shape, False)
    d = k6_inputs(shape, Kc, p['T'])
    a = _k6_args(d, Kc)
    ref = _k6_ref(d, shape)
    scales = ops.bwd_reduce(a['x'], a['mu'], a['gy'], a['st'], Kc, want_scales=True)[-1] if with_scales else None
    call = lambda: ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], scales=scales)
    return dict(two_pass=rel(call().cpu().numpy().reshape(ref.shape), ref)), p, call


@pytest.mark.parametrize("row", ACC_ROWS, ids=row_id)
def test_k6_in_two_passes_at_each_tile_count(row):
    from wc_gan_amd import ops
    shape, Kc, with_scales, want = row
    assert fast_affine_supported(shape) and not (with_scales and onepass_supported(shape))
    errs, p, call = _acc_row(ops, shape, Kc, with_scales)
    print("apply dispatch K6 two passes", row_id(row), label(p), errs)
    assert label(p) == want
    assert errs['two_pass'] < K3_TOL, errs
    if shape in ((129, 16, 16, 256), (260, 16, 16, 128)):
        _check_kernel(call, p['kernel'])


def _xsplit128_row(ops, shape, Kc, site=True):
    """K6 on planes at C = 128 with a slot table where the library takes the shape; elsewhere the refusal, the fp32 K6 of the same
    inputs and the site on the route it then takes"""
    from wc_gan_amd import _lib
    from wc_gan_amd.functional import split_route_supported
    p = plan_acc(shape, True)
    d = k6_inputs(shape, Kc, p['T'])
    a = _k6_args(d, Kc)
    ref = _k6_ref(d, shape)
    scales = ops.bwd_reduce(a['x'], a['mu'], a['gy'], a['st'], Kc, want_scales=True)[-1]
    errs = dict(taken=ops.bwd_xsplit_supported(shape, True),
                scaled=rel(ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], scales=scales).cpu().numpy().reshape(ref.shape), ref))
    call = None
    if errs['taken']:
        errs['flag'], errs['xsplit'] = _xsplit(ops, d, a, Kc, shape)
        xs = ops.split(a['x'])
        sc = ops.bwd_reduce_xsplit(xs, a['mu'], a['gy'], a['st'], Kc)[-1]
        call = lambda: ops.bwd_apply_xsplit(a['gy'], xs, a['mu'], a['At'], a['S'], a['gm'], a['st'], sc)
    else:
        xs = ops.split(a['x'])
        with pytest.raises(_lib.WcHipError, match="WC_ERR_SHAPE"):
            ops.bwd_apply_xsplit(a['gy'], xs, a['mu'], a['At'], a['S'], a['gm'], a['st'], scales)
        if site:        # the site itself: on planes where the layers would hand it planes (its backward then reads the fp32 copy)
            planes = bool(split_route_supported(shape, True))
            fused = ops.resadd_stats_supported(shape, True, 1) if planes else None
            errs['site_on_planes'] = planes
            errs.update({'site_' + k: v for k, v in _site_row(shape, Kc, planes, fused, "well").items()})
    return errs, p, call


@pytest.mark.parametrize("row", XSPLIT128_ROWS, ids=row_id)
def test_k6_on_planes_at_128_channels_takes_one_table_per_tile_only_where_tiles_lie_inside_samples(row):
    """affine_f16x3_kernel<128, ACC, SLOT> reads slot[first row of the tile / HW] for all 128 rows of a tile and has no per-row redo.
    Before wc_bwd_xsplit_supported declined HW % 128 != 0 with a slot table, every odd sample of (256, 8, 8, 128) took its even
    neighbour's table for gy At: `xsplit` read 1.03 of max |dx| on that row, 1.00 on (32, 24, 24, 128) and 1.15 on (320, 8, 8, 128), whose
    site on planes returned dx 1.32 of its maximum off the oracle's (3e-7 on every row since)."""
    from wc_gan_amd import ops
    shape, Kc, want, taken = row
    errs, p, call = _xsplit128_row(ops, shape, Kc)
    print("apply dispatch K6 planes C=128", row_id(row), label(p), errs)
    assert label(p) == want and errs['taken'] == taken
    assert errs['scaled'] < K3_TOL and errs.get('xsplit', 0.0) < K3_TOL and errs.get('flag', 0) == 0, errs
    assert all(v < SITE_TOL for k, v in errs.items() if k.startswith('site_') and k != 'site_on_planes'), errs
    if call is not None:
        _check_kernel(call, p['kernel'])


# ---- rows_gemm_kernel ------------------------------------------------------------------------------------------------------------
def _gemm_row(ops, shape, Kc):
    N, HW, C = nhwc(shape)
    p = plan_rows(shape, Kc > 1)
    d = k3_inputs(shape, Kc, p['T'])
    xd, mud, Ad, bd, st = dev(d['x']), dev(d['mu']), dev(d['A']), dev(d['b']), _st(d, Kc)
    ref = _ref_apply(d['x'], d['mu'], d['A'], d['b'], d['slot'])
    flat = lambda t: t.cpu().numpy().reshape(ref.shape)
    call = lambda: ops.apply(xd, mud, Ad, bd, st, fast=False)
    errs = dict(y=rel(flat(call()), ref))
    if N * HW % 32 == 0:
        y, mask = ops.apply(xd, mud, Ad, bd, st, fast=False, relu=True, want_mask=True)
        errs['y_mask'] = rel(flat(y), np.maximum(ref, 0))
        errs['mask_exact'] = bool(np.array_equal(mask.cpu().numpy().view(np.uint32), _mask_ref(y.cpu().numpy().reshape(-1, C))))
    d6 = k6_inputs(shape, Kc, p['T'])
    a = _k6_args(d6, Kc)
    ref6 = _k6_ref(d6, shape)
    errs['k6'] = rel(ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], fast=False).cpu().numpy().reshape(ref6.shape), ref6)
    return errs, p, call


@pytest.mark.parametrize("row", GEMM_ROWS, ids=row_id)
def test_k3_and_k6_off_the_fast_path_on_ragged_blocks(row):
    from wc_gan_amd import ops
    shape, Kc, want = row
    errs, p, call = _gemm_row(ops, shape, Kc)
    print("apply dispatch rows_gemm", row_id(row), label(p), errs)
    assert label(p) == want and p['kernel'] == ROWS
    assert errs['y'] < K3_TOL and errs.get('y_mask', 0.0) < K3_TOL and errs.get('mask_exact', True) and errs['k6'] < K3_TOL, errs
    if shape[-1] == 160:
        _check_kernel(call, ROWS)


# ---- one overflow row per ring kernel: an element beyond the fp16 range in the LAST tile of a 5-tile workgroup ----------------------
def _rest(got, ref, row):
    keep = np.ones(len(ref), bool); keep[row] = False
    return rel(got[keep], ref[keep])


def _overflow_k3(ops):
    """test_fast_apply_out_of_range_tiles_take_the_exact_path's construction on (129, 16, 16, 256) with slots: workgroup 0 owns tiles
    0...4 and the element sits in tile 4, so its exact redo of all five follows a full schedule"""
    shape, Kc = (129, 16, 16, 256), 3
    p = plan_ring(shape, True)
    assert p['owned'][0] == [0, 1, 2, 3, 4]
    d = k3_inputs(shape, Kc, p['T'])
    xd, mud, bd, st = dev(d['x']), dev(d['mu']), dev(d['b']), _st(d, Kc)
    A, plan = _tables(ops, d, xd, mud)          # the scales of the clean tensor
    row = 4 * p['T'] + 11
    x = d['x'].copy().reshape(-1, 256)
    x[row, 7] = 3.0e7 * d['mu'][7]
    xd.view(-1, 256)[row, 7] = float(x[row, 7])
    ref = _ref_apply(x.reshape(shape), d['mu'], A.cpu().numpy(), d['b'], d['slot']).reshape(-1, 256)
    y = ops.apply(xd, mud, A, bd, st, plan=plan)
    got = y.cpu().numpy().reshape(ref.shape)
    return dict(finite=bool(np.isfinite(got).all()), all=rel(got, ref), other_rows=_rest(got, ref, row))


def _overflow_k6(ops):
    """the same in gy for the one-pass kernel: (129, 8, 8, 256) with slots, pair 0 owns tiles 0...4"""
    shape, Kc = (129, 8, 8, 256), 3
    p = plan_onepass(shape, True)
    assert p['owned'][0] == [0, 1, 2, 3, 4]
    d = k6_inputs(shape, Kc, p['T'])
    a = _k6_args(d, Kc)
    scales = ops.bwd_reduce(a['x'], a['mu'], a['gy'], a['st'], Kc, want_scales=True)[-1]       # the scales of the clean tensors
    row = 4 * p['T'] + 5
    gy = d['gy'].copy().reshape(-1, 256)
    gy[row, 9] = 5.0e4
    a['gy'].view(-1, 256)[row, 9] = 5.0e4
    ref = _k6_ref(d, shape, gy=gy)
    dx = ops.bwd_apply(a['gy'], a['x'], a['mu'], a['At'], a['S'], a['gm'], a['st'], scales=scales)
    got = dx.cpu().numpy().reshape(ref.shape)
    return dict(finite=bool(np.isfinite(got).all()), all=rel(got, ref), other_rows=_rest(got, ref, row))


@pytest.mark.parametrize("which", ["affine_ring_kernel", "onepass_ring_kernel"])
def test_an_out_of_range_element_in_the_last_tile_of_a_full_schedule(which):
    """`all`: the suite's measure (the redone row carries the maximum); `other_rows`: the same bound on everything else -- the rest of the
    workgroup's five tiles, redone in fp32 (256 fused multiply-adds of terms ~1/16 of max |y|: ~1e-7), and every other workgroup"""
    from wc_gan_amd import ops
    errs = (_overflow_k3 if which == RING else _overflow_k6)(ops)
    print("apply dispatch overflow", which, errs)
    assert errs['finite'] and errs['all'] < K3_TOL and errs['other_rows'] < K3_TOL, errs


if __name__ == '__main__':
    from wc_gan_amd import ops as _ops

    def _fmt(e):
        return '  '.join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in e.items())

    def _cols(p):
        return f"{p['kernel']:<21}{p['ntiles']:>6}{p['grid']:>6}  {str(p['counts']):<20}{p['idle']:>5}{str(p['straddle']):>9}"

    head = f"{'row':<24}{'kernel':<21}{'tiles':>6}{'grid':>6}  {'{tiles/wg: wgs}':<20}{'idle':>5}{'straddle':>9}  errors against float64"
    print("K3 on fp32 (ops.apply(plan=); y_mask / mask_exact: want_mask; planes / maxima: ops.apply_planes against the fp32 output, maxima written)\n" + head)
    for r in RING_ROWS:
        errs, p, _ = _ring_row(_ops, r[0], r[1])
        print(f"{row_id(r):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nK3 on planes (ops.apply_split against float64 on what the planes hold)\n" + head)
    for r in SPLIT_ROWS:
        errs, p, _ = _split_row(_ops, r[0], r[1])
        print(f"{row_id(r):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nK6 in one pass (ops.bwd_apply(scales=); bits: relu_mask=; xsplit: ops.bwd_apply_xsplit; idle: workgroup pairs)\n" + head)
    for r in ONEPASS_ROWS:
        errs, p, _ = _onepass_row(_ops, r[0], r[1], r[3])
        print(f"{row_id(r):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nK6 in two passes (the class is the accumulating pass's, shared table)\n" + head)
    for r in ACC_ROWS:
        errs, p, _ = _acc_row(_ops, r[0], r[1], r[2])
        print(f"{row_id(r) + (' scales' if r[2] else ''):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nK6 on planes at C = 128 with a slot table (scaled: ops.bwd_apply(scales=) of the same inputs; taken: wc_bwd_xsplit_supported)\n" + head)
    for r in XSPLIT128_ROWS:
        errs, p, _ = _xsplit128_row(_ops, r[0], r[1])
        print(f"{row_id(r):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nrows_gemm_kernel (fast=False; tiles = row blocks, {rows of a block: blocks})\n" + head)
    for r in GEMM_ROWS:
        errs, p, _ = _gemm_row(_ops, r[0], r[1])
        print(f"{row_id(r):<24}{_cols(p)}  {_fmt(errs)}")
    print("\nan out-of-range element in the last tile of a 5-tile workgroup")
    print(f"{'K3 129x16x16x256-Kc3':<24}{_fmt(_overflow_k3(_ops))}")
    print(f"{'K6 129x8x8x256-Kc3':<24}{_fmt(_overflow_k6(_ops))}")
