"""The narrow (image-layer) convolution kernels of csrc/wc_conv.hip at every k-step class, tile, grid and pixel-range edge of their host
plans against NumPy float64 direct sums: conv_fwd_narrow_kernel<2|5|10|14|16> (with and without the ReLU, straight and mirrored),
conv_fwd_narrow_split_kernel, conv_wrw_narrow_kernel, conv_wrw_narrow_masked_kernel and conv_wrw_narrow_reduce_kernel through
wc_conv_fwd_narrow_f32, wc_conv_fwd_narrow_split_f32, wc_conv_wrw_narrow64_f32, wc_conv_wrw_narrow_f32 and wc_conv_wrw_narrow_masked_f32.

Rows, their class literals, inputs and references live in tests/narrow_reference.py; tests/test_narrow_edges.py holds the literals to
the library.  Bounds (max |error| over max |reference|): y and the mirrored data gradient 1e-5, dW and db 2e-6 --
test_narrow_input_weight_gradient_against_float64's.  The split variant and the masked gradient are held to the BITS of the launches
they replace by tests/test_first_block_gpu.py's own checkers.

    PYTHONPATH=. python tests/test_narrow_edges_gpu.py          # the table of profiles/narrow_parity.txt"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import narrow_reference as R
from _poison import run_patterns, same_bits
from test_conv_dispatch_gpu import _instantiations, _kernel_names
from test_first_block_gpu import _check_masked_gradient, _check_split_forward

pytestmark = pytest.mark.gpu

WC_ERR_SHAPE = -2


def _names(rows):
    return [r.name for r in rows]


def _dev(a, fmt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else t


def _tensors(row):
    x, w, b, gy, h = R.inputs(row)
    return _dev(x), _dev(w, row.fmt), (None if b is None else _dev(b)), _dev(gy), _dev(h)


def _gradients(entry, x, gy, w, has_bias, mask=None):
    """One of the three weight-gradient entries on buffers of the test's own: -> (return code, dW in w's strides, db | None).  A weight in
    contiguous format gets its dW from torch.empty, which tests/_poison.py places between guard bands."""
    from wc_gan_amd import _lib
    from wc_gan_amd.ops import _ptr, _stream
    lib = _lib.load()
    N, H, W, C = x.shape
    O, k = w.shape[0], w.shape[2]
    dw = torch.empty(w.shape, dtype=torch.float32, device='cuda') if w.is_contiguous() else \
        torch.empty_strided(w.shape, w.stride(), dtype=torch.float32, device='cuda')
    db = torch.empty(O, dtype=torch.float32, device='cuda') if has_bias else None
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(N, H, W, C, O, k)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device='cuda')
    strides = (dw.stride(1), dw.stride(0), dw.stride(2), dw.stride(3))
    if mask is None:
        code = getattr(lib, entry)(_ptr(x), _ptr(gy), N, H, W, C, O, k, _ptr(dw), *strides, _ptr(db), _ptr(ws), ws.numel(), _stream())
    else:
        code = lib.wc_conv_wrw_narrow_masked_f32(_ptr(x), _ptr(gy), _ptr(mask), N, H, W, C, O, k, _ptr(dw), *strides, _ptr(db), _ptr(ws),
                                                 ws.numel(), _stream())
    return code, dw, db


def _rel(a, r):
    return R.rel(a.detach().cpu().numpy(), r)


def _measure(row):
    """-> (errors of the HIP kernels against float64, the same of torch's fp32 convolution on the same inputs).  Asserts what is no matter
    of precision: the same bits on a second call, dW in the weight's strides, the two weight-gradient entries' agreement, no db without
    a bias, the 128-multiple entry's refusal of 64 and 192 outputs."""
    from wc_gan_amd import conv as C
    x, w, b, gy, _ = _tensors(row)
    ref = R.reference(row.name)
    assert C.narrow_wrw_supported(x, w) and C.narrow_shapes_supported(tuple(x.shape), tuple(w.shape))
    hip = {}
    y, yr = C.narrow_forward(x, w, b), C.narrow_forward(x, w, b, relu=True)
    assert same_bits(y, C.narrow_forward(x, w, b)) and same_bits(yr, C.narrow_forward(x, w, b, relu=True))
    assert torch.equal(yr, torch.relu(y)) and bool((yr == 0).any()) and bool((yr > 0).any())          # fmaxf(v, 0) on the value the plain call stores
    hip['y'], hip['relu'] = _rel(y, ref['y']), _rel(yr, ref['relu'])
    dw, db = C.narrow_gradients(x, gy, w, row.bias)
    code, dw2, db2 = _gradients('wc_conv_wrw_narrow64_f32', x, gy, w, row.bias)
    assert code == 0 and dw.stride() == w.stride() == dw2.stride() and same_bits(dw, dw2)
    assert (db is None and db2 is None and not row.bias) or same_bits(db, db2)
    hip['dw'] = _rel(dw, ref['dw'])
    hip['db'] = _rel(db, ref['db']) if row.bias else 0.0
    code, dw3, db3 = _gradients('wc_conv_wrw_narrow_f32', x, gy, w, row.bias)
    if row.Cout % 128 == 0:
        assert code == 0 and dw3.stride() == w.stride() and same_bits(dw3, dw) and (not row.bias or same_bits(db3, db))
    else:
        assert code == WC_ERR_SHAPE
    # torch's fp32 convolution of the same inputs, for the record
    xt = x.permute(0, 3, 1, 2)
    wt = w.detach().clone().requires_grad_(True)
    bt = None if b is None else b.detach().clone().requires_grad_(True)
    y32 = F.conv2d(xt, wt, bt, padding=row.k // 2)
    g32 = torch.autograd.grad(y32, (wt,) + (() if bt is None else (bt,)), gy.permute(0, 3, 1, 2))
    y32 = y32.permute(0, 2, 3, 1)
    ref32 = dict(y=_rel(y32, ref['y']), relu=_rel(torch.relu(y32), ref['relu']), dw=_rel(g32[0], ref['dw']),
                 db=_rel(g32[1], ref['db']) if row.bias else 0.0)
    return hip, ref32


def _within(errs):
    return errs['y'] < R.Y_BOUND and errs['relu'] < R.Y_BOUND and errs['dw'] < R.DW_BOUND and errs['db'] < R.DW_BOUND


# ---- a. every row against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names(R.ROWS))
def test_forward_relu_and_gradients_of_a_row_match_float64(name):
    row = R.by_name(name)
    hip, t32 = _measure(row)
    print("narrow", name, row.label(), "hip", hip, "torch fp32", t32)
    assert _within(hip), (hip, t32)


@pytest.mark.parametrize("name", _names(R.ROWS + R.MIRROR_ROWS))
def test_the_forward_instantiation_is_the_rows(name):
    from wc_gan_amd import conv as C
    row = R.by_name(name)
    if row in R.MIRROR_ROWS:
        _, w, gy = R.mirror_inputs(row)
        w, gy = _dev(w, 'channels_last'), _dev(gy)
        names = _kernel_names(lambda: C.narrow_forward(gy, w, None, mirrored=True))
    else:
        x, w, b, _, _ = _tensors(row)
        names = _kernel_names(lambda: C.narrow_forward(x, w, b))
    if not names:
        pytest.skip("this profiler build reports no device kernel names: the instantiation was not checked (the parity assertions ran)")
    assert _instantiations(names, 'conv_fwd_narrow_kernel') == [f'<{row.inst}>'], names


# ---- b. the generator's last layer: the mirrored forward and the exchanged weight gradient ------------------------------------------
def _mirror_measure(row, fmt):
    from wc_gan_amd import conv as C
    x, w, gy = R.mirror_inputs(row)
    ref = R.mirror_reference(row.name)
    x, w, gy = _dev(x), _dev(w, fmt), _dev(gy)
    dx = C.narrow_forward(gy, w, None, mirrored=True)
    assert dx.shape == x.shape and same_bits(dx, C.narrow_forward(gy, w, None, mirrored=True))
    errs = dict(dx=_rel(dx, ref['dx']), dw=0.0)
    if row.Cout % 128 == 0:
        assert C.narrow_out_wrw_supported(x, w)
        dw = C.narrow_out_weight_gradient(x, gy, w)
        assert dw.stride() == w.stride() and same_bits(dw, C.narrow_out_weight_gradient(x, gy, w))
        errs['dw'] = _rel(dw, ref['dw'])
    else:           # the exchanged gradient's entry takes the wide side in 128s: the layer keeps torch's weight gradient
        assert not C.narrow_out_wrw_supported(x, w)
    # torch's fp32 gradients of the same layer
    xt, wt = x.permute(0, 3, 1, 2).detach().requires_grad_(True), w.detach().clone().requires_grad_(True)
    g32 = torch.autograd.grad(F.conv2d(xt, wt, None, padding=row.k // 2), (xt, wt), gy.permute(0, 3, 1, 2))
    return errs, dict(dx=_rel(g32[0].permute(0, 2, 3, 1), ref['dx']), dw=_rel(g32[1], ref['dw']))


@pytest.mark.parametrize("name", _names(R.MIRROR_ROWS))
def test_mirrored_forward_and_exchanged_weight_gradient_match_float64(name):
    row = R.by_name(name)
    for fmt in ('channels_last', 'contiguous'):
        hip, t32 = _mirror_measure(row, fmt)
        print("narrow mirrored", name, fmt, row.label(), "hip", hip, "torch fp32", t32)
        assert hip['dx'] < R.Y_BOUND and hip['dw'] < R.DW_BOUND, (fmt, hip, t32)


# ---- c. the masked weight gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names([r for r in R.ROWS if 'pixel' in r.tags or 'o192' in r.tags]))
def test_masked_weight_gradient_has_the_bits_of_the_masked_copy_at_the_range_edges(name):
    row = R.by_name(name)
    x, w, _, gy, h = _tensors(row)
    _check_masked_gradient(x, gy, h, w)
    ref = R.reference(name)
    code, dw, db = _gradients(None, x, gy, w, True, mask=h)
    assert code == 0 and _rel(dw, ref['mdw']) < R.DW_BOUND and _rel(db, ref['mdb']) < R.DW_BOUND


# ---- d. the split forward -----------------------------------------------------------------------------------------------------------
_SPLIT_ROWS = R.tagged('kstep') + R.tagged('partial') + [r for r in R.GATE_ROWS if r.split and r.M * r.Cout <= 32800 * 256]


@pytest.mark.parametrize("name", _names(_SPLIT_ROWS))
def test_split_forward_leaves_y_planes_scale_and_record_at_the_rows(name):
    row = R.by_name(name)
    _check_split_forward(row.shape + (row.Cin,), row.Cout, row.k)


def _sentinels(*shapes_dtypes):
    out = []
    for shape, dtype in shapes_dtypes:
        t = torch.empty(shape, dtype=dtype, device='cuda')
        t.view(torch.uint8).fill_(0x5A)
        out.append(t)
    return out


@pytest.mark.parametrize("name", _names([r for r in R.GATE_ROWS if not r.split]))
def test_a_declined_split_shape_launches_nothing(name):
    from wc_gan_amd import _lib, conv as C
    from wc_gan_amd.ops import _ptr, _stream
    row = R.by_name(name)
    N, H, W = row.shape
    xshape, wshape = row.shape + (row.Cin,), (row.Cout, row.Cin, row.k, row.k)
    assert C.narrow_shapes_supported(xshape, wshape) and not C.narrow_split_supported(xshape, wshape)
    assert C.first_block_route(xshape, wshape, [torch.zeros(C.HIST_FLOATS, device='cuda'), True]) == 'two'
    x, w = torch.zeros(xshape, device='cuda'), torch.zeros(wshape, device='cuda')
    y, hi, lo, scale, hist = outs = _sentinels((row.shape + (row.Cout,), torch.float32), (row.shape + (row.Cout,), torch.float16),
                                               (row.shape + (row.Cout,), torch.float16), ((513,), torch.float32), ((C.HIST_FLOATS,), torch.float32))
    code = _lib.load().wc_conv_fwd_narrow_split_f32(_ptr(x), _ptr(w), w.stride(1), w.stride(0), w.stride(2), w.stride(3), None, N, H, W, row.Cin,
                                                    row.Cout, row.k, 1, 0.0, _ptr(y), _ptr(hi), _ptr(lo), _ptr(scale), _ptr(hist), 0, _stream())
    torch.cuda.synchronize()
    assert code == WC_ERR_SHAPE
    for t in outs:
        assert bool((t.view(torch.uint8) == 0x5A).all())


# ---- e. a one-pixel-wide image -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.W1_GEOMS[:3], ids=lambda g: 'x'.join(map(str, g)))
def test_a_one_pixel_wide_image_is_declined_and_nothing_is_written(geom):
    from wc_gan_amd import _lib, conv as C
    from wc_gan_amd.ops import _ptr, _stream
    lib = _lib.load()
    N, H, W, ci, co, k = geom
    x, w = torch.randn(N, H, W, ci, device='cuda'), torch.randn(co, ci, k, k, device='cuda')
    assert not C.narrow_wrw_supported(x, w) and not C.narrow_shapes_supported(tuple(x.shape), tuple(w.shape))
    assert not C.narrow_split_supported(tuple(x.shape), tuple(w.shape))
    y, dw, db, ws = outs = _sentinels(((N, H, W, co), torch.float32), (tuple(w.shape), torch.float32), ((co,), torch.float32), ((1 << 16,), torch.uint8))
    gy = torch.randn(N, H, W, co, device='cuda')
    strides = (dw.stride(1), dw.stride(0), dw.stride(2), dw.stride(3))
    assert lib.wc_conv_fwd_narrow_f32(_ptr(x), _ptr(w), *strides, None, N, H, W, ci, co, k, 0, _ptr(y), _stream()) == WC_ERR_SHAPE
    for entry in (lib.wc_conv_wrw_narrow64_f32, lib.wc_conv_wrw_narrow_f32):
        assert entry(_ptr(x), _ptr(gy), N, H, W, ci, co, k, _ptr(dw), *strides, _ptr(db), _ptr(ws), ws.numel(), _stream()) == WC_ERR_SHAPE
    assert lib.wc_conv_wrw_narrow_masked_f32(_ptr(x), _ptr(gy), _ptr(gy), N, H, W, ci, co, k, _ptr(dw), *strides, _ptr(db), _ptr(ws), ws.numel(),
                                             _stream()) == WC_ERR_SHAPE
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("k", [3, 1])
def test_conv2d_on_a_one_pixel_wide_image_takes_torchs_route_and_matches_float64(k):
    """generator.Conv2D on (N, H, 1, 3): before wc_conv_narrow64_supported declined W < 2 the narrow kernels took this layer and wrote
    little more than the bias to every pixel below the first row."""
    from wc_gan_amd import conv as C
    from wc_gan_amd.generator import Conv2D
    torch.manual_seed(21)
    layer = Conv2D(3, 128, (k, k)).cuda()
    with torch.no_grad():
        layer.conv.bias.copy_(torch.randn(128) * 0.5)
    x = (torch.randn(2, 5, 1, 3, device='cuda') * 0.7 + 0.1).requires_grad_(True)
    w, b = layer.conv.weight, layer.conv.bias
    assert not C.narrow_wrw_supported(x, w) and not C.supported(x, w, 'same')
    out = {}

    def fwd():
        out['y'] = layer(x)
    names = _kernel_names(fwd)
    assert not [n for n in names if 'narrow' in n], names
    y = out['y']
    gy = torch.randn_like(y)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gy)
    xn, wn, bn, gn = (t.detach().cpu().numpy() for t in (x, w, b, gy))
    dw64, db64 = R.gradients(xn, gn, k)
    assert y.shape == (2, 5, 1, 128)
    assert _rel(y, R.forward(xn, wn, bn)) < R.Y_BOUND and _rel(dx, R.mirrored_forward(gn, wn)) < R.Y_BOUND
    assert _rel(dw, dw64) < R.Y_BOUND and _rel(db, db64) < R.Y_BOUND          # (torch's own kernels: the suite's fp32 convolution level)


# ---- f. poisoned memory --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['M2', 'M31', 'M33', 'M32800', 'M33-o192', 'M16385-o192'])
def test_forward_and_gradients_on_poisoned_guarded_buffers(name):
    """Guard bands around x, w, b, gy, the mask, y, dW (contiguous format), db and the partial sums; the same bits whatever the fresh buffers
    held -- the clamped loads of a partial tile, the idle half group of 192 outputs and the waves behind the last pixel leave nothing."""
    from wc_gan_amd import conv as C
    row = R.by_name(name)
    x, w, b, gy, h = R.inputs(row)
    ref = R.reference(name)

    def call(P):
        xd, wd, bd, gd, hd = (P.guarded(a) for a in (x, w, b, gy, h))
        out = dict(y=C.narrow_forward(xd, wd, bd), relu=C.narrow_forward(xd, wd, bd, relu=True))
        code, out['dw'], out['db'] = _gradients('wc_conv_wrw_narrow64_f32', xd, gd, wd, True)
        code2, out['mdw'], out['mdb'] = _gradients(None, xd, gd, wd, True, mask=hd)
        assert code == 0 and code2 == 0
        return out
    outs = run_patterns(call)
    for o in outs.values():
        assert R.rel(o['y'].numpy(), ref['y']) < R.Y_BOUND and R.rel(o['relu'].numpy(), ref['relu']) < R.Y_BOUND
        for n in ('dw', 'db', 'mdw', 'mdb'):
            assert R.rel(o[n].numpy(), ref[n]) < R.DW_BOUND, n


def test_mirrored_forward_and_exchanged_gradient_on_poisoned_guarded_buffers():
    from wc_gan_amd import conv as C
    row = R.by_name('3x6x10-c3-F256')
    x, w, gy = R.mirror_inputs(row)
    ref = R.mirror_reference(row.name)

    def call(P):
        xd, wd, gd = P.guarded(x), P.guarded(w), P.guarded(gy)
        return dict(dx=C.narrow_forward(gd, wd, None, mirrored=True), dw=C.narrow_out_weight_gradient(xd, gd, wd))
    for o in run_patterns(call).values():
        assert R.rel(o['dx'].numpy(), ref['dx']) < R.Y_BOUND and R.rel(o['dw'].numpy(), ref['dw']) < R.DW_BOUND


if __name__ == '__main__':
    keys = ('y', 'relu', 'dw', 'db')
    print(f"{'row':<22}{'class':<78}{'route':<12}" + ''.join(f"{k:>10}" for k in keys))
    worst = dict.fromkeys(keys, 0.0)
    for row in R.ROWS:
        hip, t32 = _measure(row)
        for route, e in (('hip', hip), ('torch fp32', t32)):
            print(f"{row.name:<22}{row.label() if route == 'hip' else '':<78}{route:<12}" + ''.join(f"{e[k]:>10.2e}" for k in keys))
        worst = {k: max(worst[k], hip[k]) for k in keys}
    print(f"{'maximum':<22}{'':<78}{'hip':<12}" + ''.join(f"{worst[k]:>10.2e}" for k in keys))
    print()
    print(f"{'mirrored row':<22}{'class':<78}{'route':<12}{'format':<16}{'dx':>10}{'dw':>10}")
    worst = dict(dx=0.0, dw=0.0)
    for row in R.MIRROR_ROWS:
        for fmt in ('channels_last', 'contiguous'):
            hip, t32 = _mirror_measure(row, fmt)
            for route, e in (('hip', hip), ('torch fp32', t32)):
                dw = f"{e['dw']:>10.2e}" if (route != 'hip' or row.Cout % 128 == 0) else f"{'torch':>10}"
                print(f"{row.name:<22}{row.label() if route == 'hip' else '':<78}{route:<12}{fmt:<16}{e['dx']:>10.2e}{dw}")
            worst = {k: max(worst[k], hip[k]) for k in worst}
    print(f"{'maximum':<22}{'':<78}{'hip':<12}{'':<16}{worst['dx']:>10.2e}{worst['dw']:>10.2e}")
