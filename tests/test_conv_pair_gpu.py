"""One layer's backward in two launches (csrc/wc_conv.hip: conv_bwd_pair_kernel + conv_pair_reduce_kernel behind wc_conv_bwd_pair_f16x3)
against the four launches it replaces: dx, dW and db must have the BITS of wc_conv_f16x3 + wc_conv_wrw_bias_f16x3 on the same planes and
images -- every workgroup runs the same body on the same operands and the reductions keep their order -- and match torch's float64
gradients within tests/test_conv_gpu.py's bounds (dW 2e-5, as in tests/test_conv_dispatch_gpu.py).  Outputs and both workspaces are
NaN-filled and guard-banded before every call (tests/_poison.py)."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _poison import Poison
from test_conv_dispatch_gpu import _kernel_names, _ref3
from test_conv_gpu import TOL, _rel, _weights

# name: kind, N, H, W, k, contiguous-format weight -- the smallest shapes that reach each branch (128 -> 128)
CASES = {
    'a': ('same', 8, 8, 8, 3, False),       # data gradient k-split 8; 16 chunks of 32 points: one chunk per pixel range
    'b': ('same', 16, 32, 32, 3, False),    # 128 tiles: no k-split, <2,2,false>
    'c': ('same', 8, 8, 8, 1, False),       # one weight slice; 4 iterations: no k-split on 4 tiles
    'd': ('down3', 8, 16, 16, 3, False),    # phase data gradient, k-split over the phases' 16 iterations
    'e': ('same', 32, 6, 10, 3, False),     # H != W, W no power of two, 15 tiles
    'f': ('same', 2, 8, 8, 3, True),        # contiguous-format weight: the weight gradient with x_cols == false
    'g': ('down', 8, 16, 16, 4, False),     # the plain 4x4 stride-2 layer, the third kind the predicate admits: 16 weight slices, phase data gradient
}
_cache = {}


def _setup(name):
    """inputs, planes, images and the float64 gradients of a case: built once, shared, never written to"""
    if name in _cache:
        return _cache[name]
    from wc_gan_amd import conv as C
    kind, N, H, W, k, contiguous = CASES[name]
    torch.manual_seed(N + H + k)
    x = torch.randn(N, H, W, 128, device='cuda') * 1.7 + 0.3
    w = _weights('same', 128, 128, k, channels_last=not contiguous)
    b = torch.randn(128, device='cuda') * 0.1
    plan = C._plan(kind, x, w)
    assert plan and plan.ok and plan.pair, name
    assert w.stride(1) == (k * k if contiguous else 1) or k == 1
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    if kind == 'down':
        y64 = F.conv2d(x64.permute(0, 3, 1, 2), w64, b64, stride=2, padding=1).permute(0, 2, 3, 1)
    else:
        y64 = _ref3(x64, w64, b64, kind)
    gy = torch.randn(y64.shape, device='cuda')
    ref = torch.autograd.grad(y64, (x64, w64, b64), gy.double())
    xp = C.split_planes(x)
    gp = C.split_planes(gy, colsum=True)
    image = C.weight_image_pair(w, plan.fwd, plan.bwd)[1]
    torch.cuda.synchronize()
    _cache[name] = dict(kind=kind, x=x, w=w, b=b, gy=gy, plan=plan, xp=xp, gp=gp, image=image, ref=ref)
    return _cache[name]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _outputs(s, with_db):
    """dx, dW, db and the two workspaces -- allocated inside a Poison context: NaN-filled, the contiguous ones guard-banded"""
    plan, w = s['plan'], s['w']
    gb = plan.bwd[0]
    dx = torch.empty((gb.N, gb.Hout, gb.Wout, gb.Cout), dtype=torch.float32, device='cuda')
    dw = torch.empty_like(w)
    db = torch.empty(128, dtype=torch.float32, device='cuda') if with_db else None
    ws_dx = torch.empty(plan.bwd_ws, dtype=torch.uint8, device='cuda') if plan.bwd_ws else None
    ws_dw = torch.empty(plan.wrw_ws, dtype=torch.uint8, device='cuda')
    assert dw.stride() == w.stride()
    return dx, dw, db, ws_dx, ws_dw


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call_two(s, with_db, out):
    from wc_gan_amd import _lib, conv as C
    lib = _lib.load()
    plan, w = s['plan'], s['w']
    (gh, gl, gs, colsum), (xh, xl, xs), (img, wsc) = s['gp'], s['xp'], s['image']
    dx, dw, db, ws_dx, ws_dw = out
    _, kf, nf = plan.fwd
    zero = C._zero_line(gh.device)
    _lib.check(lib.wc_conv_f16x3(_p(gh), _p(gl), _p(gs), _p(img), _p(wsc), None, _p(zero), plan.bwd_ptr, 0, _p(dx), _p(ws_dx), plan.bwd_ws,
                                 _stream()), "wc_conv_f16x3")
    _lib.check(lib.wc_conv_wrw_bias_f16x3(_p(xh), _p(xl), _p(xs), _p(gh), _p(gl), _p(gs), _p(zero), plan.fwd_ptr, _p(dw), w.stride(kf),
                                          w.stride(nf), w.stride(2), w.stride(3), _p(colsum) if with_db else None, _p(db), _p(ws_dw),
                                          plan.wrw_ws, _stream()), "wc_conv_wrw_bias_f16x3")


def _call_pair(s, with_db, out):
    from wc_gan_amd import _lib, conv as C
    lib = _lib.load()
    plan, w = s['plan'], s['w']
    (gh, gl, gs, colsum), (xh, xl, xs), (img, wsc) = s['gp'], s['xp'], s['image']
    dx, dw, db, ws_dx, ws_dw = out
    _, kf, nf = plan.fwd
    zero = C._zero_line(gh.device)
    _lib.check(lib.wc_conv_bwd_pair_f16x3(_p(gh), _p(gl), _p(gs), _p(img), _p(wsc), _p(zero), plan.bwd_ptr, _p(dx), _p(ws_dx), plan.bwd_ws,
                                          _p(xh), _p(xl), _p(xs), plan.fwd_ptr, _p(dw), w.stride(kf), w.stride(nf), w.stride(2), w.stride(3),
                                          _p(colsum) if with_db else None, _p(db), _p(ws_dw), plan.wrw_ws, _stream()),
               "wc_conv_bwd_pair_f16x3")


def _run(s, with_db, call):
    """one poisoned call -> (dx, dW, db | None), guards checked"""
    with Poison(0xFF) as P:
        out = _outputs(s, with_db)
        assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[1]).all())
        call(s, with_db, out)
        P.check_guards()
        res = tuple(None if t is None else t.clone() for t in out[:3])
        P.release()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("with_db", [True, False], ids=['colsum-db', 'no-db'])
@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_has_the_bits_of_the_two_entries_and_matches_float64(name, with_db):
    s = _setup(name)
    two = _run(s, with_db, _call_two)
    pair = _run(s, with_db, _call_pair)
    dx64, dw64, db64 = s['ref']
    errs = dict(dx=_rel(pair[0], dx64), dw=_rel(pair[1], dw64), db=_rel(pair[2], db64) if with_db else 0.0)
    print("conv pair", name, CASES[name], "with db" if with_db else "no db", errs)
    assert torch.equal(pair[0], two[0]), "dx"
    assert torch.equal(pair[1], two[1]), "dW"
    assert pair[1].stride() == s['w'].stride()
    if with_db:
        assert torch.equal(pair[2], two[2]), "db"
    else:
        assert pair[2] is None and two[2] is None
    assert errs['dx'] < TOL and errs['db'] < TOL, errs
    assert errs['dw'] < 2e-5, errs


@pytest.mark.gpu
def test_a_captured_pair_replays_the_eager_bits():
    s = _setup('a')
    eager = _run(s, True, _call_pair)
    out = _outputs(s, True)
    _call_pair(s, True, out)                    # (the kernels' LDS attribute is set outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call_pair(s, True, out)
    for _ in range(2):
        for t in out:
            t.fill_(float('nan') if t.is_floating_point() else 0xFF)
        g.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(out[:3], eager, ('dx', 'dW', 'db')):
            assert torch.equal(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ['a', 'b'])
def test_the_layer_takes_the_pair_and_returns_its_bits(name):
    """fast_conv + autograd.grad: the gradients are those of the two entries at the C ABI, and the backward launches conv_bwd_pair_kernel
    in place of conv_f16x3_kernel and conv_wrw_kernel"""
    from wc_gan_amd import conv as C
    s = _setup(name)
    two = _run(s, True, _call_two)
    x, w, b = (t.clone().requires_grad_(True) for t in (s['x'], s['w'], s['b']))
    assert w.stride() == s['w'].stride()
    y = C.fast_conv(x, w, b, s['kind'])
    grads = torch.autograd.grad(y, (x, w, b), s['gy'])
    for got, want, what in zip(grads, two, ('dx', 'dW', 'db')):
        assert torch.equal(got, want), what
    y = C.fast_conv(x, w, b, s['kind'])
    names = _kernel_names(lambda: torch.autograd.grad(y, (x, w, b), s['gy']))
    if not names:
        pytest.skip("this profiler build reports no device kernel names: the launch was not checked (the bit comparison ran)")
    joined = ' '.join(names)
    assert 'conv_bwd_pair_kernel' in joined, names
    assert 'conv_wrw_kernel' not in joined and 'conv_f16x3_kernel' not in joined, names
    assert ('conv_pair_reduce_kernel' in joined) == (s['plan'].bwd_ws > 0), names


_CONV_KERNELS = ('conv_bwd_pair_kernel', 'conv_pair_reduce_kernel', 'conv_f16x3_kernel', 'conv_ksplit_reduce_kernel', 'conv_wrw_kernel',
                 'conv_wrw_reduce_kernel')


@pytest.mark.gpu
def test_the_shortcut_on_planes_takes_the_pair_and_adds_no_launch():
    """conv.split_conv (the 1x1 shortcut on the residual add's pre-split planes) on a 128 -> 128 layer, with a bias: dx, dW and db have the
    bits of the same backward on a plan that does not pair, and apart from the convolution kernels themselves the two backwards launch the
    same kernels -- the bias gradient comes out of the weight reduction once, no torch reduction beside it"""
    from wc_gan_amd import conv as C
    from wc_gan_amd.functional import residual_add, split_of
    torch.manual_seed(5)
    N, H, W = 8, 8, 8
    h = torch.randn(N, H, W, 128, device='cuda', requires_grad=True)
    s = torch.randn(N, H // 2, W // 2, 128, device='cuda', requires_grad=True)
    w = _weights('same', 128, 128, 1).requires_grad_(True)
    b = (torch.randn(128, device='cuda') * 0.1).requires_grad_(True)
    gy = torch.randn(N, H, W, 128, device='cuda')
    x = residual_add(h, s, True, planes=True, x32=False)
    st = split_of(x)
    assert st is not None
    plan = C._plan('same', x, w)
    assert plan and plan.ok and plan.pair
    single = copy.copy(plan)
    single.pair = False

    def backward(p):
        """-> (gradients, device kernel names of the backward) of the shortcut on plan p"""
        y = C._SplitConv.apply(x, w, b, p, st, None)
        grads = []
        names = _kernel_names(lambda: grads.extend(torch.autograd.grad(y, (h, s, w, b), gy, retain_graph=True)))
        return grads, names

    (pair, names_pair), (two, names_two) = backward(plan), backward(single)
    assert len(pair) == len(two) == 4
    for got, want, what in zip(pair, two, ('dh', 'ds', 'dW', 'db')):
        assert torch.equal(got, want), what
    if not names_pair:
        pytest.skip("this profiler build reports no device kernel names: the launches were not checked (the bit comparison ran)")
    others = [sorted(n for n in names if not any(k in n for k in _CONV_KERNELS)) for names in (names_pair, names_two)]
    assert others[0] == others[1], (names_pair, names_two)
    assert sum('conv_bwd_pair_kernel' in n for n in names_pair) == 1, names_pair
    assert not any('conv_wrw_kernel' in n or 'conv_f16x3_kernel' in n for n in names_pair), names_pair
    assert not any('conv_bwd_pair_kernel' in n for n in names_two), names_two
