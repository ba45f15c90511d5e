"""The generator's last layer on the narrow kernels (csrc/wc_conv.hip conv_narrow_out_kernel<., true>,
conv_wrw_narrow32_kernel + conv_wrw_narrow32_reduce_kernel, conv_fwd_narrow32_kernel through wc_conv_narrow_out_bias_f32,
wc_conv_wrw_narrow32_f32, wc_conv_fwd_narrow32_f32) against the float64 direct sums of tests/narrow_last_reference.py:

  kernels   every row in both weight memory formats: y without and with the bias (BOUND), dx (Y_BOUND), dW (DW_BOUND); the same bits on a
            second call; at the 64-wide row the bits of the entries that were there; y with a bias = y without + b in fp32, bit for bit;
            declined shapes launch nothing; three rows on poisoned, guard-banded memory
  layer     a marked Conv2D(32, 3) and a marked Conv2D(96, 2, (1, 1)): y, dx, dW, db, a forward under no_grad, a call whose input needs
            no gradient
  network   a cut-down generator (128, 64, 32 from 4 x 4, slim_conv on, batch 8) marked against unmarked: identical ReLU masks, image and
            every parameter gradient within 2e-5 of the tensor's maximum, the marked pass against tests/generator_reference.py on those
            masks (tests/test_generator_gpu.py's BOUNDS); a profiled marked pass; a captured and replayed one

    PYTHONPATH=. python tests/test_narrow_last_gpu.py          # the table of profiles/narrow_last_parity.txt"""
import copy

import numpy as np
import pytest
import torch

import narrow_last_reference as R
from _poison import run_patterns, same_bits

pytestmark = pytest.mark.gpu

WC_ERR_SHAPE = -2
FORMATS = ('contiguous', 'channels_last')
TWO_ROUTES = 2e-5           # image and parameter gradients of two routes through one network (tests/test_handoff_gpu.py, tests/test_conv_gpu.py)


def _dev(a, fmt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else t


def _passes(x, w, b, gy):
    """the three launches and the forward without its bias, as conv._NarrowLastConv issues them"""
    from wc_gan_amd import conv as C
    return dict(y0=C.narrow_out_conv(x, w, forward=True), y=C.narrow_out_conv(x, w, forward=True, bias=b),
                dx=C.narrow_forward(gy, w, None, mirrored=True, wide32=True), dw=C.narrow_out_weight_gradient(x, gy, w, wide32=True))


def _measure(row, fmt):
    """-> {key: error against float64}; asserts shapes, strides and the same bits on a second call"""
    from wc_gan_amd import conv as C
    x, w, b, gy = R.inputs(row)
    ref = R.reference(row.name)
    xd, wd, bd, gd = _dev(x), _dev(w, fmt), _dev(b), _dev(gy)
    assert C.narrow_last_supported(tuple(xd.shape), tuple(wd.shape))
    got, again = _passes(xd, wd, bd, gd), _passes(xd, wd, bd, gd)
    assert got['y'].shape == gy.shape and got['dx'].shape == x.shape and got['dw'].shape == w.shape and got['dw'].stride() == wd.stride()
    for key in got:
        assert same_bits(got[key], again[key]), key
    # with a bias: the bits of the launch without one followed by one fp32 add
    assert same_bits(got['y'], got['y0'] + bd), "bias"
    return {key: R.rel(got[key].cpu().numpy(), ref[key]) for key in got}


def _assert_bounds(errs):
    assert errs['y0'] < R.BOUND and errs['y'] < R.BOUND and errs['dx'] < R.Y_BOUND and errs['dw'] < R.DW_BOUND, errs


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", [r.name for r in R.ROWS])
def test_a_row_matches_float64_in_both_weight_formats(name, fmt):
    errs = _measure(R.by_name(name), fmt)
    print("narrow last", name, fmt, {k: f"{v:.2e}" for k, v in errs.items()})
    _assert_bounds(errs)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_64_multiple_width_has_the_bits_of_the_entries_that_were_there(fmt):
    from wc_gan_amd import _lib, conv as C
    from wc_gan_amd.ops import _ptr, _stream
    import ctypes
    lib = _lib.load()
    row = R.by_name(R.OLD_BITS_ROW)
    x, w, b, gy = R.inputs(row)
    xd, wd, bd, gd = _dev(x), _dev(w, fmt), _dev(b), _dev(gy)
    new = _passes(xd, wd, bd, gd)
    N, H, W, k = row.N, row.H, row.W, row.k
    # the exchanged weight gradient on wc_conv_wrw_narrow64_f32, called as conv.narrow_out_weight_gradient calls its entry
    dw = torch.empty_strided(wd.shape, wd.stride(), dtype=torch.float32, device='cuda')
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(N, H, W, row.Cn, row.Cw, k)
    assert nb == lib.wc_conv_wrw_narrow32_workspace_bytes(N, H, W, row.Cn, row.Cw, k) > 0
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    last = dw.data_ptr() + 4 * ((k - 1) * dw.stride(2) + (k - 1) * dw.stride(3))
    _lib.check(lib.wc_conv_wrw_narrow64_f32(_ptr(gd), _ptr(xd), N, H, W, row.Cn, row.Cw, k, ctypes.c_void_p(last), dw.stride(0), dw.stride(1),
                                            -dw.stride(2), -dw.stride(3), None, _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow64_f32")
    assert same_bits(new['dw'], dw)
    assert same_bits(new['dx'], C.narrow_forward(gd, wd, None, mirrored=True))           # wc_conv_fwd_narrow_f32
    # wc_conv_narrow_out_bias_f32 with a null bias is wc_conv_narrow_out_f32
    out = torch.empty(N, H, W, row.Cn, device='cuda')
    ptr = ctypes.c_void_p(wd.data_ptr() + 4 * ((k - 1) * wd.stride(2) + (k - 1) * wd.stride(3)))
    _lib.check(lib.wc_conv_narrow_out_bias_f32(_ptr(xd), None, ptr, wd.stride(1), wd.stride(0), -wd.stride(2), -wd.stride(3), None, N, H, W,
                                               row.Cw, row.Cn, k, _ptr(out), _stream()), "wc_conv_narrow_out_bias_f32")
    assert same_bits(out, new['y0']) and same_bits(new['y'], new['y0'] + bd)


@pytest.mark.parametrize("name", R.POISON_ROWS)
def test_on_poisoned_guarded_buffers(name):
    """guard bands around the inputs, the weight, the bias, the outputs and the weight gradient's partial sums; the same bits whatever the
    fresh buffers held: clamped loads of a partial tile, idle waves and the upper lanes of a 32-wide group leave nothing"""
    row = R.by_name(name)
    x, w, b, gy = R.inputs(row)
    ref = R.reference(name)

    def call(P):
        return _passes(*(P.guarded(a) for a in (x, w, b, gy)))
    for o in run_patterns(call).values():
        errs = {key: R.rel(val.numpy(), ref[key]) for key, val in o.items()}
        assert not any(bool(torch.isnan(v).any()) for v in o.values())
        _assert_bounds(errs)


@pytest.mark.parametrize("shape", R.DECLINED, ids=lambda s: 'x'.join(map(str, s)))
def test_a_declined_shape_launches_nothing(shape):
    from wc_gan_amd import _lib
    from wc_gan_amd.ops import _ptr, _stream
    lib = _lib.load()
    N, H, W, cn, cw, k = shape
    fill = lambda *s: torch.empty(*s, device='cuda').view(torch.uint8).fill_(0x5A).view(torch.float32)
    kept = lambda t: bool((t.view(torch.uint8) == 0x5A).all())
    x, gy, w, b = torch.randn(N, H, W, cw, device='cuda'), torch.randn(N, H, W, cn, device='cuda'), torch.randn(cn, cw, k, k, device='cuda'), \
        torch.randn(cn, device='cuda')
    y, dx, dw, ws = fill(N, H, W, cn), fill(N, H, W, cw), fill(cn, cw, k, k), fill(1 << 16)
    assert lib.wc_conv_fwd_narrow32_f32(_ptr(gy), _ptr(w), w.stride(0), w.stride(1), w.stride(2), w.stride(3), None, N, H, W, cn, cw, k, 0,
                                        _ptr(dx), _stream()) == WC_ERR_SHAPE
    assert lib.wc_conv_wrw_narrow32_f32(_ptr(gy), _ptr(x), N, H, W, cn, cw, k, _ptr(dw), dw.stride(0), dw.stride(1), dw.stride(2), dw.stride(3),
                                        None, _ptr(ws), ws.numel() * 4, _stream()) == WC_ERR_SHAPE
    assert lib.wc_conv_narrow_out_bias_f32(_ptr(x), None, _ptr(w), w.stride(1), w.stride(0), w.stride(2), w.stride(3), _ptr(b), N, H, W, cw,
                                           cn, k, _ptr(y), _stream()) == WC_ERR_SHAPE
    torch.cuda.synchronize()
    assert kept(y) and kept(dx) and kept(dw) and kept(ws)


# ---- the layer -------------------------------------------------------------------------------------------------------------------------
LAYERS = [('2x5x7-32-3-k3', (3, 3)), ('3x4x6-96-2-k1', (1, 1))]


def _layer(name, ksize):
    """a marked Conv2D of the named shape with the row's weight and bias, its inputs and the float64 reference"""
    from wc_gan_amd.generator import Conv2D
    N, H, W = (int(v) for v in name.split('-')[0].split('x'))
    cw, cn, k = int(name.split('-')[1]), int(name.split('-')[2]), ksize[0]
    row = R.Row(name, N, H, W, cw, cn, k, 1, cw // 32, 'layer')
    x, w, b, gy = R.inputs(row)
    import narrow_out_reference as NO
    import narrow_reference as NR
    ref = dict(y=NO.narrow_out(x, w, forward=True) + b.astype(np.float64), dx=NR.forward(gy, w, None, mirrored=True),
               dw=NR.exchanged_gradient(x, gy, k), db=gy.astype(np.float64).sum(axis=(0, 1, 2)))
    layer = Conv2D(cw, cn, ksize, narrow_last=True).cuda()
    with torch.no_grad():
        layer.conv.weight.copy_(_dev(w))
        layer.conv.bias.copy_(_dev(b))
    return layer, _dev(x), _dev(gy), ref


@pytest.mark.parametrize("name,ksize", LAYERS)
def test_a_marked_layer_against_float64(name, ksize, monkeypatch):
    from wc_gan_amd import conv as C
    layer, x, gy, ref = _layer(name, ksize)
    calls = []
    for fn in ('narrow_out_conv', 'narrow_forward', 'narrow_out_weight_gradient'):
        monkeypatch.setattr(C, fn, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(C, fn), fn))
    assert layer._narrow_last_route(x)
    xg = x.clone().requires_grad_(True)
    y = layer(xg)
    assert isinstance(y.grad_fn, C._NarrowLastConv._backward_cls)
    dx, dw, db = torch.autograd.grad(y, (xg, layer.conv.weight, layer.conv.bias), gy)
    assert sorted(calls) == ['narrow_forward', 'narrow_out_conv', 'narrow_out_weight_gradient']
    assert dw.shape == layer.conv.weight.shape and dw.stride() == layer.conv.weight.stride()
    errs = {k: R.rel(t.detach().cpu().numpy(), ref[k]) for k, t in (('y', y), ('dx', dx), ('dw', dw), ('db', db))}
    print("narrow last layer", name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs['y'] < R.BOUND and errs['dx'] < R.Y_BOUND and errs['dw'] < R.DW_BOUND and errs['db'] < R.DW_BOUND, errs
    # a forward under no_grad: the same launch, the same bits
    with torch.no_grad():
        assert same_bits(layer(x), y.detach())
    # an input that needs no gradient: no data-gradient launch, the same dW and db
    del calls[:]
    y2 = layer(x)
    dw2, db2 = torch.autograd.grad(y2, (layer.conv.weight, layer.conv.bias), gy)
    assert sorted(calls) == ['narrow_out_conv', 'narrow_out_weight_gradient']
    assert same_bits(dw2, dw) and same_bits(db2, db) and same_bits(y2.detach(), y.detach())


def test_an_unmarked_or_unsupported_layer_keeps_its_route():
    from wc_gan_amd.generator import Conv2D
    x = torch.randn(2, 5, 7, 32, device='cuda')
    assert not Conv2D(32, 3, (3, 3)).cuda()._narrow_last_route(x)
    marked = Conv2D(32, 3, (3, 3), narrow_last=True).cuda()
    assert marked._narrow_last_route(x)
    assert not marked._narrow_last_route(x.double()) and not marked._narrow_last_route(x.permute(0, 2, 1, 3))
    assert not Conv2D(48, 3, (3, 3), narrow_last=True).cuda()._narrow_last_route(torch.randn(2, 5, 7, 48, device='cuda'))
    assert not Conv2D(32, 3, (3, 3), spectral=True, narrow_last=True).cuda()._narrow_last_route(x)
    # a marked layer the node does not take computes what the unmarked layer computes, bit for bit
    a, b = Conv2D(48, 3, (3, 3), narrow_last=True).cuda(), Conv2D(48, 3, (3, 3)).cuda()
    b.load_state_dict(a.state_dict())
    x48 = torch.randn(2, 5, 7, 48, device='cuda')
    assert same_bits(a(x48), b(x48))


# ---- the network -----------------------------------------------------------------------------------------------------------------------
NET_KW = dict(block_sizes=(128, 64, 32), resamples=('UP', 'UP', 'UP'), first_block_shape=(4, 4, 128), number_of_classes=1000,
              block_norm='d', block_after_norm='ufconv', filters_emb=32, last_norm='d', last_after_norm='uconv', gan_type='PROJECTIVE')
NET_BATCH = 8


def _nets():
    """the cut-down generator marked and unmarked, the same parameters (tests/test_conv_slim_gpu.py's module)"""
    from wc_gan_amd.generator import make_generator
    nets = []
    for mark in (True, False):
        torch.manual_seed(7)
        G = make_generator(slim_conv=True, narrow_last=mark, **NET_KW)
        with torch.no_grad():
            for name, p in G.named_parameters():
                if name.endswith(('.bias', '.beta', '.gamma', '.kernel', '.class_matrix')):
                    p.add_(0.05 * torch.randn_like(p))
        nets.append(G.cuda().train())
    for (na, pa), (nb, pb) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert na == nb and torch.equal(pa, pb)
    return nets


def _net_inputs(seed=21):
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    z = torch.randn(NET_BATCH, 128, generator=g, dtype=torch.float64)
    cls = torch.randint(0, 1000, (NET_BATCH, 1), generator=g, dtype=torch.int32)
    w = torch.randn(NET_BATCH, 32, 32, 3, generator=g, dtype=torch.float64)
    return z.float().cuda(), cls.cuda(), w.cuda()


def _train_call(G, z, cls, w, record=None):
    import wc_gan_amd.functional as WF
    for p in G.parameters():
        p.grad = None
    if record is not None:
        WF.MASK_TAP = {'record': record}
    try:
        img = G(z, cls)
    finally:
        WF.MASK_TAP = None
    (img * w.float()).sum().backward()
    return img.detach(), {n: p.grad for n, p in G.named_parameters()}


def test_a_cut_down_generator_marked_against_unmarked():
    """identical ReLU masks on both routes (everything in front of Generator.Final is the same code on the same bits); the image and every
    parameter gradient within 2e-5 of the tensor's maximum -- a block convolution's bias gradient, zero in exact arithmetic, against the
    largest gradient of the model at 2e-6, as in tests/test_handoff_gpu.py; and the marked pass against the float64 reference"""
    import generator_reference as GR
    import test_generator_gpu as TG
    marked, plain = _nets()
    z, cls, w = _net_inputs()
    state = {k: v.detach().clone() for k, v in marked.state_dict().items()}
    rec_m, rec_p = [], []
    probe = TG._Probe(marked, signs=False)
    with probe:
        img_m, g_m = _train_call(marked, z, cls, w, rec_m)
    img_p, g_p = _train_call(plain, z, cls, w, rec_p)
    assert len(rec_m) == len(rec_p) == GR.relu_count(NET_KW['block_sizes'])
    for a, b in zip(rec_m, rec_p):
        assert same_bits(a, b), "the two routes applied different ReLU masks"
    assert set(g_m) == set(g_p) and all(v is not None for v in g_m.values())
    top = max(float(v.abs().max()) for v in g_p.values())
    bad = {}
    for n, a, b in [('image', img_m, img_p)] + [(n, g_m[n], g_p[n]) for n in g_p]:
        d = float((a - b).abs().max())
        own, of_top = d / max(float(b.abs().max()), 1e-30), d / top
        if own > TWO_ROUTES and not (GR.zero_in_exact_arithmetic(n) and of_top <= 2e-6):
            bad[n] = (own, of_top)
    final = {n: float((g_m[n] - g_p[n]).abs().max() / g_p[n].abs().max()) for n in g_p if n.startswith('final_conv.')}
    print("narrow last network, marked against unmarked: image", f"{float((img_m - img_p).abs().max() / img_p.abs().max()):.2e}", final)
    assert not bad, bad
    # the marked pass against the float64 reference on the masks it applied
    masks = [TG._unpack(m, s) for m, s in zip(rec_m, probe.shapes)]
    ref, ref_img, ref_grads = GR.run(state, dict(NET_KW, **TG._site_kw(marked)), z, cls, w, masks, training=True)
    TG._check_masks(masks, ref, 'narrow last network')
    errs = GR.errors(img_m, g_m, None, ref, ref_img, ref_grads)
    print("narrow last network against float64", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(errs[k] < TG.BOUNDS[k] for k in errs if k != 'moving'), errs


def _profile(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU], record_shapes=True) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    ops = [e for e in ev if e.device_type == torch.autograd.DeviceType.CPU]
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA]
    return ops, kernels


def _final_mm(ops):
    """aten::mm calls with an operand of 27 = 9 taps x 3 outputs columns: _NarrowConv3x3's x @ wall (no other matrix of the network has 27)"""
    return [e for e in ops if e.name in ('aten::mm', 'aten::matmul', 'aten::addmm') and any(27 in s for s in (e.input_shapes or []) if s)]


def test_a_marked_training_call_runs_the_three_narrow_kernels_and_none_of_torchs():
    marked, plain = _nets()
    z, cls, w = _net_inputs()
    _train_call(marked, z, cls, w)
    _train_call(plain, z, cls, w)
    ops, kernels = _profile(lambda: _train_call(marked, z, cls, w))
    names = {e.name for e in ops}
    assert names, "the profiler reported no operators"
    for op in ('aten::convolution_backward', 'aten::col2im', 'aten::im2col'):
        assert op not in names, op
    assert _final_mm(ops) == []
    if kernels:
        joined = ' '.join(kernels)
        for name in ('conv_narrow_out_kernel', 'conv_wrw_narrow32_kernel', 'conv_wrw_narrow32_reduce_kernel', 'conv_fwd_narrow32_kernel'):
            assert name in joined, name
    # the control: the unmarked call holds what the assertions above look for
    ops_p, kernels_p = _profile(lambda: _train_call(plain, z, cls, w))
    names_p = {e.name for e in ops_p}
    assert 'aten::convolution_backward' in names_p and 'aten::col2im' in names_p and len(_final_mm(ops_p)) >= 1
    if kernels_p:
        assert 'narrow32' not in ' '.join(kernels_p)


def test_a_captured_marked_call_replays_the_eager_bits():
    """forward and backward of the marked network captured in one graph: two replays give the bits of the eager call (the sites' split
    scales have settled on the repeated input: four eager calls in front)"""
    marked, _ = _nets()
    z, cls, w = _net_inputs()
    for _ in range(4):
        img, grads = _train_call(marked, z, cls, w)
    eager = [img.clone()] + [grads[n].clone() for n in sorted(grads)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for p in marked.parameters():
            p.grad = None
        with torch.cuda.graph(graph, stream=side):
            out = marked(z, cls)
            (out * w.float()).sum().backward()
        held = [out.detach()] + [dict(marked.named_parameters())[n].grad for n in sorted(grads)]
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(2):
        for t in held:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert same_bits(a, b), rep


if __name__ == '__main__':
    import os
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                              'narrow_last_parity.txt')
    keys = ('y0', 'y', 'dx', 'dw')
    lines = [f"{'row':<22}{'weight':<16}" + ''.join(f"{k:>12}" for k in keys)]
    worst = dict.fromkeys(keys, 0.0)
    for row in R.ROWS:
        for fmt in FORMATS:
            errs = _measure(row, fmt)
            lines.append(f"{row.name:<22}{fmt:<16}" + ''.join(f"{errs[k]:>12.2e}" for k in keys))
            worst = {k: max(worst[k], errs[k]) for k in keys}
    lines.append(f"{'maximum':<22}{'':<16}" + ''.join(f"{worst[k]:>12.2e}" for k in keys))
    lines.append(f"bounds (max |error| / max |reference|): y0, y {R.BOUND:.0e}; dx {R.Y_BOUND:.0e}; dw {R.DW_BOUND:.0e}   "
                 "(y0: the forward without its bias)")
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
