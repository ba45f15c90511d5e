"""GPU tests of the k-split whose shares are summed inside the workgroup (csrc/wc_conv.hip conv_local_kernel, wc_conv_local_f16x3; DESIGN.md
section 4.5) against the two launches it replaces, in one process: conv.LOCAL_KSPLIT on and off.  A wave of the new kernel accumulates the
products of one share in the order conv_f16x3_kernel<2,2,true> does, the shares are added ((p0 + p1) + p2) + p3 and finished by the
finish launches' own functions, so every comparison is of the BITS: y, and behind a SPLIT tail both planes, the scale word, the record's
tags and carried words and the FOLD of its maxima (workgroup b of the new route's 256 writes the pairs b and b + 256: single pairs differ).

The k-split-4 rule fixes N*H*W = 8192 at Cout = 128, so these 4 MiB tensors are the smallest shapes that reach the kernel:
  'same' (128, 8, 8), (256, 4, 8), (32, 16, 16): a 64-point tile holds one image, two images, a quarter image; H != W
  'same' with Cin = 192: 54 iterations, shares of 13, 14, 13, 14 (boundaries 0, 13, 27, 40, 54) that start in the middle of a tap
  'down3' (128, 16, 16): 16 taps, stride 2
The same rows are held against torch's float64 convolution (test_conv_dispatch_gpu._ref3) within test_conv_gpu.TOL."""
import contextlib

import pytest
import torch

from _poison import Poison, run_patterns
from test_conv_dispatch_gpu import _kernel_names, _ref3
from test_conv_gpu import TOL, _rel

# kind, x's shape (Cin last)
SHAPES = [('same', (128, 8, 8, 128)), ('same', (256, 4, 8, 128)), ('same', (32, 16, 16, 128)), ('same', (128, 8, 8, 192)),
          ('down3', (128, 16, 16, 128))]
_ID = lambda s: f"{s[0]}-{'x'.join(map(str, s[1]))}"
REFUSED = ('same', (2, 8, 8, 128))          # k-split 8: stays on the two launches
OLD_KERNELS = ('conv_f16x3_kernel', 'conv_finish_tail_kernel', 'conv_ksplit_reduce')


class _Site:
    training = True


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _route(local):
    from wc_gan_amd import conv as C
    old, C.LOCAL_KSPLIT = C.LOCAL_KSPLIT, local
    try:
        yield
    finally:
        C.LOCAL_KSPLIT = old


_layers = {}


def _layer(kind, shape):
    """a Cin -> 128 3x3 layer on x of `shape`: plan, weight, bias, both images, x, x's planes, a residual, and -- computed once, shared,
    never written -- the float64 convolution of x with bias"""
    from wc_gan_amd import conv as C
    key = (kind, shape)
    if key not in _layers:
        w = (_randn((128, shape[-1], 3, 3), 2) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
        b = (_randn((128,), 3) * 0.1).cuda()
        # (the layer entry keeps widths that are no multiple of 128 on its other path; the kernels take Cin = 192: the plan is built directly)
        plan = C._plan(kind, C._Shape(shape), C._Shape(tuple(w.shape))) or C._Plan(kind, *shape[:3], tuple(w.shape))
        assert plan and plan.ok
        img, bimg = C.weight_image_pair(w, plan.fwd, plan.bwd)
        x = (_randn(shape, 10) * 1.7 + 0.3).cuda()
        g = plan.fwd[0]
        res = _randn((g.N, g.Hout, g.Wout, g.Cout), 20).cuda()
        y64 = _ref3(x.double(), w.double(), b.double(), kind).contiguous()
        _layers[key] = (plan, w, b, img, bimg, x, C.split_planes(x), res, y64)
    return _layers[key]


def _record(site, role='x'):
    return site._wc_split_hist[role][0]


def _record_fold(rec):
    """what a reader takes from a record: per array the maximum of the pairs and every tag; the words behind the arrays (the count of
    second passes, the carried maxima) as they are"""
    r = rec.detach().cpu()
    out = []
    for arr in (r[:1024].view(512, 2), r[1024:2048].view(512, 2)):
        out += [arr[:, 0].max().view(1), arr[:, 1].contiguous()]
    return out + [r[2048:]]


def _same_record(a, b):
    return all(_same_bits(p, q) for p, q in zip(_record_fold(a), _record_fold(b)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the plain and the residual finish: y on both routes, and against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES, ids=_ID)
def test_plain_and_residual_finish_have_the_two_launch_bits_and_match_float64(case):
    from wc_gan_amd import conv as C
    kind, shape = case
    plan, w, b, img, _, x, x_pl, res, y64 = _layer(kind, shape)
    g = plan.fwd[0]
    assert plan.local and plan.res and plan.tail and plan.fwd_ws == 4 * res.numel() * 4
    for bias in (None, b):
        for relu, r in ((False, None), (True, None), (False, res)):
            with _route(True):
                got = C.run(x_pl, img, g, bias, relu=relu, nbytes=plan.fwd_ws, res=r)
            with _route(False):
                want = C.run(x_pl, img, g, bias, relu=relu, nbytes=plan.fwd_ws, res=r)
            assert _same_bits(got, want), (bias is not None, relu, r is not None)
            ref = y64 if bias is not None else y64 - b.double()
            ref = torch.relu(ref) if relu else ref
            ref = ref + res.double() if r is not None else ref
            err = _rel(got, ref)
            print("local k-split", _ID(case), "bias", bias is not None, "relu", relu, "res", r is not None, "error vs float64", err)
            assert err < TOL, (bias is not None, relu, r is not None, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# the SPLIT tail, with and without the residual, over three calls behind the seeding one: tags and parities turn over
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("case", SHAPES, ids=_ID)
def test_split_tail_over_three_calls_has_the_two_launch_bits(case, residual):
    from wc_gan_amd import _lib, conv as C
    kind, shape = case
    plan, w, b, img, _, x, _, _, y64 = _layer(kind, shape)
    g = plan.fwd[0]
    out = (g.N, g.Hout, g.Wout, g.Cout)
    mine, twin = _Site(), _Site()
    # call 0 seeds both records on the two-launch route; then: a history call, an all-zero y (the carried maximum), a normal call again
    scales = [1.0, 1.7, 0.0, 0.6]
    for k, sc in enumerate(scales):
        x_pl = C.split_planes(x * sc if k else x, relu=True)
        bias = None if sc == 0.0 else b
        res = (_randn(out, 20 + k) * sc).cuda() if residual else None
        if k == 0:
            with _route(False):
                y0 = C.run(x_pl, img, g, bias, nbytes=plan.fwd_ws, res=res)
            for site in (mine, twin):
                assert C._reader_record(site, 'x', w.device) is None
                C.split_planes(y0, relu=True, site=site, role='x')
            continue
        results = []
        for site, local in ((mine, True), (twin, False)):
            rec = C._reader_record(site, 'x', w.device)
            assert rec is not None
            tail = C._Tail(_lib.TAIL_SPLIT, out, w.device, record=rec, role='x', res=res)
            with _route(local):
                y = C.run_tail(x_pl, img, g, tail, bias=bias, nbytes=plan.fwd_ws)
            results.append((y,) + tuple(tail.planes))
        (got_y, *got_pl), (want_y, *want_pl) = results
        assert _same_bits(got_y, want_y), (k, 'y')
        if sc == 0.0:
            assert not bool(got_y.any())
        elif k == 1 and not residual:
            # (the same row against float64: relu(1.7 x) through the convolution)
            ref = _ref3(torch.relu(x.double() * sc), w.double(), b.double(), kind)
            assert _rel(got_y, ref) < TOL
        for a, e, name in zip(got_pl, want_pl, ('hi', 'lo', 'scale')):
            assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, name)
        assert C.HIST_FLOATS == _record(mine).numel() and _same_record(_record(mine), _record(twin)), (k, 'record')
    # the record the new route leaves serves the two-launch route's next call, and the other way round
    for site, local in ((mine, False), (twin, True)):
        tail = C._Tail(_lib.TAIL_SPLIT, out, w.device, record=C._reader_record(site, 'x', w.device), role='x')
        with _route(local):
            C.run_tail(C.split_planes(x, relu=True), img, g, tail, bias=b, nbytes=plan.fwd_ws)
        results.append(tail.planes)
    for a, e in zip(results[-2], results[-1]):
        assert _same_bits(a[:1] if a.numel() == 513 else a, e[:1] if e.numel() == 513 else e)
    assert _same_record(_record(mine), _record(twin))


# ---------------------------------------------------------------------------------------------------------------------------------
# the optional tails on the data gradient's geometry: MASKED without partial rows, DX
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_masked_and_dx_tails_have_the_two_launch_bits():
    from wc_gan_amd import _lib, conv as C
    kind, shape = SHAPES[0]
    plan, w, b, img, bimg, x, _, _, _ = _layer(kind, shape)
    gb = plan.bwd[0]
    assert plan.bwd_local and plan.bwd_tail
    h = _randn(shape, 6)
    h.view(-1)[::7] = 0.0
    h.view(-1)[3::11] = -0.0
    h[0, 0, 0, :4] = float('nan')
    h = h.cuda()
    other = _randn(shape, 8).cuda()
    mine, twin = _Site(), _Site()
    for k, sc in enumerate([1.0, 1.3, 0.8]):
        g_pl = C.split_planes((_randn(shape, 30 + k) * sc).cuda())[:3]
        if k == 0:
            with _route(False):
                dh = C.run(g_pl, bimg, gb, nbytes=plan.bwd_ws)
            for site in (mine, twin):
                C.split_planes_masked(dh, h, site=site, role='g')
            continue
        results = []
        for site, local in ((mine, True), (twin, False)):
            masked = C._Tail(_lib.TAIL_MASKED, shape, w.device, record=C._reader_record(site, 'g', w.device), role='g', mask=h)
            dx = C._Tail(_lib.TAIL_DX, shape, w.device, mask=h, other=other)
            with _route(local):
                dh = C.run_tail(g_pl, bimg, gb, masked, nbytes=plan.bwd_ws)
                assert C.run_tail(g_pl, bimg, gb, dx, nbytes=plan.bwd_ws) is None
            results.append((dh, dx.out) + tuple(masked.planes))
        for a, e, name in zip(results[0], results[1], ('dh', 'dx', 'hi', 'lo', 'scale')):
            assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, name)
        assert _same_record(_record(mine, 'g'), _record(twin, 'g')), k
    # with the bias gradient's partial rows the MASKED tail stays with the 512-workgroup finish, whatever the switch says
    tail = C._Tail(_lib.TAIL_MASKED, shape, w.device, record=C._reader_record(mine, 'g', w.device), role='g', mask=h, colsum=True)
    with _route(True):
        names = _kernel_names(lambda: C.run_tail(g_pl, bimg, gb, tail, nbytes=plan.bwd_ws))
    assert names and not [n for n in names if 'conv_local_kernel' in n] and [n for n in names if 'conv_finish_tail_kernel' in n], names


# ---------------------------------------------------------------------------------------------------------------------------------
# memory discipline: guard bands, no surviving fill, a captured graph replayed over re-poisoned outputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _seeded_site(kind, shape):
    from wc_gan_amd import conv as C
    plan, w, b, img, _, x, x_pl, res, _ = _layer(kind, shape)
    site = _Site()
    with _route(False):
        C.split_planes(C.run(x_pl, img, plan.fwd[0], b, nbytes=plan.fwd_ws, res=res), relu=True, site=site, role='x')
    return site


def _all_forms(kind, shape, site):
    """every required form of the entry on one input -> its outputs (the scale tensor's first word only: the rest is the split's scratch)"""
    from wc_gan_amd import _lib, conv as C
    plan, w, b, img, _, x, x_pl, res, _ = _layer(kind, shape)
    g = plan.fwd[0]
    out = (g.N, g.Hout, g.Wout, g.Cout)
    y_plain = C.run(x_pl, img, g, b, relu=True, nbytes=plan.fwd_ws)
    y_res = C.run(x_pl, img, g, b, nbytes=plan.fwd_ws, res=res)
    tail = C._Tail(_lib.TAIL_SPLIT, out, w.device, record=C._reader_record(site, 'x', w.device), role='x', res=res)
    y_tail = C.run_tail(x_pl, img, g, tail, bias=b, nbytes=plan.fwd_ws)
    return [y_plain, y_res, y_tail, tail.planes[0], tail.planes[1], tail.planes[2][:1]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[4]], ids=_ID)
def test_outputs_in_poisoned_guard_banded_buffers(case):
    kind, shape = case
    site = _seeded_site(kind, shape)
    with _route(True):
        # (the same input on every call: the record's maximum, and with it the planes' scale, stays where the seeding call left it)
        outs = run_patterns(lambda P: _all_forms(kind, shape, site))
    with _route(False):
        want = _all_forms(kind, shape, _seeded_site(kind, shape))
    for pattern, got in outs.items():
        for i, (a, e) in enumerate(zip(got, want)):
            assert _same_bits(a, e.cpu()), (hex(pattern), i)          # no fill survives: the bits are the two-launch route's
            assert not bool(torch.isnan(a.float()).any()), (hex(pattern), i)


@pytest.mark.gpu
def test_a_captured_graph_replayed_over_repoisoned_outputs_equals_the_eager_bits():
    kind, shape = SHAPES[0]
    site = _seeded_site(kind, shape)
    with _route(True):
        eager = [t.clone() for t in _all_forms(kind, shape, site)]
        with Poison(0xFF) as P:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                outs = _all_forms(kind, shape, site)
            for replay in range(2):
                for t in outs[:5]:
                    t.fill_(float('nan'))       # (on top of the captured fills: what the replay before left is gone)
                graph.replay()
                P.check_guards()
                for i, (a, e) in enumerate(zip(outs, eager)):
                    assert _same_bits(a, e), (replay, i)


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_eligible_forward_is_one_launch_of_the_new_kernel():
    from wc_gan_amd import _lib, conv as C
    kind, shape = SHAPES[0]
    plan, w, b, img, _, x, x_pl, res, _ = _layer(kind, shape)
    g = plan.fwd[0]
    out = (g.N, g.Hout, g.Wout, g.Cout)
    site = _seeded_site(kind, shape)
    tail = lambda: C._Tail(_lib.TAIL_SPLIT, out, w.device, record=C._reader_record(site, 'x', w.device), role='x', res=res)
    forms = {'plain': lambda: C.run(x_pl, img, g, b, nbytes=plan.fwd_ws),
             'res': lambda: C.run(x_pl, img, g, b, nbytes=plan.fwd_ws, res=res),
             'split': lambda: C.run_tail(x_pl, img, g, tail(), bias=b, nbytes=plan.fwd_ws)}
    for name, fn in forms.items():
        with _route(True):
            new = _kernel_names(fn)
        with _route(False):
            old = _kernel_names(fn)
        assert new and old, "this profiler build reports no device kernel names"
        assert len([n for n in new if 'conv_local_kernel' in n]) == 1, (name, new)
        assert not [n for n in new for k in OLD_KERNELS if k in n], (name, new)
        assert not [n for n in old if 'conv_local_kernel' in n] and len([n for n in old if 'conv_f16x3_kernel' in n]) == 1, (name, old)
        assert len(old) - len(new) == 1, (name, old, new)       # the finish launch is gone; the gated second pass stays behind the tail


@pytest.mark.gpu
def test_a_refused_geometry_launches_what_it_launched_before():
    from wc_gan_amd import conv as C
    kind, shape = REFUSED
    plan, w, b, img, _, x, x_pl, res, _ = _layer(kind, shape)
    assert not plan.local and plan.fwd_ws > 0
    fn = lambda: C.run(x_pl, img, plan.fwd[0], b, nbytes=plan.fwd_ws, res=res)
    with _route(True):
        new, y_new = _kernel_names(fn), fn()
    with _route(False):
        old, y_old = _kernel_names(fn), fn()
    assert new and new == old and not [n for n in new if 'conv_local_kernel' in n], (new, old)
    assert _same_bits(y_new, y_old)
