"""GPU tests of the critic's first block on the HIP route (csrc/wc_conv.hip conv_fwd_narrow_split_kernel and
conv_wrw_narrow_masked_kernel; conv._CriticFirstBlock): conv1's kernel writes conv2's planes, conv1's weight gradient applies the ReLU
mask, and the block's conv1 -> ReLU -> conv2 runs as one autograd node.  Every fused launch computes each element with the expressions of
the launches it replaces, so every comparison is of the BITS: the new entries against the two-launch route in one process.

The record of a site is compared by what its readers see -- the fold of the newer complete array, that array's tag, the two assumed words
and the redo counter: conv_split_hist_kernel's workgroup b leaves the maximum of ITS grid-stride elements in pair b, the narrow kernel's
workgroup b the maximum of its tiles in the pairs b, b + G, ..., so single pairs differ and only their fold is the tensor's maximum.

Shapes (M = N*H*W pixels in 32-pixel tiles, G = workgroups): 2x5x5 -> 64: a partial last tile, G = 1 owns all 512 pairs; 3x8x8 -> 128:
G = 4; 2x12x12 -> 128: G = 6, which does not divide 512; Cin = 1; k = 1 (the <2> instantiation); 9x64x64 -> 128: two tiles per wave."""
import contextlib
from functools import partial

import pytest
import torch

from _poison import run_patterns
from test_conv_dispatch_gpu import _kernel_names


class _Site:
    training = True


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _every_split_gated():
    """WC_SPLIT_HIST_REDO=2 for the duration: role 'x' takes the gated second pass too (the default gates the gradients' roles only)"""
    from wc_gan_amd import conv as C
    old, C._REDO_MODE = C._REDO_MODE, '2'
    try:
        yield
    finally:
        C._REDO_MODE = old


def _observable(rec):
    """what a reader of the record sees: (bits of the fold of the newer complete array, its tag, the two assumed words' bits, redo count)"""
    from wc_gan_amd import conv as C
    r = rec.detach().cpu()
    assert r.numel() == C.HIST_FLOATS
    arrays = r[:4 * 512].view(2, 512, 2)
    tags = arrays[:, :, 1].contiguous().view(torch.int32)
    complete = [int(tags[a].min()) == int(tags[a].max()) for a in (0, 1)]
    assert all(complete), "a record at rest has two complete arrays"
    newer = 1 if int(tags[1, 0]) > int(tags[0, 0]) else 0
    fold = arrays[newer, :, 0].max().view(1)
    words = r[C.HIST_REDO:C.HIST_REDO + 4].contiguous().view(torch.int32)
    return (int(fold.view(torch.int32)), int(tags[newer, 0]), int(words[2]), int(words[3]), int(words[0]))


def _layer(cin, cout, k, seed=0):
    w = (_randn((cout, cin, k, k), 2 + seed) * 0.3).cuda().contiguous(memory_format=torch.channels_last)
    b = (_randn((cout,), 3 + seed) * 0.1).cuda()
    return w, b


CASES = [((2, 5, 5, 3), 64, 3), ((3, 8, 8, 3), 128, 3), ((2, 12, 12, 3), 128, 3), ((2, 5, 5, 1), 64, 3), ((3, 8, 8, 3), 64, 1),
         ((9, 64, 64, 3), 128, 3)]


def _sequence(shape):
    """(input, with bias?) of the calls behind the seeding one: inside the window; grown 1000-fold (the gate fires); all zero with zero
    bias (the carried maximum); a normal call again"""
    x = _randn(shape, 11)
    # (the last call shrinks about 500-fold from the maximum the record carries past the zero tensor: inside the window's 4096)
    return [(x * 1.3, True), (x * 1000.0, True), (torch.zeros(shape), False), (_randn(shape, 12) * 2.0, True)]


def _two_launches(C, x, w, b, site):
    y = C.narrow_forward(x, w, b)
    return y, C.split_planes(y, relu=True, site=site, role='x')


def _check_call(C, k, got, want, mine, twin):
    (gy, gpl), (wy, wpl) = got, want
    assert _same_bits(gy, wy), (k, 'y')
    for a, e, name in zip(gpl, wpl, ('hi', 'lo', 'scale')):
        assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, name)
    om, ot = _observable(mine._wc_split_hist['x'][0]), _observable(twin._wc_split_hist['x'][0])
    print(f"call {k}: record (fold, tag, assumed, assumed, redo) mine {om} twin {ot}")
    assert om == ot, (k, 'record')
    return om


# ---------------------------------------------------------------------------------------------------------------------------------
# entry 1: the narrow forward that writes the reader's planes
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_split_forward(shape, cout, ks):
    """y, the reader's planes, the scale and the record of wc_conv_fwd_narrow_split_f32 against the two launches over a sequence of calls
    (tests/test_narrow_edges_gpu.py runs it at its rows too)"""
    from wc_gan_amd import conv as C
    w, b = _layer(shape[-1], cout, ks)
    assert C.narrow_split_supported(shape, tuple(w.shape))
    mine, twin = _Site(), _Site()
    with _every_split_gated():
        x0 = _randn(shape, 10).cuda()
        assert C._reader_record(mine, 'x', w.device) is None and C.first_block_route(shape, tuple(w.shape), None) == 'two'
        _two_launches(C, x0, w, b, mine)            # the seeding call: two launches on both sites
        _two_launches(C, x0, w, b, twin)
        for k, (x, with_bias) in enumerate(_sequence(shape), 1):
            x = x.cuda()
            bias = b if with_bias else None
            rec = C._reader_record(mine, 'x', w.device)
            assert rec is not None and C.first_block_route(shape, tuple(w.shape), rec) == 'planes'
            got = C.narrow_forward_split(x, w, bias, rec, relu=True, role='x')
            want = _two_launches(C, x, w, bias, twin)
            obs = _check_call(C, k, got, want, mine, twin)
            assert obs[4] == (0 if k == 1 else 1), (k, 'redo')          # the gate fires once: at the 1000-fold call
            if k == 2:      # ... and its result has the bits of the measured form -- of the ACTIVATED tensor: the record holds max relu(y),
                # conv_absmax_kernel measures max |y|, and where the largest |y| is a negative one a binade above (2x5x7, 2 -> 64, k = 1)
                # the measured form of y itself takes half the scale
                meas = C.split_planes(torch.relu(want[0]), relu=True)
                for a, e, name in zip(got[1], meas, ('hi', 'lo', 'scale')):
                    assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, 'measured', name)
            if k == 3:
                assert not bool(got[0].any()) and not bool(got[1][0].any()) and obs[0] == 0        # an all-zero tensor, maximum +0
        # non-temporal y stores: the same bits
        old, C.FIRST_BLOCK_NT = C.FIRST_BLOCK_NT, not C.FIRST_BLOCK_NT
        try:
            x = _randn(shape, 13).cuda()
            got = C.narrow_forward_split(x, w, b, C._reader_record(mine, 'x', w.device), relu=True, role='x')
            _check_call(C, 5, got, _two_launches(C, x, w, b, twin), mine, twin)
        finally:
            C.FIRST_BLOCK_NT = old


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cout,ks", CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_narrow_forward_leaves_y_and_the_readers_planes_scale_and_record(shape, cout, ks):
    _check_split_forward(shape, cout, ks)


@pytest.mark.gpu
def test_narrow_forward_with_planes_captured_and_replayed():
    from wc_gan_amd import conv as C
    shape, cout, ks = (2, 12, 12, 3), 128, 3
    w, b = _layer(3, cout, ks)
    mine, twin = _Site(), _Site()
    with _every_split_gated():
        x0 = _randn(shape, 10).cuda()
        _two_launches(C, x0, w, b, mine)
        _two_launches(C, x0, w, b, twin)
        static_x, static_b = x0.clone(), b.clone()
        rec = C._reader_record(mine, 'x', w.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = C.narrow_forward_split(static_x, w, static_b, rec, relu=True, role='x')
        # (the capture launched nothing: the record is as the seeding call left it)
        for k, (x, with_bias) in enumerate(_sequence(shape), 1):
            static_x.copy_(x.cuda())
            static_b.copy_(b if with_bias else torch.zeros_like(b))
            graph.replay()
            torch.cuda.synchronize()
            want = _two_launches(C, static_x, w, static_b, twin)
            obs = _check_call(C, k, got, want, mine, twin)
            assert obs[4] == (0 if k == 1 else 1), (k, 'redo')


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cout,ks", [((2, 5, 5, 3), 64, 3), ((2, 12, 12, 3), 128, 3)], ids=['2x5x5', '2x12x12'])
def test_narrow_forward_with_planes_on_poisoned_guarded_buffers(shape, cout, ks):
    from wc_gan_amd import conv as C
    w, b = _layer(3, cout, ks)
    x = _randn(shape, 21)
    seeded = _Site()
    _two_launches(C, _randn(shape, 20).cuda(), w, b, seeded)
    rec0 = seeded._wc_split_hist['x'][0].detach().cpu().clone()
    ref_site = _Site()
    ref_site._wc_split_hist = {'x': [rec0.cuda(), True]}
    ref_y, ref_pl = _two_launches(C, x.cuda(), w, b, ref_site)

    def call(P):
        rec = [P.guarded(rec0), True]
        y, (hi, lo, scale) = C.narrow_forward_split(P.guarded(x), P.guarded(w.cpu().contiguous()), P.guarded(b.cpu()), rec, relu=True, role='x')
        # (the scale tensor's other 512 floats are scratch of the measuring form: nobody writes them here)
        return dict(y=y, hi=hi, lo=lo, scale=scale[:1].clone())
    outs = run_patterns(call)       # nothing outside the tensors is written; the same bits whatever the buffers held: no poison left inside
    for o in outs.values():
        assert _same_bits(o['y'], ref_y.cpu()) and _same_bits(o['hi'], ref_pl[0].cpu()) and _same_bits(o['lo'], ref_pl[1].cpu())
        assert _same_bits(o['scale'], ref_pl[2][:1].cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# entry 2: the narrow weight gradient that applies the ReLU mask
# ---------------------------------------------------------------------------------------------------------------------------------
def _mask_tensor(shape, seed):
    """+0, -0, NaN and (from the normal draw) negative values among the pre-activations"""
    h = _randn(shape, seed)
    flat = h.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = float('nan')
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cout,ks", [((2, 5, 5, 3), 64, 3), ((2, 5, 5, 1), 64, 3), ((2, 5, 5, 3), 64, 1), ((3, 8, 8, 3), 128, 3),
                                           ((3, 8, 8, 1), 128, 1)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_masked_narrow_weight_gradient_has_the_bits_of_the_masked_copy(shape, cout, ks):
    """M = 50 with Cout = 64: clamped loads and the idle upper half of the 128-channel group.  The comparison is of the results' bits, not
    of the intermediate zeros: a masked-out element is g * 0 = (+-0) here and +0 in threshold_backward's copy (tests/test_critic_glue_gpu.py
    explains), which no sum that started as +0 can tell apart.  A NaN pre-activation lets the gradient through, as threshold_backward does."""
    w, _ = _layer(shape[-1], cout, ks)
    x = _randn(shape, 31).cuda()
    gshape = shape[:3] + (cout,)
    g = (_randn(gshape, 32) * 0.8).cuda()
    h = _mask_tensor(gshape, 33).cuda()
    _check_masked_gradient(x, g, h, w)


def _check_masked_gradient(x, g, h, w):
    """the masked weight gradient has the bits of narrow_gradients on threshold_backward's output (tests/test_narrow_edges_gpu.py runs it
    at its rows too)"""
    from wc_gan_amd import conv as C
    assert bool(torch.isnan(h).any()) and bool((h < 0).any()) and bool(torch.isfinite(g).all())
    want_dw, want_db = C.narrow_gradients(x, torch.ops.aten.threshold_backward(g, h, 0), w, True)
    got_dw, got_db = C.narrow_gradients(x, g, w, True, mask=h)
    assert got_dw.stride() == w.stride() and _same_bits(got_dw, want_dw) and _same_bits(got_db, want_db)
    assert bool(torch.isfinite(got_dw).all()) and bool(got_dw.any())
    # without the bias gradient, and against the entry the separate node calls
    got_dw2, none = C.narrow_gradients(x, g, w, False, mask=h)
    assert none is None and _same_bits(got_dw2, C.narrow_weight_gradient(x, torch.ops.aten.threshold_backward(g, h, 0), w))


# ---------------------------------------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(ragged):
    from wc_gan_amd.discriminator import ResBlockDown
    from wc_gan_amd.generator import Conv2D, create_norm
    torch.manual_seed(3)
    blk = ResBlockDown(3, 128, 'DOWN', 'D.0', create_norm('n', 'n'), partial(Conv2D, ragged_conv=ragged), is_first=True)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name.endswith('.bias'):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(7)) * 0.1)
    return blk.cuda()


def _block_call(blk, x, need_x, route):
    from wc_gan_amd import conv as C
    old, C.FIRST_BLOCK = C.FIRST_BLOCK, route
    try:
        blk.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(need_x)
        y = blk(xx, None)
        gy = _randn(tuple(y.shape), 41).cuda()
        y.backward(gy)
    finally:
        C.FIRST_BLOCK = old
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters()}
    if need_x:
        grads['x'] = xx.grad.detach().clone()
    return y.detach().clone(), grads


# 2x8x8x3: the block convolutions take conv2 there on a partial last tile only (layers marked ragged_conv); 2x16x16x3: the plain layers
@pytest.mark.gpu
@pytest.mark.parametrize("shape,ragged", [((2, 8, 8, 3), True), ((2, 16, 16, 3), False)], ids=['2x8x8', '2x16x16'])
@pytest.mark.parametrize("need_x", [False, True], ids=['critic-update', 'generator-update'])
def test_first_block_as_one_node_has_the_bits_of_the_separate_nodes(shape, ragged, need_x):
    """The image's gradient is MIOpen's data gradient on both routes (the same call on the same operands); at these shapes its default
    solver is not reproducible from one call to the next (four calls on one set of operands differ in their last bit), so both routes run
    with torch.backends.cudnn.deterministic, under which it is."""
    import copy
    a = _block(ragged)
    b = copy.deepcopy(a)
    assert a._first_plan_of(shape) is not None
    for k in range(3):              # the first call unseeded
        x = (_randn(shape, 50 + k) * (1.0 + k)).cuda()
        if need_x:                  # as the generator hands its images over: an NHWC view of an NCHW tensor
            x = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
            assert not x.is_contiguous() and a._first_plan(x) is not None
        old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
        try:
            ya, ga = _block_call(a, x, need_x, True)
            yb, gb = _block_call(b, x, need_x, False)
        finally:
            torch.backends.cudnn.deterministic = old
        assert _same_bits(ya, yb), (k, 'y')
        assert sorted(ga) == sorted(gb) and len(ga) == 6 + (1 if need_x else 0)
        for n in ga:
            assert _same_bits(ga[n], gb[n]), (k, n)


@pytest.mark.gpu
def test_first_block_launches_by_kernel_names():
    from wc_gan_amd import conv as C
    shape = (2, 8, 8, 3)
    blk = _block(True)
    x = _randn(shape, 60).cuda()
    _block_call(blk, x, False, True)                # seeds the sites' records

    def passes(need_x, train=True):
        out = {}
        blk.train(train)
        blk.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(need_x)

        def fwd():
            out['y'] = blk(xx, None)
        f = _kernel_names(fwd)
        g = _randn(tuple(out['y'].shape), 61).cuda()
        b = _kernel_names(lambda: out['y'].backward(g)) if train else []
        blk.train(True)
        return f, b
    # the elementwise kernel of torch's threshold_backward at h's shape, by the name a call of its own shows
    h0 = _randn((2, 8, 8, 128), 62).cuda()
    thr = set(_kernel_names(lambda: torch.ops.aten.threshold_backward(h0, h0, 0)))
    assert len(thr) == 1, thr

    def masks(names):
        return [n for n in names if n in thr]
    assert C.FIRST_BLOCK and C.FIRST_BLOCK_PLANES and C.FIRST_BLOCK_MASK
    fwd, bwd = passes(False)
    # conv2's input planes come out of conv1's kernel: no pass over h in the forward
    assert [n for n in fwd if 'conv_fwd_narrow_split_kernel' in n] and not [n for n in fwd if 'conv_split_hist_kernel' in n], fwd
    assert not [n for n in fwd if 'conv_fwd_narrow_kernel<14' in n], fwd
    # the critic's own update: the mask rides in conv1's weight gradient
    assert [n for n in bwd if 'conv_wrw_narrow_masked_kernel' in n], bwd
    assert not masks(bwd), bwd
    # the generator's update: the data gradient reads the masked copy, so threshold_backward writes it
    fwd, bwd = passes(True)
    assert [n for n in fwd if 'conv_fwd_narrow_split_kernel' in n]
    assert masks(bwd), bwd
    assert not [n for n in bwd if 'conv_wrw_narrow_masked_kernel' in n] and [n for n in bwd if 'conv_wrw_narrow_kernel' in n], bwd
    # eval mode measures every tensor: the two launches (the narrow forward, then absmax + split)
    with torch.no_grad():
        fwd, _ = passes(False, train=False)
    assert [n for n in fwd if 'conv_fwd_narrow_kernel' in n] and [n for n in fwd if 'conv_absmax_kernel' in n], fwd
    assert not [n for n in fwd if 'conv_fwd_narrow_split_kernel' in n], fwd
    # each part has its own switch
    for flag, gone in (('FIRST_BLOCK_PLANES', 'conv_fwd_narrow_split_kernel'), ('FIRST_BLOCK_MASK', 'conv_wrw_narrow_masked_kernel')):
        old = getattr(C, flag)
        setattr(C, flag, False)
        try:
            fwd, bwd = passes(False)
        finally:
            setattr(C, flag, old)
        assert not [n for n in fwd + bwd if gone in n], (flag, fwd, bwd)
        if flag == 'FIRST_BLOCK_PLANES':
            assert [n for n in fwd if 'conv_split_hist_kernel' in n] and [n for n in bwd if 'conv_wrw_narrow_masked_kernel' in n], (fwd, bwd)
        else:
            assert masks(bwd) and [n for n in fwd if 'conv_fwd_narrow_split_kernel' in n], (fwd, bwd)
