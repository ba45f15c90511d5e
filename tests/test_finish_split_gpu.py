"""GPU tests of the k-split finishes that write what their next launch read back (csrc/wc_conv.hip conv_finish_tail_kernel and
conv_pair_reduce_tail_kernel): F1 / F2 the reader's planes of relu(y), B1 conv1's masked output-gradient planes with
the bias gradient's partial rows, B2 the SAME block's input gradient.  Every fused launch computes each element with the expressions of the
two launches it replaces, on the split's own 512 x 256 grid, so every comparison is torch.equal -- and, for what leaves as planes, scale
words, records and partial rows, of the BITS (zeros' signs included): the fused route against the two-launch route in one process.

Shapes: SAME (2, 8, 8, 128): one tile, ksplit 8, most of the 512 workgroups idle.  DOWN (2, 16, 16, 128): down3's finish with the
residual.  SAME (72, 8, 8, 128): n / 4 = 147 456 > 512 * 256, so some threads take a second grid-stride element -- the column sums' order."""
import contextlib
import copy
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from test_conv_dispatch_gpu import _kernel_names

SAME_SMALL, DOWN_SMALL, SAME_STRIDE2 = (2, 8, 8, 128), (2, 16, 16, 128), (72, 8, 8, 128)
FLAGS = ('FUSED_FINISH', 'FUSED_FINISH_F1', 'FUSED_FINISH_F2', 'FUSED_FINISH_B1', 'FUSED_FINISH_B2')


class _Site:
    training = True


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def _route(**flags):
    """the module flags of wc_gan_amd.conv for the duration of a call"""
    from wc_gan_amd import conv as C
    old = {k: getattr(C, k) for k in flags}
    for k, v in flags.items():
        assert k in FLAGS
        setattr(C, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(C, k, v)


def _layer(kind, shape, seed=0):
    """a 128 -> 128 3x3 layer on x of `shape`: plan, weight, bias, both images"""
    from wc_gan_amd import conv as C
    w = (_randn((128, shape[-1], 3, 3), 2 + seed) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
    b = (_randn((128,), 3 + seed) * 0.1).cuda()
    plan = C._plan(kind, C._Shape(shape), C._Shape(tuple(w.shape)))
    assert plan and plan.ok
    img, bimg = C.weight_image_pair(w, plan.fwd, plan.bwd)
    return plan, w, b, img, bimg


def _record(site, role):
    return site._wc_split_hist[role][0]


def _redo(site, role):
    from wc_gan_amd import conv as C
    return int(_record(site, role)[C.HIST_REDO:C.HIST_REDO + 1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# F1 / F2: the forward finish (with and without the residual) writes the reader's planes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,residual", [('same', SAME_SMALL, False), ('same', SAME_SMALL, True), ('down3', DOWN_SMALL, True),
                                                 ('same', SAME_STRIDE2, False), ('same', SAME_STRIDE2, True)])
def test_forward_finish_leaves_y_and_the_readers_planes_scale_and_record(kind, shape, residual):
    from wc_gan_amd import _lib, conv as C
    plan, w, b, img, _ = _layer(kind, shape)
    g = plan.fwd[0]
    out = (g.N, g.Hout, g.Wout, g.Cout)
    assert plan.tail and plan.fwd_ws > 0
    mine, twin = _Site(), _Site()
    # call 0 seeds both records on the two-launch route; then: a history call, an all-zero y (the carried maximum), a normal call again
    scales = [1.0, 1.7, 0.0, 0.6]
    for k, sc in enumerate(scales):
        x_pl = C.split_planes((_randn(shape, 10 + k) * sc).cuda(), relu=True)
        bias = None if sc == 0.0 else b
        res = (_randn(out, 20 + k) * sc).cuda() if residual else None
        want_y = C.run(x_pl, img, g, bias, nbytes=plan.fwd_ws, res=res) if residual else C.run(x_pl, img, g, bias, nbytes=plan.fwd_ws)
        want_pl = C.split_planes(want_y, relu=True, site=twin, role='x')
        rec = C._reader_record(mine, 'x', w.device)
        if k == 0:
            assert rec is None          # no record yet: the caller keeps the two launches
            C.split_planes(want_y, relu=True, site=mine, role='x')
            continue
        assert rec is not None
        tail = C._Tail(_lib.TAIL_SPLIT, out, w.device, record=rec, role='x', res=res)
        got_y = C.run_tail(x_pl, img, g, tail, bias=bias, nbytes=plan.fwd_ws)
        assert _same_bits(got_y, want_y), (k, 'y')
        if sc == 0.0:
            assert not bool(got_y.any())
        for a, e, name in zip(tail.planes, want_pl, ('hi', 'lo', 'scale')):
            assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, name)
        assert C.HIST_FLOATS == _record(mine, 'x').numel() and _same_bits(_record(mine, 'x'), _record(twin, 'x')), (k, 'record')


# ---------------------------------------------------------------------------------------------------------------------------------
# B1: the data gradient's finish writes dh, conv1's masked planes, the record and the partial rows -- both launch forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [('same', SAME_SMALL), ('down3', DOWN_SMALL), ('same', SAME_STRIDE2)])
@pytest.mark.parametrize("paired", [True, False])
def test_data_gradient_finish_leaves_dh_masked_planes_record_and_rows(kind, shape, paired):
    from wc_gan_amd import _lib, conv as C
    plan, w, b, img, bimg = _layer(kind, shape)
    gf, gb = plan.fwd[0], plan.bwd[0]
    assert plan.bwd_tail and plan.pair and plan.bwd_ws > 0
    gshape = (gf.N, gf.Hout, gf.Wout, gf.Cout)
    h = _randn(shape, 6)
    h.view(-1)[::7] = 0.0
    h.view(-1)[3::11] = -0.0
    h = h.cuda()
    x_pl = C.split_planes(_randn(shape, 5).cuda(), relu=True)
    mine, twin = _Site(), _Site()
    # seed; history; an all-zero gradient; a normal one; one grown 1000-fold: the gated second pass is taken, on both routes alike
    scales = [1.0, 1.3, 0.0, 0.8, 800.0]
    for k, sc in enumerate(scales):
        g_pl = C.split_planes((_randn(gshape, 30 + k) * sc).cuda(), colsum=True)
        if paired:
            want_dh, want_dw, want_db = C.backward_pair(g_pl, bimg, x_pl, plan, w, colsum=g_pl[3])
        else:
            want_dh = C.run(g_pl[:3], bimg, gb, nbytes=plan.bwd_ws)
        want_pl = C.split_planes_masked(want_dh, h, site=twin, role='g', colsum=True)
        rec = C._reader_record(mine, 'g', w.device)
        if k == 0:
            assert rec is None
            C.split_planes_masked(want_dh, h, site=mine, role='g', colsum=True)
            continue
        tail = C._Tail(_lib.TAIL_MASKED, shape, w.device, record=rec, role='g', mask=h, colsum=True)
        assert tail.c.redo == 1         # role 'g' is guarded: the gated launch follows the fused one
        if paired:
            got_dh, got_dw, got_db = C.backward_pair(g_pl, bimg, x_pl, plan, w, colsum=g_pl[3], tail=tail)
            assert _same_bits(got_dw, want_dw) and _same_bits(got_db, want_db), k
        else:
            got_dh = C.run_tail(g_pl[:3], bimg, gb, tail, nbytes=plan.bwd_ws)
        assert _same_bits(got_dh, want_dh), (k, 'dh')
        for a, e, name in zip(tail.planes, want_pl, ('hi', 'lo', 'scale', 'rows')):
            assert _same_bits(a[:1] if name == 'scale' else a, e[:1] if name == 'scale' else e), (k, name)
        assert tail.planes[3].shape == (512, 128)
        assert _same_bits(_record(mine, 'g'), _record(twin, 'g')), (k, 'record')
        assert _redo(mine, 'g') == _redo(twin, 'g') == (1 if k == 4 else 0), k


# ---------------------------------------------------------------------------------------------------------------------------------
# B2: the data gradient's finish writes the block's input gradient -- both launch forms
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SAME_SMALL, SAME_STRIDE2])
@pytest.mark.parametrize("paired", [True, False])
def test_data_gradient_finish_writes_the_block_input_gradient(shape, paired):
    from wc_gan_amd import _lib, conv as C
    plan, w, b, img, bimg = _layer('same', shape)
    assert plan.bwd_tail and plan.pair
    x = _randn(shape, 6)
    x.view(-1)[::7] = 0.0
    x.view(-1)[3::11] = -0.0
    x[0, 0, 0, :4] = float('nan')       # (a NaN lets the gradient through, as aten::threshold_backward)
    x = x.cuda()
    x_pl = C.split_planes(_randn(shape, 5).cuda(), relu=True)
    other = _randn(shape, 8).cuda()
    g_pl = C.split_planes(_randn(shape, 9).cuda(), colsum=True)
    tail = C._Tail(_lib.TAIL_DX, shape, w.device, mask=x, other=other)
    if paired:
        dx1, want_dw, want_db = C.backward_pair(g_pl, bimg, x_pl, plan, w, colsum=g_pl[3])
        none, got_dw, got_db = C.backward_pair(g_pl, bimg, x_pl, plan, w, colsum=g_pl[3], tail=tail)
        assert _same_bits(got_dw, want_dw) and _same_bits(got_db, want_db)
    else:
        dx1 = C.run(g_pl[:3], bimg, plan.bwd[0], nbytes=plan.bwd_ws)
        none = C.run_tail(g_pl[:3], bimg, plan.bwd[0], tail, nbytes=plan.bwd_ws)
    assert none is None                 # dx1 is never materialised
    assert _same_bits(tail.out, C.block_input_gradient(dx1, x, other, False))


# ---------------------------------------------------------------------------------------------------------------------------------
# the block and the critic: three consecutive training calls (call 1 unseeded, so unfused; calls 2 and 3 fused)
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(resample, spectral):
    from wc_gan_amd.discriminator import ResBlockDown
    from wc_gan_amd.generator import Conv2D, create_norm
    torch.manual_seed(3)
    conv_layer = partial(Conv2D, spectral=spectral, conv_singular=False, spectral_iterations=1, fully_diff_spectral=False)
    blk = ResBlockDown(128, 128, resample, 'D.1', create_norm('n', 'n'), conv_layer, is_first=False)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return blk.cuda().train()


def _in_critic(blk, x):
    """the block called as Discriminator.forward calls it (here: the last block, nobody behind it to hand planes to)"""
    return blk(x, None, handover={'next': None})


def _run_block(blk, x0, gy, fused):
    x = x0.clone().requires_grad_(True)
    params = list(blk.parameters())
    with _route(FUSED_FINISH=fused):
        y = _in_critic(blk, x)
        grads = torch.autograd.grad(y, [x] + params, gy)
    return (y.detach(),) + grads


def _records(blk):
    return {(s, r): rec[0] for s in ('conv1', 'conv2', 'shortcut') for r, rec in getattr(getattr(blk, s, None), '_wc_split_hist', {}).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("resample,shape", [('DOWN', DOWN_SMALL), ('SAME', SAME_SMALL)])
def test_block_over_three_calls_has_the_bits_of_the_two_launch_route(resample, shape, spectral):
    a = _block(resample, spectral)
    b = copy.deepcopy(a)
    out = (shape[0], shape[1] // 2, shape[2] // 2, 128) if resample == 'DOWN' else shape
    names = ['y', 'dx'] + [n for n, _ in a.named_parameters()]     # dW1, db1, dW2, db2 (and the shortcut's) among them
    for call in range(3):
        x = (_randn(shape, 10 + call) * (1.0 + 0.5 * call)).cuda()
        gy = (_randn(out, 20 + call) * (1.0 + call)).cuda()
        for got, want, name in zip(_run_block(a, x, gy, True), _run_block(b, x, gy, False), names):
            assert _same_bits(got, want), (call, name)
    ra, rb = _records(a), _records(b)
    assert ra.keys() == rb.keys() and all(_same_bits(ra[k], rb[k]) for k in ra)


def _critic(seed=5):
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.train import CONFIGS
    torch.manual_seed(seed)
    D = make_discriminator(**CONFIGS['cifar10_uncond']['discriminator'])
    with torch.no_grad():
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.cuda().train()


def _hinge(D, x):
    out = D(x, None)
    n = x.shape[0] // 2
    return F.relu(1.0 - out[:n]).mean() + F.relu(1.0 + out[n:]).mean()


def _critic_call(D, x, fused):
    with _route(FUSED_FINISH=fused):
        D.zero_grad(set_to_none=True)
        loss = _hinge(D, x)
        loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in D.named_parameters()}


@pytest.fixture(scope="module")
def critic_runs():
    """the four-block CIFAR-10 critic at batch 4, three calls on each route -> (the untouched start, inputs, fused results, two-launch
    results, the two critics)"""
    start = _critic()
    a, b = copy.deepcopy(start), copy.deepcopy(start)
    xs = [(torch.rand((4, 32, 32, 3), generator=torch.Generator().manual_seed(s)) * 2 - 1).cuda() for s in (1, 2, 3)]
    fused = [_critic_call(a, x, True) for x in xs]
    plain = [_critic_call(b, x, False) for x in xs]
    return start, xs, fused, plain, a, b


@pytest.mark.gpu
def test_critic_over_three_calls_has_the_bits_of_the_two_launch_route(critic_runs):
    _, xs, fused, plain, a, b = critic_runs
    for k in range(3):
        assert _same_bits(fused[k][0], plain[k][0]), k
        for n in fused[k][1]:
            assert _same_bits(fused[k][1][n], plain[k][1][n]), (k, n)
    for i, (ba, bb) in enumerate(zip(a.blocks, b.blocks)):
        ra, rb = _records(ba), _records(bb)
        assert ra.keys() == rb.keys() and all(_same_bits(ra[k], rb[k]) for k in ra), i


@pytest.mark.gpu
def test_critic_captured_after_an_eager_warm_up_equals_three_eager_calls(critic_runs):
    from wc_gan_amd import conv as C
    start, xs, fused, _, _, _ = critic_runs
    assert C.FUSED_FINISH
    c = copy.deepcopy(start)
    _critic_call(c, xs[0], True)        # (allocates and seeds the sites' records)
    static_x = xs[0].clone()
    c.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = _hinge(c, static_x)
        loss.backward()
    for k in (1, 2):
        static_x.copy_(xs[k])
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(loss.detach(), fused[k][0]), k
        for n, p in c.named_parameters():
            assert _same_bits(p.grad, fused[k][1][n]), (k, n)


@pytest.mark.gpu
def test_critic_hands_planes_between_consecutive_fused_blocks_only(critic_runs):
    """a seeded training pass: blocks 1 and 2 finish with the next block's planes (F2), block 3 -- whose output goes to the tail -- and
    the image block 0 do not; blocks 2 and 3 take the planes and skip their first split"""
    _, xs, _, _, a, b = critic_runs
    names = _kernel_names(lambda: a(xs[0], None))
    with _route(FUSED_FINISH=False):
        plain = _kernel_names(lambda: b(xs[0], None))
    count = lambda ns, k: len([n for n in ns if k in n])
    # F1 in blocks 1-3 and F2 behind blocks 1 and 2: five finishes with a tail, five splits and five plain finishes fewer
    assert count(names, 'conv_finish_tail_kernel') == 5 and count(plain, 'conv_finish_tail_kernel') == 0, names
    assert count(plain, 'conv_split_hist_kernel') - count(names, 'conv_split_hist_kernel') == 5, (names, plain)
    assert count(plain, 'conv_ksplit_reduce_kernel') - count(names, 'conv_ksplit_reduce_kernel') == 3, (names, plain)
    # block 3's conv2 keeps the finish with the residual: its output goes to the tail
    assert count(plain, 'conv_ksplit_reduce_res_kernel') == 3 and count(names, 'conv_ksplit_reduce_res_kernel') == 1, (names, plain)
    assert len(plain) - len(names) == 5


# ---------------------------------------------------------------------------------------------------------------------------------
# launches: a seeded SAME block in training mode; a reader in eval mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_seeded_same_block_launches_none_of_the_passes_the_finishes_took_over():
    blk = _block('SAME', False)
    x = _randn(SAME_SMALL, 1).cuda().requires_grad_(True)
    gy = _randn(SAME_SMALL, 2).cuda()
    params = list(blk.parameters())
    torch.autograd.grad(_in_critic(blk, x), [x] + params, gy)   # (the sites' first call: unseeded, two launches everywhere)
    box = {}
    fwd = _kernel_names(lambda: box.__setitem__('y', _in_critic(blk, x)))
    bwd = _kernel_names(lambda: torch.autograd.grad(box['y'], [x] + params, gy))
    assert fwd and bwd
    # forward: conv1's input is split (nobody in front), conv2's input is not: conv1's finish wrote its planes
    assert len([n for n in fwd if 'conv_split_hist_kernel' in n]) == 1, fwd
    assert len([n for n in fwd if 'conv_finish_tail_kernel' in n]) == 1, fwd
    assert not [n for n in fwd if 'conv_ksplit_reduce_kernel' in n], fwd
    # backward: no masked split, no block-dx launch; the pair's second launch carries both; the gated second pass stays
    assert not [n for n in bwd if 'gp_split_hist_kernel' in n], bwd
    assert not [n for n in bwd if 'conv_block_dx_kernel' in n], bwd
    assert not [n for n in bwd if 'conv_pair_reduce_kernel' in n], bwd
    assert len([n for n in bwd if 'conv_pair_reduce_tail_kernel' in n]) == 2, bwd
    assert len([n for n in bwd if 'gp_split_redo_kernel' in n]) == 1, bwd


@pytest.mark.gpu
def test_a_block_called_on_its_own_keeps_its_backwards_launches_and_its_bits():
    """B1 and B2 are the critic pass's (critic_block's backward_tails): outside it the masked split and the block input's gradient stay
    launches of their own -- conv1's finish still writes conv2's planes (F1) -- and the values are those of the critic's call"""
    a = _block('SAME', False)
    b = copy.deepcopy(a)
    gy = _randn(SAME_SMALL, 2).cuda()
    params = list(a.parameters())
    for call in range(2):
        x0 = _randn(SAME_SMALL, 10 + call).cuda()
        x = x0.clone().requires_grad_(True)
        box = {}
        names = _kernel_names(lambda: box.__setitem__('got', torch.autograd.grad(a(x, None), [x] + params, gy)))
        for got, want in zip(box['got'], _run_block(b, x0, gy, True)[1:]):
            assert _same_bits(got, want), call
    assert not [n for n in names if 'conv_pair_reduce_tail_kernel' in n], names
    assert [n for n in names if 'gp_split_hist_kernel' in n] and [n for n in names if 'conv_block_dx_kernel' in n], names
    assert len([n for n in names if 'conv_finish_tail_kernel' in n]) == 1, names


@pytest.mark.gpu
def test_a_reader_in_eval_mode_gets_no_fused_launch():
    a = _block('SAME', False)
    b = copy.deepcopy(a)
    gy = _randn(SAME_SMALL, 2).cuda()
    _run_block(a, _randn(SAME_SMALL, 1).cuda(), gy, True)
    _run_block(b, _randn(SAME_SMALL, 1).cuda(), gy, False)
    for blk in (a, b):
        blk.conv2.eval()                # F1's reader measures now: conv1's finish must not write its planes
        blk.conv1.eval()                # ... and B1's reader too
    x = _randn(SAME_SMALL, 3).cuda()
    box = {}
    names = _kernel_names(lambda: box.__setitem__('got', _run_block(a, x, gy, True)))
    assert not [n for n in names if 'conv_finish_tail_kernel' in n], names
    assert [n for n in names if 'conv_absmax_kernel' in n] and [n for n in names if 'gp_absmax_kernel' in n], names
    # B2 has no reader: it stays fused, alone in the pair's second launch
    assert len([n for n in names if 'conv_pair_reduce_tail_kernel' in n]) == 1, names
    for got, want in zip(box['got'], _run_block(b, x, gy, False)):
        assert _same_bits(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("off", FLAGS[1:])
def test_each_part_switched_off_alone_keeps_the_bits(off):
    a = _block('SAME', False)
    b = copy.deepcopy(a)
    for call in range(2):
        x, gy = _randn(SAME_SMALL, 10 + call).cuda(), _randn(SAME_SMALL, 20 + call).cuda()
        with _route(**{off: False}):
            got = _run_block(a, x, gy, True)
        for g, w in zip(got, _run_block(b, x, gy, False)):
            assert _same_bits(g, w), (off, call)
