"""GPU tests of the passes between the critic's convolutions on the HIP route: the masked split with the bias
gradient's partial rows, the residual operand of the k-split finish, the block-input gradient in one launch, and the critic block as one
autograd node.  Nothing is re-rounded anywhere, so every comparison is torch.equal: the fused route against the separate nodes.
torch.equal compares values: it does not tell -0 from +0.  Where the two routes can differ in a zero's sign -- the masked split writes
t * 0 = -0 for a negative t where threshold_backward writes +0 -- the test says so and compares the bits with the tensor that has them."""
import copy
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from test_conv_dispatch_gpu import _kernel_names


class _Site:
    training = True


def _signed_zeros_(a):
    """exact +0, -0 and (from the normal draw) negative values in the mask tensor"""
    flat = a.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return a


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the masked split with the column sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 8, 128), (3, 4, 4, 64)])
def test_masked_split_leaves_the_planes_rows_and_record_of_the_split_of_the_masked_tensor(shape):
    from wc_gan_amd import conv as C
    t = _randn(shape, 5).cuda()
    a = _signed_zeros_(_randn(shape, 6)).cuda()
    assert (a < 0).any() and (a == 0).any()
    mine, twin, pre = _Site(), _Site(), _Site()
    bits = lambda v: v.contiguous().view(torch.int16 if v.dtype == torch.float16 else torch.int32)
    redo = lambda site: int(site._wc_split_hist['g'][0][C.HIST_REDO:C.HIST_REDO + 1].view(torch.int32))
    # the first call measures, the second takes the history, an all-zero tensor, then one 2^12 times larger: the gated second pass
    calls = [t, (1.25 * t).contiguous(), torch.zeros_like(t), (4096.0 * t).contiguous()]
    for k, tt in enumerate(calls):
        got = C.split_planes_masked(tt, a, colsum=True, site=mine, role='g')
        want = C.split_planes(torch.ops.aten.threshold_backward(tt, a, 0), colsum=True, site=twin, role='g')
        for g, w, name in zip(got, want, ('hi', 'lo', 'scale', 'rows')):
            if name == 'scale':
                g, w = g[:1], w[:1]         # (the rest of that tensor is scratch of the measuring form)
            assert torch.equal(g, w), (k, name)
        assert torch.equal(mine._wc_split_hist['g'][0], twin._wc_split_hist['g'][0]), (k, 'record')
        # the comparison above is by value (the masked-out zeros of `got` carry t's sign, threshold_backward's are +0); bit for bit,
        # zeros' signs included, the planes, the scale, the rows and the record are those of the split of the premultiplied tensor
        same = C.split_planes((tt * (a > 0).to(tt.dtype)).contiguous(), colsum=True, site=pre, role='g')
        for g, w, name in zip(got, same, ('hi', 'lo', 'scale', 'rows')):
            assert torch.equal(bits(g[:1] if name == 'scale' else g), bits(w[:1] if name == 'scale' else w)), (k, name, 'bits')
        assert torch.equal(bits(mine._wc_split_hist['g'][0]), bits(pre._wc_split_hist['g'][0])), (k, 'record bits')
        assert redo(mine) == redo(twin) == (1 if k == 3 else 0), k
    # a site in eval mode (no record): the measuring twin, rows included
    got = C.split_planes_masked(t, a, colsum=True)
    want = C.split_planes(torch.ops.aten.threshold_backward(t, a, 0), colsum=True)
    assert all(torch.equal(g, w) for g, w in zip((got[0], got[1], got[2][:1], got[3]), (want[0], want[1], want[2][:1], want[3])))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the residual operand
# ---------------------------------------------------------------------------------------------------------------------------------
def _direct_epilogue_batch():
    """the smallest batch of a 128 -> 128 3x3 'same' layer at 8x8 whose forward does not share its tap loop (no workspace)"""
    from wc_gan_amd import conv as C
    for N in range(2, 1025, 2):
        p = C._plan('same', C._Shape((N, 8, 8, 128)), C._Shape((128, 128, 3, 3)))
        if p and p.ok and p.fwd_ws == 0:
            return N
    raise AssertionError("no direct-epilogue shape found")


def _residual_case(kind, shape):
    from wc_gan_amd import conv as C
    N, H, W, Cin = shape
    w0 = (_randn((128, Cin, 3, 3), 2) * 0.05).cuda().contiguous(memory_format=torch.channels_last)
    b0 = (_randn((128,), 3) * 0.1).cuda()
    x0 = _randn(shape, 1).cuda()
    out = (N, H // 2, W // 2, 128) if kind == 'down3' else (N, H, W, 128)
    s0, gy = _randn(out, 4).cuda(), _randn(out, 7).cuda()
    res = []
    for fused in (True, False):
        x, w, b, s = (v.clone().requires_grad_(True) for v in (x0, w0, b0, s0))
        y = C.fast_conv(x, w, b, kind, residual=s) if fused else C.fast_conv(x, w, b, kind) + s
        res.append((y.detach(),) + torch.autograd.grad(y, (x, w, b, s), gy))
    for a, b, name in zip(res[0], res[1], ('y', 'dx', 'dw', 'db', 'ds')):
        assert torch.equal(a, b), (kind, shape, name)
    assert torch.equal(res[0][4], gy)
    return C._plan(kind, C._Shape(shape), C._Shape((128, Cin, 3, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [('same', (2, 8, 8, 128)), ('down3', (2, 16, 16, 128))])
def test_residual_in_the_ksplit_finish_equals_the_add_behind_the_convolution(kind, shape):
    p = _residual_case(kind, shape)
    assert p.res and p.fwd_ws > 0       # the finish that takes the operand


@pytest.mark.gpu
def test_residual_behind_the_direct_epilogue():
    N = _direct_epilogue_batch()
    p = _residual_case('same', (N, 8, 8, 128))
    assert p.fwd_ws == 0 and not p.res


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the block input's gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,down", [((2, 8, 8, 128), False), ((2, 16, 16, 128), True), ((2, 6, 6, 132), False), ((1, 6, 10, 132), True)])
def test_block_input_gradient_equals_the_three_passes(shape, down):
    from wc_gan_amd import conv as C
    N, H, W, Cc = shape
    dx1 = _randn(shape, 1).cuda()
    x = _signed_zeros_(_randn(shape, 2)).cuda()
    other = _signed_zeros_(_randn((N, H // 2, W // 2, Cc) if down else shape, 3)).cuda()
    got = C.block_input_gradient(dx1, x, other, down)
    want = torch.ops.aten.threshold_backward(dx1, x, 0)
    if down:
        z = x.clone().requires_grad_(True)
        pooled = F.avg_pool2d(z.permute(0, 3, 1, 2), 2)
        want = want + torch.autograd.grad(pooled, z, other.permute(0, 3, 1, 2))[0]
    else:
        want = want + other
    assert torch.equal(got, want)
    # the masked-out value is +0 (threshold_backward's), whatever the sign of the gradient behind the mask
    zero = C.block_input_gradient(-dx1.abs(), x, torch.zeros_like(other), down)
    assert (x <= 0).any() and not torch.signbit(zero[x <= 0]).any() and not zero[x <= 0].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the block
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


def _run_block(blk, x0, gy, fused):
    from wc_gan_amd import conv as C
    x = x0.clone().requires_grad_(True)
    params = list(blk.parameters())
    old, C.FUSED_BLOCK = C.FUSED_BLOCK, fused
    try:
        y = blk(x, None)
        grads = torch.autograd.grad(y, [x] + params, gy)
    finally:
        C.FUSED_BLOCK = old
    return (y.detach(),) + grads


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("resample,shape", [('DOWN', (4, 16, 16, 128)), ('SAME', (2, 8, 8, 128))])
def test_fused_block_has_the_bits_of_the_separate_nodes(resample, shape, spectral):
    a = _block(resample, spectral)
    b = copy.deepcopy(a)
    assert a._fused_plans(torch.empty(shape, device='cuda')) is not None
    out = (shape[0], shape[1] // 2, shape[2] // 2, 128) if resample == 'DOWN' else shape
    names = ['y', 'dx'] + [n for n, _ in a.named_parameters()]
    for call in range(2):           # the first call measures every split, the second takes the sites' history
        x = (_randn(shape, 10 + call) * (1.0 + call)).cuda()
        gy = _randn(out, 20 + call).cuda()
        for got, want, name in zip(_run_block(a, x, gy, True), _run_block(b, x, gy, False), names):
            assert torch.equal(got, want), (call, name)
    for site in ('conv1', 'conv2') + (('shortcut',) if a.has_shortcut else ()):
        for role in ('x', 'g'):
            assert torch.equal(getattr(a, site)._wc_split_hist[role][0], getattr(b, site)._wc_split_hist[role][0]), (site, role)


@pytest.mark.gpu
@pytest.mark.parametrize("resample,shape", [('DOWN', (4, 16, 16, 128)), ('SAME', (2, 8, 8, 128))])
def test_fused_block_launches_no_elementwise_pass_of_torch(resample, shape):
    from wc_gan_amd import conv as C
    assert C.FUSED_BLOCK
    blk = _block(resample, False)
    x = _randn(shape, 1).cuda().requires_grad_(True)
    out = (shape[0], shape[1] // 2, shape[2] // 2, 128) if resample == 'DOWN' else shape
    gy = _randn(out, 2).cuda()
    params = list(blk.parameters())
    torch.autograd.grad(blk(x, None), [x] + params, gy)         # (the sites' first call, with its measuring launches)
    box = {}
    fwd = _kernel_names(lambda: box.__setitem__('y', blk(x, None)))
    bwd = _kernel_names(lambda: torch.autograd.grad(box['y'], [x] + params, gy))
    assert fwd and bwd
    assert not [n for n in fwd if 'CUDAFunctor_add' in n], fwd
    assert not [n for n in bwd if 'BinaryFunctor' in n or 'CUDAFunctor_add' in n or 'avg_pool2d_backward' in n], bwd
    assert not [n for n in bwd if 'FillFunctor' in n], bwd      # no zero gradient is made up for the node's second output (conv1's h)
    assert [n for n in bwd if 'conv_block_dx_kernel' in n] and [n for n in bwd if 'gp_split_hist_kernel' in n]
    assert [n for n in fwd if 'conv_ksplit_reduce_res_kernel' in n]


# ---------------------------------------------------------------------------------------------------------------------------------
# the critic, eager and captured
# ---------------------------------------------------------------------------------------------------------------------------------
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
    from wc_gan_amd import conv as C
    old, C.FUSED_BLOCK = C.FUSED_BLOCK, fused
    try:
        D.zero_grad(set_to_none=True)
        loss = _hinge(D, x)
        loss.backward()
    finally:
        C.FUSED_BLOCK = old
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in D.named_parameters()}


@pytest.mark.gpu
def test_critic_on_both_routes_and_captured():
    a = _critic()
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    xs = [(torch.rand((4, 32, 32, 3), generator=torch.Generator().manual_seed(s)) * 2 - 1).cuda() for s in (1, 2, 3)]
    eager = []
    for x in xs:                    # a: fused, b: separate nodes, three calls each
        la, ga = _critic_call(a, x, True)
        lb, gb = _critic_call(b, x, False)
        assert torch.equal(la, lb)
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n
        eager.append((la, ga))
    # c: the first call eager (it allocates and seeds the sites' records), then the fused route recorded once and replayed twice
    from wc_gan_amd import conv as C
    assert C.FUSED_BLOCK
    _critic_call(c, xs[0], True)
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
        assert torch.equal(loss.detach(), eager[k][0]), k
        for n, p in c.named_parameters():
            assert torch.equal(p.grad, eager[k][1][n]), (k, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# one WGAN-GP critic update on both routes.  The update as a whole is not reproducible bit for bit on EITHER route: two updates on
# the separate nodes, same seeds, differ in 11 gradients by an ulp or two and in the penalty's 't' / 'd' records (the penalty's tangent
# and adjoint passes go through MIOpen's data gradient of the image layers; tools/wgan_update_repro.py,
# profiles/critic_glue_wgan_repro.txt).  What the fused route computes -- the Wasserstein pass -- is compared bit for bit, taken from the
# .grad tensors at the moment the penalty starts; the penalty walks the blocks itself.  The gradients the optimizer is handed are
# compared within a few units in the last place, beside what two updates on the separate nodes differ by.
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgan_update(fused):
    from wc_gan_amd import conv as C
    from wc_gan_amd import penalty
    from wc_gan_amd.train import WGAN_CONFIGS, build_trainer
    n = 8
    old, C.FUSED_BLOCK = C.FUSED_BLOCK, fused
    real_penalty = penalty.gradient_penalty
    try:
        torch.manual_seed(11)       # (the modules' initialisation draws from the global generator)
        tr = build_trainer(WGAN_CONFIGS['cifar10_wgan_uncond'], 'cuda', batch_size=n, training_ratio=1, seed=3)
        assert tr.objective == 'wgan'
        g = torch.Generator().manual_seed(8)
        real, fake = ((torch.rand(n, 32, 32, 3, generator=g) * 2 - 1).cuda() for _ in range(2))
        eps = torch.rand(n, generator=g).cuda()
        seen, roles = {}, set()

        def spy(D, *a, **k):        # the Wasserstein pass is done, the penalty has not started
            seen.update({k_: p.grad.detach().clone() for k_, p in D.named_parameters()})
            for blk in D.blocks:
                for site in ('conv1', 'conv2', 'shortcut'):
                    roles.update(getattr(getattr(blk, site, None), '_wc_split_hist', {}))
            return real_penalty(D, *a, **k)
        penalty.gradient_penalty = spy
        final, step = {}, tr.opt_d.step

        def at_step(*a, **k):       # the gradients the optimizer is handed: the Wasserstein pass's plus the penalty's
            final.update({k_: p.grad.detach().clone() for k_, p in tr.D.named_parameters()})
            return step(*a, **k)
        tr.opt_d.step = at_step
        loss = tr.d_step(real, fake=fake, cls=None, eps=eps)
        tr.opt_d.step = step
    finally:
        C.FUSED_BLOCK = old
        penalty.gradient_penalty = real_penalty
    records = {}
    for i, blk in enumerate(tr.D.blocks):
        for site in ('conv1', 'conv2', 'shortcut'):
            for role, rec in getattr(getattr(blk, site, None), '_wc_split_hist', {}).items():
                records[(i, site, role)] = rec[0].clone()
    return loss.detach().clone(), seen, records, tr.last_penalty.detach().clone(), roles, final


@pytest.mark.gpu
def test_wgan_gp_update_on_both_routes():
    la, ga, ra, pa, roles_a, fa = _wgan_update(True)
    lb, gb, rb, pb, roles_b, fb = _wgan_update(False)
    lc, gc, rc, pc, roles_c, fc = _wgan_update(False)
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert ga.keys() == gb.keys() and ra.keys() == rb.keys()
    differ = {n: float((ga[n] - gb[n]).abs().max()) for n in ga if not torch.equal(ga[n], gb[n])}
    assert not differ, differ
    # the critic's pass keeps 'x' and 'g' records only, on either route: the penalty's own ('p', 't', 'd') are untouched by it ...
    assert roles_a == roles_b == {'x', 'g'}
    assert {r for _, _, r in ra} == {'x', 'g', 'p', 't', 'd'}
    # ... and the records the two routes leave behind agree wherever an update reproduces itself
    for key in ra:
        if key[2] in ('x', 'g', 'p'):
            assert torch.equal(ra[key], rb[key]), key
    # The gradients the optimizer sees (Wasserstein pass + penalty).  The two runs of the separate nodes show what an update's own
    # non-reproducibility is (printed); the routes must agree within ULPS units in the last place of each tensor's largest entry:
    # the penalty adds its gradient in fp32 to a bit-equal one, an order-dependent fp32 sum moves a result by a few ulp of its
    # size, and an error in the routes -- a wrong mask, a dropped term -- is of the size of the gradient itself, 2^19 times more.
    ULPS = 16
    worst = 0.0
    for n in fa:
        size = float(fb[n].abs().max())
        own, got = float((fb[n] - fc[n]).abs().max()), float((fa[n] - fb[n]).abs().max())
        allowed = ULPS * 2.0 ** -23 * size
        print(f"  {n}: max {size:.3e}, separate against itself {own:.2e}, fused against separate {got:.2e}, allowed {allowed:.2e}")
        assert got <= allowed, (n, got, allowed)
        worst = max(worst, own / size if size else 0.0)
    print(f"  two updates on the separate nodes differ by up to {worst:.2e} of a tensor's largest entry")
