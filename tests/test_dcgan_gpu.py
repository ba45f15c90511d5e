"""arch='dcgan' as networks on the GPU.

The DC critic on the HIP route (the narrow first layer 3 -> 64, the 64-wide tiles, LeakyReLU in the operand split, the fused spectral-norm
op) against tests/dcgan_reference.py with forced activation masks: the CIFAR-10 recipe's critic (widths 64 ... 512, 32x32, spectral,
type None) at batch 8 -- the smallest batch at which the 4x4-grid layers fill a 128-point tile -- and a synthetic non-spectral AC_GAN critic
(16x16x3, widths 64, 128, 128, batch 2); in eval mode and in two successive training calls; output, input gradient and every parameter
gradient.  Then: no torch convolution operator in a critic update pass or a generator pass; the DC generator at recipe widths on two routes
(HIP deconvolutions / torch's) on identical recorded masks; the 256-channel site's planes hand-off; two eager and one replayed trainer step.

BOUNDS follow tests/test_critic_gpu.py's protocol: both routes (HIP; torch fp32 with the same spectral op) against the float64 reference,
four times the worse of the two per tensor kind, rounded up to one digit, capped at the project's 1e-4 (`PYTHONPATH=. python
tests/test_dcgan_gpu.py` prints the table kept in profiles/dcgan_parity.txt)."""
import pytest
import torch

import dcgan_reference as R

MASK_BAND = R.MASK_BAND
CEILING = 1e-4
# relative error = max |a - ref| / max |ref| per tensor, the worst tensor of a kind, worst over both critics and all three calls, the larger
# of the two routes, x 4, rounded up to one digit (profiles/dcgan_parity.txt):
#   out     hip 1.44e-06  torch fp32 2.10e-06  -> 8.4e-06 -> 9e-06
#   dx      hip 6.10e-07  torch fp32 1.02e-06  -> 4.1e-06 -> 5e-06
#   conv_w  hip 1.42e-06  torch fp32 1.04e-06  -> 5.7e-06 -> 6e-06
#   bias    hip 2.17e-06  torch fp32 1.43e-06  -> 8.7e-06 -> 9e-06
#   head    hip 2.91e-07  torch fp32 3.79e-07  -> 1.6e-06 -> 2e-06
BOUNDS = dict(out=9e-6, dx=5e-6, conv_w=6e-6, bias=9e-6, head=2e-6)
assert all(b <= CEILING for b in BOUNDS.values())

RECIPE_BATCH = 8
SYNTHETIC = dict(input_image_shape=(16, 16, 3), block_sizes=(64, 128, 128), resamples=('SAME', 'DOWN', 'SAME'), number_of_classes=10,
                 type='AC_GAN', spectral=False, arch='dcgan')
GENERATOR_BOUND = 2e-5          # the ResNet generator's two-route bound (tests/test_producer_gpu.py)


def _recipe():
    from wc_gan_amd.train import DCGAN_CONFIGS
    return DCGAN_CONFIGS['cifar10_dcgan_uncond']


def _kind(name):
    if name.startswith('blocks.'):
        return 'conv_w' if name.endswith('.weight') else 'bias'
    return 'head'


def _rel(a, ref):
    return float((a.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max().clamp_min(1e-300))


def _loss(out, weights):
    outs = out if isinstance(out, tuple) else (out,)
    return sum((o * w.to(o.dtype)).sum() for o, w in zip(outs, weights))


def _inputs(kw, batch, seed):
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    H, W, C = kw['input_image_shape']
    x = (torch.rand(batch, H, W, C, generator=g, dtype=torch.float64) * 2 - 1).float().cuda().requires_grad_(True)
    weights = (torch.randn(batch, 1, generator=g, dtype=torch.float64).cuda(),
               torch.randn(batch, kw['number_of_classes'], generator=g, dtype=torch.float64).cuda())
    return x, weights


def _critic(kw, seed=5):
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(seed)
    D = make_discriminator(**kw)
    with torch.no_grad():                           # (the biases start at zero: a bias that is dropped somewhere would not show)
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.cuda()


class _Probe:
    """forward hooks that keep the fp32 tensors the network applies its LeakyReLUs to (every block's output), and a list of the
    convolutions with >= 64 input channels that the fast kernel turned down"""

    def __init__(self, D):
        from wc_gan_amd import conv as C
        self.D, self.C, self.rec, self.missed = D, C, {}, []
        self.handles = [blk.register_forward_hook(self._keep(i)) for i, blk in enumerate(D.blocks)]

    def _keep(self, key):
        def hook(_mod, _inp, out):
            self.rec[key] = out.detach()
        return hook

    def __enter__(self):
        self.orig = self.C.fast_conv_or_none

        def counting(x, w, *a, **k):
            y = self.orig(x, w, *a, **k)
            if y is None and x.shape[-1] >= 64:
                self.missed.append((tuple(x.shape), tuple(w.shape)))
            return y
        self.C.fast_conv_or_none = counting
        return self

    def __exit__(self, *exc):
        self.C.fast_conv_or_none = self.orig

    def close(self):
        for h in self.handles:
            h.remove()

    def masks(self):
        return [self.rec[i] > 0 for i in range(len(self.D.blocks))]


def _call(D, probe, kw, x, weights, expect_fast):
    """One forward + backward of the module and of the reference built from the state the module had before the call.
    -> {kind: worst relative error}; asserts the mask band, the fast route and (training mode) the advanced u, v."""
    state = {k: v.detach().clone() for k, v in D.state_dict().items()}
    probe.rec.clear(); del probe.missed[:]
    with probe:
        out = D(x)
        names = [n for n, _ in D.named_parameters()]
        grads = dict(zip(['x'] + names, torch.autograd.grad(_loss(out, weights), [x] + list(D.parameters()))))
    if expect_fast:
        assert probe.missed == [], probe.missed
    masks = probe.masks()
    iterations = int(kw.get('spectral_iterations', 1)) if D.training else 0
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=iterations, masks=masks, **kw)
    x64 = x.detach().double().requires_grad_(True)
    out64 = critic(x64)
    grads64 = dict(zip(['x'] + list(params), torch.autograd.grad(_loss(out64, weights), [x64] + list(params.values()))))
    assert len(critic.pre) == R.leaky_count(kw['block_sizes']) == len(masks)
    worst, count = R.mask_disagreement(masks, critic.pre)
    print(f"  leaky masks: {count} elements differ from the float64 signs, the farthest at {worst:.2e} of its tensor's maximum")
    assert worst <= MASK_BAND, (worst, count)
    errs = dict(out=0.0, dx=0.0, conv_w=0.0, bias=0.0, head=0.0)
    for a, b in zip(out if isinstance(out, tuple) else (out,), out64 if isinstance(out64, tuple) else (out64,)):
        assert a.shape == b.shape
        errs['out'] = max(errs['out'], _rel(a, b))
    assert set(grads) == set(grads64)
    for n, g in grads.items():
        k = 'dx' if n == 'x' else _kind(n)
        assert g.shape == grads64[n].shape
        errs[k] = max(errs[k], _rel(g, grads64[n]))
    if kw['spectral']:
        sd = D.state_dict()
        assert len(critic.uv) == len(kw['block_sizes']) + 1, "every convolution and the dense head are spectrally normalised"
        for prefix, (u, v) in critic.uv.items():
            for got, want in ((sd[prefix + '.sn_u'], u), (sd[prefix + '.sn_v'], v)):
                d = float((got.double().cpu() - torch.from_numpy(want)).abs().max())
                assert d < 2e-5, (prefix, d)            # test_spectral.py's bound on u, v
            if not D.training:
                assert torch.equal(sd[prefix + '.sn_u'], state[prefix + '.sn_u'])
    return errs


def _critic_errors(kw, batch, training, fast=True):
    """-> [errors of each call]: one eval-mode call, or two successive training-mode calls on one module"""
    import wc_gan_amd.generator as G
    D = _critic(kw)
    D.train(training)
    probe = _Probe(D)
    before = G.FAST_CONV
    G.FAST_CONV = fast
    try:
        out = []
        for call in range(2 if training else 1):
            x, weights = _inputs(kw, batch, 10 + call)
            out.append(_call(D, probe, kw, x, weights, expect_fast=fast))
    finally:
        G.FAST_CONV = before
        probe.close()
    return out


def _check(errs, label):
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (label, k, v, BOUNDS[k])


CRITICS = {'cifar10_dcgan': (lambda: _recipe()['discriminator'], RECIPE_BATCH), 'synthetic': (lambda: SYNTHETIC, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(CRITICS))
def test_dc_critic_in_eval_mode(which):
    """iterations = 0, no scale history: output, input gradient and every parameter gradient"""
    kw, batch = CRITICS[which][0](), CRITICS[which][1]
    errs, = _critic_errors(kw, batch, training=False)
    _check(errs, f"dc critic {which} eval")


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(CRITICS))
def test_dc_critic_in_two_training_calls(which):
    """the second call runs on history-scaled leaky splits and a (u, v) the first call advanced; each call against its own reference"""
    kw, batch = CRITICS[which][0](), CRITICS[which][1]
    for call, errs in enumerate(_critic_errors(kw, batch, training=True)):
        _check(errs, f"dc critic {which} train call {call + 1}")


def _op_and_kernel_names(fn):
    """-> (operator names, device kernel names) of one profiled call of fn"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = list(prof.events())
    ops = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CPU]
    kernels = [e.name for e in ev if e.device_type == torch.autograd.DeviceType.CUDA]
    return ops, kernels


def _convolution_ops(ops):
    return sorted({n for n in ops if n.startswith(('aten::convolution', 'aten::miopen_convolution', 'aten::cudnn_convolution',
                                                    'aten::_convolution', 'aten::conv2d', 'aten::conv_transpose2d'))})


@pytest.mark.gpu
def test_critic_update_pass_runs_no_torch_convolution():
    """forward + backward of the recipe's critic as a critic update runs it (the images need no gradient): every convolution, its data
    gradient and its weight gradient is a HIP kernel of csrc/wc_conv.hip -- the profile holds no convolution operator of torch's.
    (In the GENERATOR update the first layer's data gradient, 64 -> 3 channels, is MIOpen's, as the ResNet critic's is.)"""
    kw = _recipe()['discriminator']
    D = _critic(kw).train()
    x, weights = _inputs(kw, RECIPE_BATCH, 3)
    x = x.detach()

    def update():
        for p in D.parameters():
            p.grad = None
        _loss(D(x), weights).backward()
    update()                                            # (the sites' first calls measure: profile the steady state)
    ops, kernels = _op_and_kernel_names(update)
    assert ops, "the profiler reported no operators"
    assert _convolution_ops(ops) == [], _convolution_ops(ops)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in D.parameters())
    if kernels:
        joined = ' '.join(kernels)
        for name in ('conv_f16x3_kernel', 'conv_wrw_kernel', 'conv_fwd_narrow_kernel', 'conv_wrw_narrow_kernel', 'conv_split_hist_kernel',
                     'conv_leaky_bwd_kernel'):
            assert name in joined, name


def _generator(batch_norm=False):
    from wc_gan_amd.generator import make_generator
    torch.manual_seed(7)
    kw = dict(_recipe()['generator'])
    G = make_generator(**kw).cuda().train()
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return G


@pytest.fixture(scope="module")
def generator_routes():
    """One DC generator at recipe widths, batch 64 (the first site then has 1024 rows for its 512 channels), forward + backward on the HIP
    deconvolutions and on torch's (generator.FAST_CONV = False) with the second route's sites saving the first route's ReLU masks."""
    import wc_gan_amd.functional as WF
    import wc_gan_amd.generator as gen
    G = _generator()
    z = torch.randn(64, 128, device='cuda')
    with torch.no_grad():
        G(z)                                            # moving statistics and scale histories off their initial state
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    gimg = torch.randn(64, 32, 32, 3, device='cuda')
    res, masks, handed = {}, [], []
    orig = gen.fast_conv_mod.fast_conv_or_none

    def spy(x, w, *a, **k):
        y = orig(x, w, *a, **k)
        handed.append((tuple(x.shape), k.get('kind', a[1] if len(a) > 1 else 'same'), getattr(x, '_wc_planes', None) is not None, y is not None))
        return y
    for fast in (True, False):
        G.load_state_dict(state)
        for p in G.parameters():
            p.grad = None
        gen.FAST_CONV = fast
        gen.fast_conv_mod.fast_conv_or_none = spy if fast else orig
        try:
            WF.MASK_TAP = {'record': masks} if fast else {'replay': list(masks)}
            img = G(z)
            assert fast or not WF.MASK_TAP['replay'], "the two routes did not run the same ReLU'd sites"
            WF.MASK_TAP = None
            img.backward(gimg)
            res[fast] = (img.detach().clone(), {n: p.grad.clone() for n, p in G.named_parameters()})
        finally:
            gen.FAST_CONV = True
            gen.fast_conv_mod.fast_conv_or_none = orig
            WF.MASK_TAP = None
    return G, z, gimg, res, masks, handed


@pytest.mark.gpu
def test_dc_generator_on_hip_deconvolutions_equals_torchs_on_the_same_masks(generator_routes):
    G, z, gimg, res, masks, handed = generator_routes
    assert len(masks) == 4, len(masks)                  # len(blocks) + 1 ReLU'd WC sites, each with a one-bit mask
    assert [h[0] for h in handed if h[1] == 'up'] == [(64, 4, 4, 512), (64, 8, 8, 512), (64, 16, 16, 256)]
    assert all(h[3] for h in handed if h[1] == 'up'), handed      # the three deconvolutions ran on the HIP kernel
    out = _rel(res[True][0], res[False][0])
    print("dc generator, HIP route vs torch's deconvolutions on the same masks: image", f"{out:.2e}")
    assert out < GENERATOR_BOUND
    # gradients that are zero in exact arithmetic (the bias of a deconvolution in front of a WC site: the site removes the mean) are rounding
    # noise on either route: bounded by 2e-6 of the largest gradient's maximum instead, as tests/test_producer_gpu.py does
    top = max(float(g.abs().max()) for g in res[False][1].values())
    bad = {}
    for n, a in res[True][1].items():
        b = res[False][1][n]
        d = float((a.double() - b.double()).abs().max())
        rel_own, rel_top = d / max(float(b.abs().max()), 1e-30), d / top
        print(f"  {n:<44} {rel_own:.2e} of its own maximum, {rel_top:.2e} of the largest gradient's")
        if rel_own > GENERATOR_BOUND and rel_top > 2e-6:
            bad[n] = (rel_own, rel_top)
    assert not bad, bad


@pytest.mark.gpu
def test_the_256_channel_site_hands_planes_to_its_deconvolution(generator_routes):
    """Block 2's site (64 x 16 x 16 x 256) writes the 256 -> 128 deconvolution's operand planes from K3's epilogue; the 512-channel sites
    return fp32 and are split by the history-scaled split -- so a steady-state forward launches exactly two split kernels, both of
    512-channel tensors, and none in front of block 2's deconvolution."""
    from wc_gan_amd import conv as C
    G, z, gimg, res, masks, handed = generator_routes
    ups = [h for h in handed if h[1] == 'up']
    assert [h[2] for h in ups] == [False, False, True], ups
    split_calls = []
    orig = C.split_planes

    def spy(x, *a, **k):
        split_calls.append((tuple(x.shape), k.get('role', 'x')))
        return orig(x, *a, **k)
    C.split_planes = spy
    try:
        ops, kernels = _op_and_kernel_names(lambda: G(z))
    finally:
        C.split_planes = orig
    assert split_calls == [((64, 4, 4, 512), 'x'), ((64, 8, 8, 512), 'x')], split_calls
    assert _convolution_ops(ops) == [], _convolution_ops(ops)
    if kernels:
        splits = [n for n in kernels if 'conv_split' in n]         # (conv_absmax_kernel also measures the weights: not counted)
        assert len(splits) == 2 and all('conv_split_hist_kernel' in n for n in splits), splits


@pytest.mark.gpu
def test_generator_pass_runs_no_torch_convolution(generator_routes):
    G, z, gimg, *_ = generator_routes

    def both():
        for p in G.parameters():
            p.grad = None
        G(z).backward(gimg)
    both()
    ops, kernels = _op_and_kernel_names(both)
    assert ops, "the profiler reported no operators"
    assert _convolution_ops(ops) == [], _convolution_ops(ops)


@pytest.mark.gpu
def test_trainer_runs_eager_and_replayed_steps():
    """build_trainer on the CIFAR-10 DCGAN-SN configuration at batch 64: two eager steps and one captured-and-replayed step; finite losses,
    every parameter of both networks moved, the split records' second-pass counters readable."""
    from wc_gan_amd import conv as C
    from wc_gan_amd.train import build_trainer
    cfg = _recipe()
    torch.manual_seed(0)
    tr = build_trainer(cfg, 'cuda', batch_size=64)
    assert (tr.training_ratio, tr.gbm) == (1, 1)
    g = torch.Generator(device='cpu'); g.manual_seed(1)
    reals = [(torch.rand(64, 32, 32, 3, generator=g) * 2 - 1).cuda()]
    before = {id(p): p.detach().clone() for net in (tr.G, tr.D) for p in net.parameters()}
    losses = [tr.step(reals) for _ in range(2)]
    replay = tr.capture(reals, warmup=1)
    losses.append(replay())
    torch.cuda.synchronize()
    for d_loss, g_loss in losses:
        assert bool(torch.isfinite(d_loss)) and bool(torch.isfinite(g_loss)), losses
    # Every parameter moved -- with one exception that is arithmetic, not a missing gradient: the hinge loss's gradient with respect to the
    # critic's output bias is (active margins among the generated images - active margins among the real ones) / 64, EXACTLY 0 in every
    # update in which all 128 margins are active, which is the state of the first updates from initialisation; Adam then leaves the bias
    # where it was.  The bias may stand still only on that evidence: the optimiser has stepped it, every gradient it ever received was
    # exactly zero (Adam's second-moment accumulator is a sum of squares: 0 says so), and the wiring is checked directly -- d sum(D(x)) /
    # d bias is the batch size.
    for net, label in ((tr.G, 'G'), (tr.D, 'D')):
        for n, p in net.named_parameters():
            assert bool(torch.isfinite(p).all()), (label, n)
            if label == 'D' and n == 'out.bias' and torch.equal(p.detach(), before[id(p)]):
                st = tr.opt_d.state[p]
                assert float(st['step']) >= 3 and float(st['exp_avg_sq'].abs().max()) == 0.0, (n, st)
                p.grad = None
                tr._d(reals[0], None).sum().backward()
                assert float(p.grad) == 64.0, p.grad
                continue
            assert not torch.equal(p.detach(), before[id(p)]), (label, n)
    records = 0
    for net in (tr.G, tr.D):
        for m in net.modules():
            for role, (hist, seeded) in m.__dict__.get('_wc_split_hist', {}).items():
                assert seeded and int(hist.view(torch.int32)[C.HIST_REDO]) >= 0
                records += 1
    # input and output-gradient records of the 6 block convolutions of the critic and of the 3 deconvolutions -- less the input record of
    # the 256 -> 128 deconvolution, whose operand arrives as planes
    assert records >= 12 + 5, records


if __name__ == '__main__':
    kinds = ('out', 'dx', 'conv_w', 'bias', 'head')
    print(f"{'critic':<44}{'route':<12}" + ''.join(f"{k:>10}" for k in kinds), flush=True)
    worst = {route: dict.fromkeys(kinds, 0.0) for route in ('hip', 'torch fp32')}
    for name, (make, batch) in CRITICS.items():
        for training in (False, True):
            for route, fast in (('hip', True), ('torch fp32', False)):
                for call, errs in enumerate(_critic_errors(make(), batch, training, fast)):
                    label = f"{name} {'train call ' + str(call + 1) if training else 'eval'}"
                    print(f"{label:<44}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" for k in kinds), flush=True)
                    for k in kinds:
                        worst[route][k] = max(worst[route][k], errs[k])
    for route in worst:
        print(f"{'worst':<44}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in kinds), flush=True)
