"""The critic as a network against tests/critic_reference.py, a float64 restatement of the reference project's critic layer by layer.

CPU (default suite): the reference itself against `make_discriminator(spectral=False).double()` run by torch -- output, every parameter
gradient and the input gradient at 1e-12, for the three heads with sum and mean pooling; forced masks equal to its own signs change nothing.

GPU: the four train.CONFIGS critics on the HIP route (block convolutions of conv.py, the narrow first layers, the fused spectral-norm op)
at the smallest batch where every convolution with >= 128 input channels is taken by the fast kernel, in eval mode and in two successive
training-mode calls (the second on history-scaled splits and an advanced u, v), one AC_GAN / mean-pooling critic without spectral
normalisation, and one fully_diff_spectral critic: output, input gradient and every parameter gradient.  The reference is given the signs
the HIP network applied its ReLUs to (forward hooks on the identity bn1 / bn2 modules and on the last block); any element where those differ
from the reference's own float64 signs must lie within 1e-4 of zero relative to its tensor's maximum.

BOUNDS: four times the worst error either route (HIP, torch / MIOpen fp32 with the same spectral op) showed against the reference over the
four recipes, rounded up to one digit, capped at the project's 1e-4 (profiles/critic_parity.txt; `PYTHONPATH=. python
tests/test_critic_gpu.py` prints that table)."""
import pytest
import torch

import critic_reference as R

MASK_BAND = 1e-4
CEILING = 1e-4
# relative error = max |a - ref| / max |ref| per tensor, the worst tensor of a kind.  Worst over the four recipes (eval, training calls 1 and 2),
# the larger of the two routes, x 4, rounded up to one digit (profiles/critic_parity.txt):
#   out     hip 6.04e-07  torch fp32 6.64e-07  -> 2.7e-06 -> 3e-06
#   dx      hip 8.00e-07  torch fp32 7.69e-07  -> 3.2e-06 -> 4e-06
#   conv_w  hip 4.34e-07  torch fp32 1.45e-06  -> 5.8e-06 -> 6e-06
#   bias    hip 3.92e-07  torch fp32 3.46e-07  -> 1.6e-06 -> 2e-06
#   head    hip 1.17e-06  torch fp32 9.49e-07  -> 4.7e-06 -> 5e-06
BOUNDS = dict(out=3e-6, dx=4e-6, conv_w=6e-6, bias=2e-6, head=5e-6)
assert all(b <= CEILING for b in BOUNDS.values())

RECIPE_BATCH = {'cifar10_uncond': 4, 'cifar10_cond': 2, 'stl10_uncond': 8, 'tinyimagenet_cond_sa': 2}
SYNTHETIC = dict(input_image_shape=(16, 16, 3), block_sizes=(128, 256), resamples=('DOWN', 'SAME'), number_of_classes=10, type='AC_GAN',
                 spectral=False, sum_pool=False)


def _kind(name):
    if name.startswith('blocks.'):
        return 'conv_w' if name.endswith('.weight') else 'bias'
    return 'head'


def _rel(a, ref):
    return float((a.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max().clamp_min(1e-300))


def _loss(out, weights):
    outs = out if isinstance(out, tuple) else (out,)
    return sum((o * w.to(o.dtype)).sum() for o, w in zip(outs, weights))


def _inputs(kw, batch, device, seed, dtype=torch.float32):
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    H, W, C = kw['input_image_shape']
    x = (torch.rand(batch, H, W, C, generator=g, dtype=torch.float64) * 2 - 1).to(dtype).to(device).requires_grad_(True)
    cls = torch.randint(0, kw['number_of_classes'], (batch, 1), generator=g, dtype=torch.int32).to(device)
    weights = (torch.randn(batch, 1, generator=g, dtype=torch.float64).to(device),
               torch.randn(batch, kw['number_of_classes'], generator=g, dtype=torch.float64).to(device))
    return x, cls, weights


def _module(kw, device, seed=5, dtype=torch.float32):
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(seed)
    D = make_discriminator(**kw)
    with torch.no_grad():                           # (the biases start at zero: a bias that is dropped somewhere would not show)
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.to(dtype).to(device)


def _reference(state, kw, x, cls, weights, iterations, masks=None):
    """-> (critic, outputs, {name: gradient}) of the float64 network on copies of x and the state dict's tensors"""
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=iterations, masks=masks, **kw)
    x64 = x.detach().double().requires_grad_(True)
    out = critic(x64, cls)
    names = list(params)
    grads = torch.autograd.grad(_loss(out, weights), [x64] + [params[n] for n in names])
    return critic, out, dict(zip(['x'] + names, grads))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the reference against torch running the same module in float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", [None, 'PROJECTIVE', 'AC_GAN'])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_reference_equals_the_float64_module_on_the_cpu(head, sum_pool):
    for widths in ((32, 64, 64), (32, 32, 64)):         # the SAME block without and with its 1x1 shortcut
        kw = dict(input_image_shape=(16, 16, 3), block_sizes=widths, resamples=('DOWN', 'DOWN', 'SAME'), number_of_classes=7, type=head,
                  spectral=False, sum_pool=sum_pool)
        D = _module(kw, 'cpu', dtype=torch.float64)
        x, cls, weights = _inputs(kw, 3, 'cpu', 1, torch.float64)
        out = D(x, cls)
        names = [n for n, _ in D.named_parameters()]
        grads = dict(zip(['x'] + names, torch.autograd.grad(_loss(out, weights), [x] + list(D.parameters()))))
        critic, out64, grads64 = _reference(D.state_dict(), kw, x, cls, weights, 0)
        assert len(critic.pre) == R.relu_count(widths)
        for a, b in zip(out if isinstance(out, tuple) else (out,), out64 if isinstance(out64, tuple) else (out64,)):
            assert a.shape == b.shape and _rel(a, b) < 1e-12
        assert set(grads) == set(grads64)
        for n in grads:
            assert grads[n].shape == grads64[n].shape and _rel(grads[n], grads64[n]) < 1e-12, n
        # its own signs, forced: nothing changes
        masks = [h > 0 for h in critic.pre]
        forced, outf, gradsf = _reference(D.state_dict(), kw, x, cls, weights, 0, masks)
        assert R.mask_disagreement(masks, forced.pre) == (0.0, 0)
        for a, b in zip(outf if isinstance(outf, tuple) else (outf,), out64 if isinstance(out64, tuple) else (out64,)):
            assert _rel(a, b) < 1e-14
        for n in grads64:
            assert _rel(gradsf[n], grads64[n]) < 1e-14, n


def test_a_wrong_forced_mask_is_seen():
    """an element far from zero whose forced mask is flipped: the disagreement measure reports it and the gradients move"""
    kw = dict(input_image_shape=(16, 16, 3), block_sizes=(32, 32, 32), resamples=('DOWN', 'DOWN', 'SAME'), number_of_classes=7, type=None,
              spectral=False, sum_pool=True)
    D = _module(kw, 'cpu', dtype=torch.float64)
    x, cls, weights = _inputs(kw, 2, 'cpu', 2, torch.float64)
    critic, out64, grads64 = _reference(D.state_dict(), kw, x, cls, weights, 0)
    masks = [(h > 0).contiguous() for h in critic.pre]
    h = critic.pre[1]
    at = int(h.abs().argmax())
    masks[1].view(-1)[at] = not bool(masks[1].view(-1)[at])
    forced, outf, gradsf = _reference(D.state_dict(), kw, x, cls, weights, 0, masks)
    worst, count = R.mask_disagreement(masks, forced.pre)
    assert count >= 1 and worst == 1.0           # (the layers behind it see other pre-activations: their signs may differ too)
    assert _rel(gradsf['blocks.1.conv1.conv.weight'], grads64['blocks.1.conv1.conv.weight']) > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
class _Probe:
    """forward hooks that keep the fp32 tensors the network applies its ReLUs to, and a count of the convolutions with >= 128 input
    channels that the fast kernel turned down"""

    def __init__(self, D):
        from wc_gan_amd import conv as C
        self.D, self.C, self.rec, self.missed, self.handles = D, C, {}, [], []
        for i, blk in enumerate(D.blocks):
            for part in ('bn1', 'bn2'):
                assert not list(getattr(blk, part).parameters()), "critic norm 'n': bn1 / bn2 are identities"
                self.handles.append(getattr(blk, part).register_forward_hook(self._keep(f'{i}.{part}')))
        self.handles.append(D.blocks[-1].register_forward_hook(self._keep('last')))

    def _keep(self, key):
        def hook(_mod, _inp, out):
            self.rec[key] = out.detach()
        return hook

    def __enter__(self):
        self.orig = self.C.fast_conv_or_none

        def counting(x, w, *a, **k):
            y = self.orig(x, w, *a, **k)
            if y is None and x.shape[-1] >= 128:
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
        keys = [k for i in range(len(self.D.blocks)) for k in ((f'{i}.bn1',) if i else ()) + (f'{i}.bn2',)] + ['last']
        return [self.rec[k] > 0 for k in keys]


def _call(D, probe, kw, x, cls, weights, expect_fast=True):
    """One forward + backward of the module and of the reference built from the state the module had before the call.
    -> {kind: worst relative error}; asserts the mask band, the fast route and (training mode) the advanced u, v."""
    state = {k: v.detach().clone() for k, v in D.state_dict().items()}
    probe.rec.clear(); del probe.missed[:]
    with probe:
        out = D(x, cls)
        names = [n for n, _ in D.named_parameters()]
        grads = dict(zip(['x'] + names, torch.autograd.grad(_loss(out, weights), [x] + list(D.parameters()))))
    if expect_fast:
        assert probe.missed == [], probe.missed
    masks = probe.masks()
    iterations = int(kw.get('spectral_iterations', 1)) if D.training else 0
    critic, out64, grads64 = _reference(state, kw, x, cls, weights, iterations, masks)
    worst, count = R.mask_disagreement(masks, critic.pre)
    print(f"  relu masks: {count} elements differ from the float64 signs, the farthest at {worst:.2e} of its tensor's maximum")
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
        assert critic.uv, "no spectrally normalised layer was met"
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
    D = _module(kw, 'cuda')
    D.train(training)
    probe = _Probe(D)
    before = G.FAST_CONV
    G.FAST_CONV = fast
    try:
        out = []
        for call in range(2 if training else 1):
            x, cls, weights = _inputs(kw, batch, 'cuda', 10 + call)
            out.append(_call(D, probe, kw, x, cls, weights, expect_fast=fast))
    finally:
        G.FAST_CONV = before
        probe.close()
    return out


def _check(errs, label):
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (label, k, v, BOUNDS[k])


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", list(RECIPE_BATCH))
def test_recipe_critic_in_eval_mode(recipe):
    """iterations = 0, no scale history: output, input gradient and every parameter gradient"""
    from wc_gan_amd.train import CONFIGS
    kw = CONFIGS[recipe]['discriminator']
    errs, = _critic_errors(kw, RECIPE_BATCH[recipe], training=False)
    _check(errs, f"critic {recipe} eval")


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", list(RECIPE_BATCH))
def test_recipe_critic_in_two_training_calls(recipe):
    """the second call runs on history-scaled splits and a (u, v) the first call advanced; each call against its own reference"""
    from wc_gan_amd.train import CONFIGS
    kw = CONFIGS[recipe]['discriminator']
    for call, errs in enumerate(_critic_errors(kw, RECIPE_BATCH[recipe], training=True)):
        _check(errs, f"critic {recipe} train call {call + 1}")


@pytest.mark.gpu
def test_unnormalised_ac_gan_critic_with_mean_pooling():
    """what no shipped recipe uses: spectral=False, the AC_GAN class head, mean pooling, a SAME block that widens (1x1 shortcut at 8x8)"""
    for call, errs in enumerate(_critic_errors(SYNTHETIC, 4, training=True)):
        _check(errs, f"critic synthetic AC_GAN train call {call + 1}")


@pytest.mark.gpu
def test_fully_differentiable_spectral_critic():
    """fully_diff_spectral=True: the gradient flows through sigma = u^T W v"""
    from wc_gan_amd.train import CONFIGS
    kw = dict(CONFIGS['cifar10_uncond']['discriminator'], fully_diff_spectral=True)
    for call, errs in enumerate(_critic_errors(kw, RECIPE_BATCH['cifar10_uncond'], training=True)):
        _check(errs, f"critic cifar10_uncond fully_diff_spectral train call {call + 1}")


if __name__ == '__main__':
    from wc_gan_amd.train import CONFIGS
    kinds = ('out', 'dx', 'conv_w', 'bias', 'head')
    print(f"{'critic':<44}{'route':<12}" + ''.join(f"{k:>10}" for k in kinds), flush=True)
    rows = [(name, CONFIGS[name]['discriminator'], batch) for name, batch in RECIPE_BATCH.items()]
    rows += [('synthetic AC_GAN', SYNTHETIC, 4),
             ('cifar10_uncond fully_diff', dict(CONFIGS['cifar10_uncond']['discriminator'], fully_diff_spectral=True), 4)]
    worst = {route: dict.fromkeys(kinds, 0.0) for route in ('hip', 'torch fp32')}
    for i, (name, kw, batch) in enumerate(rows):
        for training in (False, True):
            for route, fast in (('hip', True), ('torch fp32', False)):
                for call, errs in enumerate(_critic_errors(kw, batch, training, fast)):
                    label = f"{name} {'train call ' + str(call + 1) if training else 'eval'}"
                    print(f"{label:<44}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" for k in kinds), flush=True)
                    if i < len(RECIPE_BATCH):
                        for k in kinds:
                            worst[route][k] = max(worst[route][k], errs[k])
    for route in worst:
        print(f"{'worst over the four recipes':<44}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in kinds), flush=True)
