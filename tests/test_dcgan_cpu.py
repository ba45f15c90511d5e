"""arch='dcgan' on the CPU (default suite): the DC critic and the DC generator as torch runs them in float64 against
tests/dcgan_reference.py at 1e-12, the two DCGAN-SN configurations' widths, resamples and WC sites, and the projection head's refusal."""
import pytest
import torch

import dcgan_reference as R

CRITIC = dict(input_image_shape=(16, 16, 3), block_sizes=(8, 16, 16), resamples=('SAME', 'DOWN', 'SAME'), number_of_classes=10,
              spectral=False, arch='dcgan')
GENERATOR = dict(arch='dcgan', block_norm='b', last_norm='b', block_after_norm='ucs', last_after_norm='ucs', first_block_shape=(4, 4, 16),
                 block_sizes=(16, 8), resamples=('UP', 'UP'))


def _rel(a, ref):
    return float((a.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max().clamp_min(1e-300))


def _loss(out, weights):
    outs = out if isinstance(out, tuple) else (out,)
    return sum((o * w.to(o.dtype)).sum() for o, w in zip(outs, weights))


def _jitter(module, names=('.bias', '.beta', '.gamma')):
    """biases and colorings off their initial 0 / 1: a term that is dropped somewhere would not show otherwise"""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith(names):
                p.add_(0.05 * torch.randn_like(p))


@pytest.mark.parametrize("head", [None, 'AC_GAN'])
def test_dc_critic_equals_the_float64_reference_on_the_cpu(head):
    from wc_gan_amd.discriminator import DCBlockDown, make_discriminator
    torch.manual_seed(3)
    kw = dict(CRITIC, type=head)
    D = make_discriminator(**kw).double()
    _jitter(D)
    assert all(isinstance(b, DCBlockDown) for b in D.blocks)
    assert [tuple(b.conv.conv.weight.shape) for b in D.blocks] == [(8, 3, 3, 3), (16, 8, 4, 4), (16, 16, 3, 3)]
    assert D.out.in_features == 8 * 8 * 16                          # the flatten tail: every point of the 8 x 8 grid
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(3, 16, 16, 3, generator=g, dtype=torch.float64) * 2 - 1).requires_grad_(True)
    weights = (torch.randn(3, 1, generator=g, dtype=torch.float64), torch.randn(3, 10, generator=g, dtype=torch.float64))
    out = D(x)
    names = [n for n, _ in D.named_parameters()]
    grads = dict(zip(['x'] + names, torch.autograd.grad(_loss(out, weights), [x] + list(D.parameters()))))

    params, buffers = R.leaves(D.state_dict())
    critic = R.Critic(params, buffers, iterations=0, **kw)
    x64 = x.detach().clone().requires_grad_(True)
    out64 = critic(x64)
    grads64 = dict(zip(['x'] + list(params), torch.autograd.grad(_loss(out64, weights), [x64] + list(params.values()))))
    assert len(critic.pre) == R.leaky_count(kw['block_sizes']) == 3
    assert isinstance(out, tuple) == (head == 'AC_GAN')
    for a, b in zip(out if isinstance(out, tuple) else (out,), out64 if isinstance(out64, tuple) else (out64,)):
        assert a.shape == b.shape and _rel(a, b) < 1e-12
    assert set(grads) == set(grads64)
    for n in grads:
        assert grads[n].shape == grads64[n].shape and _rel(grads[n], grads64[n]) < 1e-12, n
    # the reference's own signs, forced: nothing changes
    masks = [h > 0 for h in critic.pre]
    forced = R.Critic(params, buffers, iterations=0, masks=masks, **kw)
    outf = forced(x64)
    assert R.mask_disagreement(masks, forced.pre) == (0.0, 0)
    for a, b in zip(outf if isinstance(outf, tuple) else (outf,), out64 if isinstance(out64, tuple) else (out64,)):
        assert _rel(a, b) < 1e-14


def test_dc_generator_equals_the_float64_reference_and_norms_sit_on_the_block_inputs():
    from wc_gan_amd.generator import DCBlockUp, make_generator
    torch.manual_seed(4)
    G = make_generator(**GENERATOR).double()
    _jitter(G)
    G.train()
    assert all(isinstance(b, DCBlockUp) for b in G.blocks)
    seen = []
    sites = [b.bn for b in G.blocks] + [G.final_norm]
    hooks = [m.register_forward_hook(lambda _m, inp, _out: seen.append(tuple(inp[0].shape))) for m in sites]
    z = torch.randn(6, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y = G(z)
    for h in hooks:
        h.remove()
    # exactly len(blocks) + 1 norm sites, each on a block INPUT (the last one behind the last block): (N, H, W, C)
    assert seen == [(6, 4, 4, 16), (6, 8, 8, 16), (6, 16, 16, 8)]
    from wc_gan_amd.generator import _UnfusedStack
    norm_modules = [n for n, m in G.named_modules() if isinstance(m, _UnfusedStack)]
    assert norm_modules == ['blocks.0.bn', 'blocks.1.bn', 'final_norm']
    names = [n for n, _ in G.named_parameters()]
    w = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    grads = dict(zip(names, torch.autograd.grad((y * w).sum(), list(G.parameters()))))

    params, _ = R.leaves({k: v for k, v in G.state_dict().items() if k in names})
    ref = R.Generator(params, **GENERATOR)
    y64 = ref(z)
    assert ref.sites == seen
    grads64 = dict(zip(list(params), torch.autograd.grad((y64 * w).sum(), list(params.values()))))
    assert y.shape == y64.shape == (6, 16, 16, 3) and _rel(y, y64) < 1e-12
    assert set(grads) == set(grads64)
    for n in grads:
        assert grads[n].shape == grads64[n].shape
        if n.endswith('.deconv.bias'):
            # a bias straight in front of a batch normalisation: the mean subtraction removes it, its gradient is exactly zero and both
            # sides hold rounding residue only -- measured against the gradient of the same layer's weight instead of against itself
            scale = grads64[n.replace('.bias', '.weight')].abs().max()
            assert grads[n].abs().max() < 1e-12 * scale and grads64[n].abs().max() < 1e-12 * scale, n
        else:
            assert _rel(grads[n], grads64[n]) < 1e-12, n


def test_dcgan_configs_follow_the_recipes():
    from wc_gan_amd.train import CONFIGS, DCGAN_CONFIGS, dcgan_sites
    assert sorted(CONFIGS) == ['cifar10_cond', 'cifar10_uncond', 'stl10_uncond', 'tinyimagenet_cond_sa']
    assert sorted(DCGAN_CONFIGS) == ['cifar10_dcgan_uncond', 'stl10_dcgan_uncond']
    for name, w, image in (('cifar10_dcgan_uncond', 4, 32), ('stl10_dcgan_uncond', 6, 48)):
        cfg = DCGAN_CONFIGS[name]
        g, d = cfg['generator'], cfg['discriminator']
        assert g['arch'] == d['arch'] == 'dcgan'
        assert tuple(g['block_sizes']) == (512, 256, 128) and tuple(g['resamples']) == ('UP', 'UP', 'UP')
        assert tuple(g['first_block_shape']) == (w, w, 512)
        assert (g['block_norm'], g['block_after_norm'], g['last_norm'], g['last_after_norm']) == ('d', 'uconv', 'd', 'uconv')
        assert tuple(d['block_sizes']) == (64, 128, 128, 256, 256, 512, 512)
        assert tuple(d['resamples']) == ('SAME', 'DOWN', 'SAME', 'DOWN', 'SAME', 'DOWN', 'SAME')
        assert d['spectral'] is True and d['type'] is None and tuple(d['input_image_shape']) == (image, image, 3)
        assert cfg['training_ratio'] == 1 and cfg['generator_batch_multiple'] == 1 and cfg['conditional'] is False
        shapes = [s[1:] for s in dcgan_sites(cfg, 64)]
        assert shapes == [(64, w, w, 512), (64, 2 * w, 2 * w, 512), (64, 4 * w, 4 * w, 256), (64, 8 * w, 8 * w, 128)]
    assert [s[2:] for s in dcgan_sites(DCGAN_CONFIGS['cifar10_dcgan_uncond'], 8)] == [(4, 4, 512), (8, 8, 512), (16, 16, 256), (32, 32, 128)]
    assert [s[2:] for s in dcgan_sites(DCGAN_CONFIGS['stl10_dcgan_uncond'], 8)] == [(6, 6, 512), (12, 12, 512), (24, 24, 256), (48, 48, 128)]


def test_build_trainer_forwards_the_recipes_schedule():
    """training_ratio / generator_batch_multiple of a DCGAN configuration reach GanTrainer unless the caller overrides them (tiny widths,
    CPU: only the constructor runs)"""
    import copy
    from wc_gan_amd.train import DCGAN_CONFIGS, build_trainer
    cfg = copy.deepcopy(DCGAN_CONFIGS['cifar10_dcgan_uncond'])
    cfg['generator'].update(block_sizes=(16, 8, 8), first_block_shape=(4, 4, 16), block_norm='n', last_norm='n', block_after_norm='n',
                            last_after_norm='n')
    cfg['discriminator'].update(block_sizes=(8, 8, 8, 8, 8, 8, 8), spectral=False)
    t = build_trainer(cfg, device='cpu')
    assert (t.training_ratio, t.gbm) == (1, 1)
    t = build_trainer(cfg, device='cpu', training_ratio=3)
    assert (t.training_ratio, t.gbm) == (3, 1)


def test_projective_head_on_a_grid_is_refused():
    from wc_gan_amd.discriminator import make_discriminator
    with pytest.raises(ValueError, match="1 x 1"):
        make_discriminator(**dict(CRITIC, type='PROJECTIVE'))
    # on a 1 x 1 final grid the embedding and the flattened features have the same width
    D = make_discriminator(input_image_shape=(2, 2, 3), block_sizes=(8, 16), resamples=('SAME', 'DOWN'), number_of_classes=10,
                           type='PROJECTIVE', spectral=False, arch='dcgan').double()
    out = D(torch.randn(3, 2, 2, 3, dtype=torch.float64), torch.tensor([[1], [2], [3]], dtype=torch.int32))
    assert out.shape == (3, 1)
