"""tests/generator_reference.py pinned on the CPU (default suite) before the HIP generator is held to it (tests/test_generator_gpu.py):

* a reference WC site against oracle.wc_forward / wc_backward at 1e-10 of each tensor's maximum -- alone (uconv) and with class tables
  (ucconv, ufconv), training and evaluation mode, two statistic groups, the moving-statistics update -- and its tables against
  oracle.coloring_table;
* everything that is not a site (concat_cls embedding, dense, upsample + convolution, shortcut, add, tanh) against torch.nn.functional
  run directly at 1e-12;
* forcing the reference's own signs changes nothing (1e-14);
* SENSITIVITY: a reference built with one deliberate change (ddof 0, a shortcut bias dropped, Gamma transposed, one forced mask element
  flipped far from zero) moves the named tensors by more than 1e-4 under generator_reference.errors, the GPU tests' comparison;
* the route decisions of the GPU tests' batches equal the recipes' own, from the library's host predicates;
* CONDITION: on the GPU tests' own cases the reference in fp32 picks signs that differ from the float64 signs in at most 1e-4 of a
  site's elements, each within 1e-4 of zero -- the caps the GPU tests put on the HIP network's signs hold with room for rounding.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import generator_reference as R
import test_generator_gpu as TG
from oracle import wc_oracle as O

SMALL = dict(block_sizes=(32, 32), resamples=('UP', 'UP'), first_block_shape=(4, 4, 32), number_of_classes=5, block_norm='d',
             block_after_norm='ucconv', last_norm='d', last_after_norm='uconv', gan_type='PROJECTIVE')


def _rel(a, ref):
    a = torch.as_tensor(np.asarray(a.detach() if torch.is_tensor(a) else a), dtype=torch.float64)
    ref = torch.as_tensor(np.asarray(ref.detach() if torch.is_tensor(ref) else ref), dtype=torch.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------------------
# a site against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _site_params(after_norm, C, K, E, rng):
    """state-dict tensors of one site 's' and the oracle's `params` of the same coloring"""
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    o = dict(u_kernel=rng.standard_normal((C, C)) / np.sqrt(C), u_bias=0.1 * rng.standard_normal(C),
             c_kernel=rng.standard_normal((K, C, C)) / np.sqrt(C), c_bias=0.1 * rng.standard_normal((K, C)),
             f_kernel=rng.standard_normal((E, C, C)) / np.sqrt(C), f_alpha=rng.standard_normal((K, E)))
    state = {'s.npart.moving_mean': t(0.1 * rng.standard_normal((C, 1)))}
    a = rng.standard_normal((C, 2 * C))
    state['s.npart.moving_cov'] = t(a @ a.T / (2 * C))
    kinds = R.BRANCHES[after_norm]
    u = kinds.index('u')
    state[f's.branches.{u}.kernel'], state[f's.branches.{u}.bias'] = t(o['u_kernel']).view(1, 1, C, C), t(o['u_bias'])
    if 'c' in kinds:
        state['s.branches.0.kernel'], state['s.branches.0.bias'] = t(o['c_kernel']), t(o['c_bias'])
    if 'f' in kinds:
        state['s.branches.0.kernel'], state['s.branches.0.class_matrix'] = t(o['f_kernel']), t(o['f_alpha'])
    return state, o


def _branch_gradients(after_norm, o, dG, dB):
    """the oracle's table gradients (dG (K, C, C), dB (K, C)) taken to the branches' own weights"""
    kinds = R.BRANCHES[after_norm]
    u = kinds.index('u')
    C = dG.shape[-1]
    out = {f's.branches.{u}.kernel': dG.sum(0).reshape(1, 1, C, C), f's.branches.{u}.bias': dB.sum(0)}
    if 'c' in kinds:
        out['s.branches.0.kernel'], out['s.branches.0.bias'] = dG, dB
    if 'f' in kinds:
        out['s.branches.0.kernel'] = np.einsum('ke,kio->eio', o['f_alpha'], dG)
        out['s.branches.0.class_matrix'] = np.einsum('kio,eio->ke', dG, o['f_kernel'])
    return out


@pytest.mark.parametrize("after_norm", ['uconv', 'ucconv', 'ufconv'])
@pytest.mark.parametrize("training", [True, False])
def test_reference_site_equals_the_oracle(after_norm, training):
    rng = np.random.default_rng(3)
    N, H, W, C, K, E = 12, 5, 3, 16, 4, 3
    state, o = _site_params(after_norm, C, K, E, rng)
    x = O.synth_activation(rng, (N, H, W, C), 'well') + 0.3
    gy = rng.standard_normal((N, H, W, C))
    cls = rng.integers(0, K, (N, 1))
    # the tables, one per class
    params, buffers = R.leaves(state)
    ref = R.Generator(params, buffers, training=training, block_after_norm=after_norm, last_after_norm=after_norm)
    G_ref, B_ref = O.coloring_table(after_norm, C, o, K)
    gamma, beta = ref.tables('s', after_norm, torch.arange(K).view(K, 1), K)
    assert _rel(gamma.expand(K, C, C) if gamma.dim() == 3 else gamma.expand(G_ref.shape[0], C, C), G_ref) < 1e-14
    assert _rel(beta.expand(G_ref.shape[0], C), B_ref) < 1e-14
    # the site: y, dx and the gradient of every branch weight; the moving statistics
    idx = cls.reshape(-1) if after_norm != 'uconv' else None
    y_ref, cache = O.wc_forward(x, G_ref, B_ref, idx, training=training, moving_mean=state['s.npart.moving_mean'].numpy(),
                                moving_cov=state['s.npart.moving_cov'].numpy(), eps=1e-3, momentum=0.99, ddof=1)
    dx_ref, dG_ref, dB_ref = O.wc_backward(gy, cache)
    xt = torch.tensor(x, requires_grad=True)
    y = ref.site('s', after_norm, xt, torch.tensor(cls))
    names = list(params)
    grads = torch.autograd.grad((y * torch.tensor(gy)).sum(), [xt] + [params[n] for n in names])
    assert _rel(y, y_ref) < 1e-10 and _rel(grads[0], dx_ref) < 1e-10
    want = _branch_gradients(after_norm, o, dG_ref, dB_ref)
    assert set(want) == set(names)
    for n, g in zip(names, grads[1:]):
        assert _rel(g, want[n]) < 1e-10, n
    if training:
        mm, mc = ref.moving['s']
        assert mm.shape == (C, 1) and _rel(mm.view(-1), cache['moving_mean']) < 1e-10 and _rel(mc, cache['moving_cov']) < 1e-10
    else:
        assert ref.moving == {}


def test_reference_site_with_statistic_groups_equals_the_oracle_group_by_group():
    rng = np.random.default_rng(4)
    N, H, W, C, K, E = 12, 4, 4, 16, 4, 3
    state, o = _site_params('ucconv', C, K, E, rng)
    x = O.synth_activation(rng, (N, H, W, C), 'well') + 0.3
    cls = rng.integers(0, K, (N, 1))
    params, buffers = R.leaves(state)
    ref = R.Generator(params, buffers, groups=3, block_after_norm='ucconv')
    with torch.no_grad():
        y = ref.site('s', 'ucconv', torch.tensor(x), torch.tensor(cls))
    G_ref, B_ref = O.coloring_table('ucconv', C, o, K)
    mm, mc = state['s.npart.moving_mean'].numpy(), state['s.npart.moving_cov'].numpy()
    for g in range(3):          # three calls, one after the other: each on its own statistics, the moving statistics handed on
        rows = slice(4 * g, 4 * g + 4)
        y_ref, cache = O.wc_forward(x[rows], G_ref, B_ref, cls[rows].reshape(-1), moving_mean=mm, moving_cov=mc)
        mm, mc = cache['moving_mean'], cache['moving_cov']
        assert _rel(y[rows], y_ref) < 1e-10
    assert _rel(ref.moving['s'][0].view(-1), mm) < 1e-10 and _rel(ref.moving['s'][1], mc) < 1e-10


# ---------------------------------------------------------------------------------------------------------------------------------
# everything that is not a site against torch.nn.functional
# ---------------------------------------------------------------------------------------------------------------------------------
class _NoSites(R.Generator):
    def site(self, prefix, after_norm, x, cls):
        return x


def _small_state(kw, seed=2, concat_cls=False):
    """a float64 state dict of a small generator with every bias and coloring off its initial value"""
    from wc_gan_amd.generator import make_generator
    torch.manual_seed(seed)
    G = make_generator(concat_cls=concat_cls, **kw).double()
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith(('.bias', '.kernel')):
                p.add_(0.05 * torch.randn_like(p))
    return {k: v.detach().clone() for k, v in G.state_dict().items()}


@pytest.mark.parametrize("concat_cls", [False, True])
def test_reference_outside_the_sites_equals_torch_functional(concat_cls):
    kw = dict(SMALL, resamples=('UP', 'SAME'))
    state = _small_state(kw, concat_cls=concat_cls)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(3, 128, generator=g, dtype=torch.float64)
    cls = torch.randint(0, 5, (3, 1), generator=g)
    w = torch.randn(3, 8, 8, 3, generator=g, dtype=torch.float64)

    params, buffers = R.leaves(state)
    ref = _NoSites(params, buffers, concat_cls=concat_cls, **kw)
    img = ref(z, cls)
    grads = dict(zip(params, torch.autograd.grad((img * w).sum(), list(params.values()), allow_unused=True)))

    p2, _ = R.leaves(state)
    conv = lambda name, t: F.conv2d(t, p2[name + '.conv.weight'], p2[name + '.conv.bias'], padding=p2[name + '.conv.weight'].shape[2] // 2)
    y = torch.cat([F.embedding(cls.view(-1), p2['emb.weight']), z], dim=-1) if concat_cls else z
    y = F.linear(y, p2['dense.weight'], p2['dense.bias']).view(-1, 4, 4, 32).permute(0, 3, 1, 2)
    for i, rs in enumerate(kw['resamples']):
        up = (lambda t: F.interpolate(t, scale_factor=2, mode='nearest')) if rs == 'UP' else (lambda t: t)
        h = conv(f'blocks.{i}.conv1', up(F.relu(y)))
        h = conv(f'blocks.{i}.conv2', F.relu(h))
        y = h + conv(f'blocks.{i}.shortcut', up(y))
    img2 = torch.tanh(conv('final_conv', F.relu(y))).permute(0, 2, 3, 1)
    grads2 = dict(zip(p2, torch.autograd.grad((img2 * w).sum(), list(p2.values()), allow_unused=True)))
    assert img.shape == (3, 8, 8, 3) and _rel(img, img2) < 1e-12
    assert len(ref.pre) == R.relu_count(kw['block_sizes']) == 5
    used = [n for n in params if grads2[n] is not None]
    assert set(used) == set(n for n in params if '.branches.' not in n) and ('emb.weight' in used) == concat_cls
    for n in used:
        assert _rel(grads[n], grads2[n]) < 1e-12, n
    # the pieces on their own, odd sizes
    x = torch.randn(2, 5, 3, 6, generator=g, dtype=torch.float64)
    assert torch.equal(R.upsample2x(x), F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1))
    for k in (1, 3):
        wt, b = torch.randn(4, 6, k, k, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
        assert _rel(R.conv2d(x, wt, b), F.conv2d(x.permute(0, 3, 1, 2), wt, b, padding=k // 2).permute(0, 2, 3, 1)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# forced masks and sensitivity
# ---------------------------------------------------------------------------------------------------------------------------------
def _small_case(seed=5, batch=16):
    state = _small_state(SMALL)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(batch, 128, generator=g, dtype=torch.float64)
    cls = torch.randint(0, 5, (batch, 1), generator=g)
    w = torch.randn(batch, 16, 16, 3, generator=g, dtype=torch.float64)
    return state, z, cls, w


@pytest.fixture(scope='module')
def small():
    """the unchanged reference of the small case, computed once: (state, z, cls, w, ref, image, gradients, its own signs)"""
    state, z, cls, w = _small_case()
    ref, img, grads = R.run(state, SMALL, z, cls, w)
    return state, z, cls, w, ref, img, grads, [(h > 0) for h in ref.pre]


def _errors_of(changed, small):
    ref, img, grads = small[4:7]
    c_ref, c_img, c_grads = changed
    return R.errors(c_img, c_grads, c_ref.moving if c_ref.moving else None, ref, img, grads)


def test_forcing_the_references_own_signs_changes_nothing(small):
    state, z, cls, w, ref, img, grads, masks = small
    assert len(masks) == R.relu_count(SMALL['block_sizes']) == 5 and ref.sites[0] == 'blocks.0.bn1' and ref.sites[-1] == 'final_norm'
    forced = R.run(state, SMALL, z, cls, w, masks)
    assert R.mask_disagreement(masks, forced[0].pre) == (0.0, 0)
    assert all(v < 1e-14 for v in _errors_of(forced, small).values())
    # every block bias is a zero gradient of this training-mode network: what `errors` measures against the weight's gradient
    for n, g in grads.items():
        if R.zero_in_exact_arithmetic(n):
            assert float(g.abs().max()) < 1e-12 * float(grads[n.replace('.bias', '.weight')].abs().max()), n


def test_ddof_0_in_place_of_1_is_seen(small):
    state, z, cls, w = small[:4]
    errs = _errors_of(R.run(state, SMALL, z, cls, w, small[7], ddof=0), small)
    assert errs['moving'] > 1e-4
    assert errs['image'] > 1e-4


def test_a_dropped_shortcut_bias_is_seen(small):
    """in training mode the site behind the block removes the constant from the image -- the moving mean keeps it; in evaluation mode the
    image shows it"""
    state, z, cls, w = small[:4]
    dropped = dict(state)
    dropped['blocks.1.shortcut.conv.bias'] = torch.zeros_like(state['blocks.1.shortcut.conv.bias'])
    errs = _errors_of(R.run(dropped, SMALL, z, cls, w, small[7]), small)
    assert errs['moving'] > 1e-4
    ref, img, _ = R.run(state, SMALL, z, cls, None, training=False)
    masks = [h > 0 for h in ref.pre]
    changed = R.run(dropped, SMALL, z, cls, None, masks, training=False)
    assert R.errors(changed[1], None, None, ref, img, None)['image'] > 1e-4


def test_a_transposed_gamma_is_seen(small):
    state, z, cls, w = small[:4]
    for name in ('blocks.0.bn2.branches.1.kernel', 'blocks.1.bn1.branches.0.kernel', 'final_norm.branches.0.kernel'):
        swapped = dict(state)
        swapped[name] = state[name].transpose(-1, -2).contiguous()
        changed = R.run(swapped, SMALL, z, cls, w, small[7])
        changed[2][name] = changed[2][name].transpose(-1, -2)          # (the gradient back in the unchanged layout)
        errs = _errors_of(changed, small)
        assert errs['image'] > 1e-4, name
        assert errs['gamma'] > 1e-4, name


def test_a_forced_mask_element_flipped_far_from_zero_is_seen(small):
    state, z, cls, w, ref = small[:5]
    masks = [m.clone() for m in small[7]]
    at = int(ref.pre[2].abs().argmax())
    masks[2].view(-1)[at] = not bool(masks[2].view(-1)[at])
    changed = R.run(state, SMALL, z, cls, w, masks)
    band, share = R.site_disagreement(masks, changed[0].pre)[2]
    assert band == 1.0 and share >= 1.0 / masks[2].numel()
    worst, count = R.mask_disagreement(masks, changed[0].pre)
    assert worst == 1.0 and count >= 1
    errs = _errors_of(changed, small)
    assert errs['image'] > 1e-4
    assert errs['conv_w'] > 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU tests' cases: routes and conditioning
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", list(TG.CASES))
def test_the_gpu_cases_take_the_recipes_routes(recipe):
    """host predicates only: at the case's batch every route decision of a training-mode and of an evaluation-mode pass equals the one at
    the recipe's generator-update batch; the first site has at least 4 C rows"""
    G = TG._module(recipe, 'cpu')
    routes = TG._assert_recipe_routes(G, recipe)
    kw = TG._kw(recipe)
    H, W, C = kw['first_block_shape']
    assert TG.CASES[recipe] * H * W >= 4 * C
    assert len([w for w, _ in routes if w.endswith('bn1') or w.endswith('bn2') or w == 'final_norm']) == R.relu_count(kw['block_sizes'])
    if recipe == 'tinyimagenet_cond_sa':
        assert all(d['per_sample'] for w, d in routes if w.endswith(('.bn1', '.bn2')))


@pytest.mark.parametrize("recipe", list(TG.CASES))
def test_fp32_signs_of_the_gpu_cases_stay_within_the_caps(recipe):
    """the reference in fp32 on the case the GPU test runs (first training call), its signs forced on the float64 reference.  Measured:
    shares <= 9.5e-7, bands <= 8.4e-7 -- two orders of room under both caps.  (STL-10 at half its batch: 128 x 48 x 48 x 256 in float64
    takes eight CPU cores 30 s, the first 64 of the same samples 15 s; its first site then still has 2304 rows >= 4 C.)"""
    G = TG._module(recipe, 'cpu')
    kw = dict(TG._kw(recipe), **TG._site_kw(G))
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    z, cls, _ = TG._inputs(recipe, TG.CASES[recipe], 'cpu', 21)
    if recipe == 'stl10_uncond':
        z = z[:64]
    r32, _, _ = R.run(state, kw, z, cls, None, dtype=torch.float32)
    masks = [h > 0 for h in r32.pre]
    ref, _, _ = R.run(state, kw, z, cls, None, masks)
    per_site = R.site_disagreement(masks, ref.pre)
    print(recipe, [(f"{b:.1e}", f"{s:.1e}") for b, s in per_site])
    assert len(per_site) == R.relu_count(kw['block_sizes'])
    for prefix, (band, share) in zip(ref.sites, per_site):
        assert band <= TG.MASK_BAND and share <= TG.MASK_SHARE, (prefix, band, share)
