"""The projection critic's tail (wc_gan_amd/tail.py: projection_tail; csrc/wc_tail.hip) without a GPU: the float64
restatement of tests/projection_reference.py against torch.autograd, tail.projection_tail's torch-op route against it, the critic's
`fused_projection` switch, what each mistake the GPU bounds must see moves, the entries' shape gate and argument checks (no launch), and the
three recipe tables."""
import copy

import pytest
import torch
import torch.nn.functional as F

import projection_reference as PRJ
from projection_reference import rel

NAMES = dict(y='dy', w_out='dw_out', b_out='db_out', emb='dE')


def _case(K=10, seed=0, N=5, H=4, W=5, C=8, bias=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cls = torch.randint(0, K, (N, 1), generator=g)
    cls[0], cls[-1] = 0, K - 1
    return dict(y=rn(N, H, W, C), w_out=rn(1, C), b_out=rn(1) if bias else None, emb=rn(K, C), g_out=rn(N, 1), cls=cls)


def _autograd(c, sum_pool):
    """F.linear(f, w) + (E[cls] * f).sum(1), differentiated by torch"""
    leaves = {k: c[k].clone().requires_grad_(True) for k in NAMES if c[k] is not None}
    f = F.relu(leaves['y'])
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, leaves['w_out'], leaves.get('b_out')) + (leaves['emb'][c['cls'].reshape(-1)] * f).sum(dim=1, keepdim=True)
    grads = dict(zip(leaves, torch.autograd.grad((out * c['g_out']).sum(), list(leaves.values()))))
    return dict(feat=f, out=out[:, 0]), grads


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_restatement_equals_autograd(sum_pool, bias):
    c = _case(seed=1 + bias, bias=bias)
    want, grads = _autograd(c, sum_pool)
    ref = PRJ.reference(c, sum_pool)
    for k in want:
        assert rel(ref[k], want[k]) < 1e-12, k
    for k, g in grads.items():
        assert rel(ref[NAMES[k]].reshape(g.shape), g) < 1e-12, k


def _tail_call(c, sum_pool):
    from wc_gan_amd import tail
    leaves = {k: c[k].clone().requires_grad_(True) for k in NAMES if c[k] is not None}
    out = tail.projection_tail(leaves['y'], leaves['w_out'], leaves.get('b_out'), leaves['emb'], c['cls'], sum_pool)
    assert tail.last_route == 'torch' and out.shape == (c['y'].shape[0], 1)
    grads = dict(zip(leaves, torch.autograd.grad((out * c['g_out']).sum(), list(leaves.values()))))
    return out[:, 0], grads


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_projection_tail_on_the_cpu_equals_the_restatement(sum_pool, bias):
    c = _case(seed=11 + bias, bias=bias)
    ref = PRJ.reference(c, sum_pool)
    out, grads = _tail_call(c, sum_pool)
    assert rel(out, ref['out']) < 1e-12
    for k, g in grads.items():
        assert rel(g, ref[NAMES[k]].reshape(g.shape)) < 1e-12, k


@pytest.mark.parametrize("bad", [10, -1])
def test_a_label_outside_the_classes_gives_nan_and_changes_nothing_else(bad):
    """out[n] is NaN; that sample's dy keeps the adversarial head's term alone, it reaches no row of dE, everything else is as it was"""
    c = _case(seed=4)
    good = PRJ.reference(c, True)
    cls = c['cls'].clone()
    cls[1] = bad
    cb = dict(c, cls=cls)
    ref = PRJ.reference(cb, True)
    keep = [0, 2, 3, 4]
    assert torch.isnan(ref['out'][1]) and torch.equal(ref['out'][keep], good['out'][keep])
    assert torch.equal(ref['dy'][keep], good['dy'][keep]) and torch.equal(ref['dw_out'], good['dw_out']) and torch.equal(ref['db_out'], good['db_out'])
    alone = (c['y'][1] > 0).double() * (c['g_out'][1] * c['w_out']).reshape(1, 1, -1)
    assert rel(ref['dy'][1], alone) < 1e-14
    k = int(c['cls'][1])
    others = [j for j in range(10) if j != k]
    assert torch.equal(ref['dE'][others], good['dE'][others])
    assert rel(good['dE'][k] - ref['dE'][k], c['g_out'][1] * good['feat'][1]) < 1e-12
    out, grads = _tail_call(cb, True)
    assert torch.isnan(out[1]) and rel(out[keep], ref['out'][keep]) < 1e-12
    for name, g in grads.items():
        assert torch.isfinite(g).all() and rel(g, ref[NAMES[name]].reshape(g.shape)) < 1e-12, name


def test_what_each_mistake_moves():
    """On the GPU rows' own inputs, in float64: each of these moves out, dy or dE by more than 1e-2 of its maximum, so a bound of 1e-4 or
    less sees it.  (A row with one class cannot read another row, and one with a single sample has nothing to sum dE over: those two
    mistakes are measured where they can be made.)"""
    for shape in PRJ.SHAPES:
        N, HW, C, K = shape
        for label, c, sum_pool in PRJ.rows(shape):
            if 'negative' in label and N == 1:
                continue                                # every output is the bias alone
            ref = PRJ.reference(c, sum_pool)
            if K > 1:                                   # reading row cls[n] + 1
                wrong = PRJ.reference(dict(c, cls=(c['cls'] + 1) % K), sum_pool)
                assert rel(wrong['out'], ref['out']) > 1e-2 and rel(wrong['dy'], ref['dy']) > 1e-2 and rel(wrong['dE'], ref['dE']) > 1e-2, (shape, label)
            # dropping E from dy
            s = 1.0 if sum_pool else 1.0 / HW
            no_e = (c['y'] > 0).double() * (s * c['g_out'].double()[:, None] * c['w_out'].double()[None]).reshape(N, 1, 1, C)
            assert rel(no_e, ref['dy']) > 1e-2, (shape, label)
            if N > 1 and len(set(c['cls'].tolist())) > 1:       # summing dE over all n
                every = (c['g_out'].double() @ ref['feat']).expand(K, C)
                assert rel(every, ref['dE']) > 1e-2, (shape, label)


# ---------------------------------------------------------------------------------------------------------------------------------
# the entries, without a launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib
    return _lib.load()


def test_the_shape_gate_at_its_edges(lib):
    ok = lib.wc_critic_proj_supported
    assert ok(1, 1, 4, 1) == 1 and ok(128, 64, 256, 100) == 1
    assert ok(1, 1, 1024, 1) == 1 and ok(1, 1, 1028, 1) == 0 and ok(1, 1, 6, 1) == 0 and ok(1, 1, 0, 1) == 0
    assert ok(1, 1, 4, 0) == 0 and ok(1, 1, 4, 1024) == 1 and ok(1, 1, 4, 1025) == 0 and ok(1, 1, 4, -1) == 0
    assert ok(0, 1, 4, 1) == 0 and ok(1, 0, 4, 1) == 0
    assert ok(2 ** 21, 1, 1024, 1) == 0 and ok(2 ** 21 - 1, 1, 1024, 1) == 1                # N HW C = 2^31 and just below
    assert ok(2 ** 20, 2 ** 9, 4, 1) == 0 and ok(2 ** 40, 2 ** 40, 4, 1) == 0
    assert lib.wc_critic_tail_supported(1, 1, 4, 0) == 1                                    # the existing gate keeps K = 0


def test_argument_errors_are_codes(lib):
    import ctypes
    buf = (ctypes.c_float * 80)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, as the entries ask of y, dy, w_out and the table
    fwd, bwd, wg = lib.wc_critic_proj_fwd_f32, lib.wc_critic_proj_bwd_f32, lib.wc_critic_proj_wgrad_f32
    NULL, SHAPE, ARG = -1, -2, -5
    for i in (0, 1, 3, 4, 10, 11):                  # y, w_out, the table, the labels, feat, out (b_out is optional)
        a = [p, p, p, p, p, 1, 1, 4, 2, 1, p, p, None]
        a[i] = None
        assert fwd(*a) == NULL, i
    assert fwd(p, p, None, p, p, 1, 1, 4, 2, 2, p, p, None) == ARG
    assert fwd(p, p, None, p, p, 1, 1, 4, 2, -1, p, p, None) == ARG
    assert fwd(p, p, None, p, p, 1, 1, 6, 2, 1, p, p, None) == SHAPE
    assert fwd(p, p, None, p, p, 1, 1, 4, 0, 1, p, p, None) == SHAPE                # no table: the other entries' case
    assert fwd(p, p, None, p, p, 0, 1, 4, 2, 1, p, p, None) == SHAPE
    assert fwd(p + 4, p, None, p, p, 1, 1, 4, 2, 1, p, p, None) == ARG              # y is read 16 bytes at a time
    assert fwd(p, p + 8, None, p, p, 1, 1, 4, 2, 1, p, p, None) == ARG
    assert fwd(p, p, None, p + 4, p, 1, 1, 4, 2, 1, p, p, None) == ARG
    for i in (0, 1, 2, 3, 4, 10):                   # y, w_out, the table, the labels, g_out, dy
        a = [p, p, p, p, p, 1, 1, 4, 2, 1, p, None]
        a[i] = None
        assert bwd(*a) == NULL, i
    assert bwd(p, p, p, p, p, 1, 1, 4, 2, 3, p, None) == ARG
    assert bwd(p, p, p, p, p, 1, 1, 1028, 2, 1, p, None) == SHAPE
    assert bwd(p, p, p, p, p, 1, 1, 4, 1025, 1, p, None) == SHAPE
    assert bwd(p + 4, p, p, p, p, 1, 1, 4, 2, 1, p, None) == ARG
    assert bwd(p, p, p, p, p, 1, 1, 4, 2, 1, p + 8, None) == ARG                    # dy is written 16 bytes at a time
    assert bwd(p, p + 4, p, p, p, 1, 1, 4, 2, 1, p, None) == ARG
    assert bwd(p, p, p + 12, p, p, 1, 1, 4, 2, 1, p, None) == ARG
    for i in (0, 1, 2, 6, 7, 8):                    # feat, g_out, the labels, dw_out, db_out, demb
        a = [p, p, p, 1, 4, 2, p, p, p, None]
        a[i] = None
        assert wg(*a) == NULL, i
    assert wg(p, p, p, 1, 4, 0, p, p, p, None) == SHAPE
    assert wg(p, p, p, 1, 4, 1025, p, p, p, None) == SHAPE
    assert wg(p, p, p, 0, 4, 2, p, p, p, None) == SHAPE


# ---------------------------------------------------------------------------------------------------------------------------------
# the critic
# ---------------------------------------------------------------------------------------------------------------------------------
CRITIC = dict(input_image_shape=(16, 16, 3), block_sizes=(8, 16), resamples=('DOWN', 'SAME'), number_of_classes=7, spectral=False)


def _critic(seed=3, **kw):
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(seed)
    D = make_discriminator(**dict(CRITIC, **kw)).double()
    with torch.no_grad():
        for name, p in D.named_parameters():
            p.add_((0.1 if name.endswith('.bias') else 0.02) * torch.randn_like(p))
    return D


@pytest.mark.parametrize("sum_pool", [True, False])
def test_the_flag_changes_the_route_not_the_map(sum_pool):
    from wc_gan_amd import tail
    plain = _critic(type='PROJECTIVE', sum_pool=sum_pool)
    fused = _critic(type='PROJECTIVE', sum_pool=sum_pool, fused_projection=True)
    assert plain.fused_projection is False and fused.fused_projection is True and fused._projection_is_fused()
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), fused.state_dict().values()))
    g = torch.Generator().manual_seed(2)
    x = torch.rand(4, 16, 16, 3, generator=g, dtype=torch.float64) * 2 - 1
    cls = torch.tensor([[0], [6], [3], [6]], dtype=torch.int32)
    weights = torch.randn(4, 1, generator=g, dtype=torch.float64)
    tail.last_route = None
    a = plain(x, cls)
    assert tail.last_route is None
    b = fused(x, cls)
    assert tail.last_route == 'torch'
    assert a.shape == b.shape == (4, 1) and rel(b, a) < 1e-12
    ga = torch.autograd.grad((a * weights).sum(), list(plain.parameters()))
    gb = torch.autograd.grad((b * weights).sum(), list(fused.parameters()))
    assert 'emb.weight' in dict(plain.named_parameters())
    for (n, _), s, t in zip(plain.named_parameters(), ga, gb):
        assert float(s.abs().max()) > 0 and rel(t, s) < 1e-12, n


def test_which_critics_take_the_projection_route():
    from wc_gan_amd.discriminator import make_discriminator
    make = lambda **kw: make_discriminator(**dict(CRITIC, **kw))
    assert make(type='PROJECTIVE', fused_projection=True)._projection_is_fused()
    assert not make(type=None, fused_projection=True)._projection_is_fused()
    assert not make(type='AC_GAN', fused_projection=True)._projection_is_fused()
    assert not make(type='PROJECTIVE', dropout=0.2, fused_projection=True)._projection_is_fused()
    assert not make(type='PROJECTIVE', arch='dcgan', input_image_shape=(2, 2, 3), resamples=('SAME', 'DOWN'), fused_projection=True)._projection_is_fused()
    assert not make(type='PROJECTIVE')._projection_is_fused()
    assert not make(type='PROJECTIVE', fused_tail=True)._projection_is_fused()
    for kw in (dict(fused_tail=True), dict(fused_projection=True), dict(fused_tail=True, fused_projection=True)):
        assert not make(type='PROJECTIVE', **kw)._tail_is_fused()
    assert make(type=None, fused_tail=True, fused_projection=True)._tail_is_fused()        # the other switch is left alone


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_three_recipes_hold_what_their_scripts_say():
    from wc_gan_amd.train import FUSED_PROJECTION_SHIPS, PROJECTION_CONFIGS, PROJECTION_SCHEDULES
    assert set(PROJECTION_CONFIGS) == set(PROJECTION_SCHEDULES) == {'cifar10_cond_sa', 'cifar100_cond', 'cifar100_cond_sa'}
    for name, after_norm, filters_emb, classes in (('cifar10_cond_sa', 'ufconv', 4, 10), ('cifar100_cond', 'ucconv', None, 100),
                                                   ('cifar100_cond_sa', 'ufconv', 10, 100)):
        cfg = PROJECTION_CONFIGS[name]
        assert cfg['conditional'] is True and cfg['image_shape'] == (32, 32, 3)
        assert not {'objective', 'gan_type', 'gradient_penalty_weight', 'training_ratio'} & set(cfg)       # the hinge defaults
        g, d = cfg['generator'], cfg['discriminator']
        assert g['block_sizes'] == (128,) * 3 and g['resamples'] == ("UP",) * 3 and g['first_block_shape'] == (4, 4, 128)
        assert (g['block_norm'], g['block_after_norm'], g['last_norm'], g['last_after_norm']) == ('d', after_norm, 'd', 'uconv')
        assert g['gan_type'] == 'PROJECTIVE' and g['number_of_classes'] == d['number_of_classes'] == classes
        assert d['input_image_shape'] == (32, 32, 3) and d['block_sizes'] == (256,) * 4 and d['resamples'] == ('DOWN', 'DOWN', 'SAME', 'SAME')
        assert (d['type'], d['spectral'], d['sum_pool'], d['conv_singular']) == ('PROJECTIVE', True, True, False)
        assert d['fused_projection'] is FUSED_PROJECTION_SHIPS and 'fused_tail' not in d
        if filters_emb is None:
            assert 'filters_emb' not in g and 'filters_emb' not in d                # the script leaves run.py's default
        else:
            assert g['filters_emb'] == d['filters_emb'] == filters_emb
        assert PROJECTION_SCHEDULES[name] == dict(lr_decay_schedule='linear', number_of_epochs=50)


def test_the_existing_tables_keep_their_keys_and_the_copy_leaves_them_alone():
    from wc_gan_amd import train
    assert set(train.CONFIGS) == {'cifar10_uncond', 'cifar10_cond', 'stl10_uncond', 'tinyimagenet_cond_sa'}
    assert set(train.DCGAN_CONFIGS) == {'cifar10_dcgan_uncond', 'stl10_dcgan_uncond'}
    assert set(train.WGAN_CONFIGS) == {'cifar10_wgan_uncond'}
    assert set(train.ACGAN_CONFIGS) == {'cifar10_wgan_cond', 'cifar10_wgan_cond_sa'}
    assert set(train.RECIPE_SCHEDULES) == set(train.CONFIGS) | set(train.DCGAN_CONFIGS) | set(train.WGAN_CONFIGS)
    tables = (train.CONFIGS, train.DCGAN_CONFIGS, train.WGAN_CONFIGS, train.ACGAN_CONFIGS)
    assert all('fused_projection' not in c['discriminator'] for t in tables for c in t.values())
    for table in tables + (train.PROJECTION_CONFIGS,):
        for cfg in table.values():
            before = copy.deepcopy(cfg)
            on = train.fused_projection_config(cfg)
            assert cfg == before and on['discriminator']['fused_projection'] is True
            on['discriminator'].pop('fused_projection')
            before['discriminator'].pop('fused_projection', None)
            assert on == before


def test_build_trainer_on_a_projection_recipe():
    from wc_gan_amd.train import PROJECTION_CONFIGS, build_trainer, fused_projection_config
    cfg = fused_projection_config(PROJECTION_CONFIGS['cifar100_cond_sa'])
    cfg['generator'].update(block_sizes=(8,), resamples=("UP",), first_block_shape=(4, 4, 8), block_norm='b', last_norm='b',
                            block_after_norm='ucs', last_after_norm='ucs')
    cfg['discriminator'].update(input_image_shape=(8, 8, 3), block_sizes=(8, 8), resamples=('DOWN', 'SAME'))
    t = build_trainer(cfg, device='cpu')
    assert (t.conditional, t.objective, t.gan_type, t.gp_weight) == (True, 'hinge', None, 0.0)
    assert t.D.type == 'PROJECTIVE' and t.D.fused_projection is True and t.D._projection_is_fused() and t.D.emb.weight.shape == (100, 8)
