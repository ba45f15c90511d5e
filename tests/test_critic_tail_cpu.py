"""The critic's tail (wc_gan_amd/tail.py, csrc/wc_tail.hip) and the AC-GAN trainer without a GPU: the float64 restatement of
tests/tail_reference.py against torch.autograd, tail.critic_tail's torch-op route against it, what each mistake the GPU bounds must see
moves, the entries' shape gate and argument checks (no launch), the two new recipe tables, and GanTrainer(gan_type='AC_GAN') against a
hand-written float64 step."""
import copy

import pytest
import torch
import torch.nn.functional as F

import tail_reference as TR


def _case(K, seed=0, N=3, H=4, W=5, C=8):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = dict(y=rn(N, H, W, C), w_out=rn(1, C), b_out=rn(1), g_out=rn(N, 1))
    if K:
        c.update(w_cls=rn(K, C), b_cls=rn(K), g_logits=rn(N, K), g_ce=rn(N), labels=torch.randint(0, K, (N,), generator=g))
        c['labels'][0], c['labels'][-1] = 0, K - 1
    return c


def _autograd(c, sum_pool, K):
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('y', 'w_out', 'b_out') + (('w_cls', 'b_cls') if K else ())}
    f = F.relu(leaves['y'])
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, leaves['w_out'], leaves['b_out'])
    total = (out * c['g_out']).sum()
    r = dict(feat=f, out=out[:, 0])
    if K:
        logits = F.linear(f, leaves['w_cls'], leaves['b_cls'])
        ce = F.cross_entropy(logits, c['labels'], reduction='none')
        total = total + (logits * c['g_logits']).sum() + (ce * c['g_ce']).sum()
        r.update(logits=logits, ce=ce)
    grads = dict(zip(leaves, torch.autograd.grad(total, list(leaves.values()))))
    return r, grads


def _reference(c, sum_pool, K, **over):
    c = dict(c, **over)
    fwd = TR.forward(c['y'], c['w_out'], c['b_out'], c.get('w_cls'), c.get('b_cls'), c.get('labels'), sum_pool)
    bwd = TR.backward(c['y'], c['w_out'], c.get('w_cls'), fwd, c['g_out'], c.get('g_logits'), c.get('g_ce'), c.get('labels'), sum_pool)
    return fwd, bwd


NAMES = dict(y='dy', w_out='dw_out', b_out='db_out', w_cls='dW_cls', b_cls='db_cls')


@pytest.mark.parametrize("K", [0, 1, 10])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_restatement_equals_autograd(K, sum_pool):
    c = _case(K, seed=K)
    want, grads = _autograd(c, sum_pool, K)
    fwd, bwd = _reference(c, sum_pool, K)
    for k in want:
        assert TR.rel(fwd[k], want[k]) < 1e-12, k
    for k, g in grads.items():
        assert TR.rel(bwd[NAMES[k]].reshape(g.shape), g) < 1e-12, k


@pytest.mark.parametrize("K", [0, 1, 10])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_critic_tail_on_the_cpu_equals_it(K, sum_pool):
    from wc_gan_amd import tail
    c = _case(K, seed=10 + K)
    want, grads = _autograd(c, sum_pool, K)
    leaves = {k: c[k].clone().requires_grad_(True) for k in grads}
    out, logits, ce = tail.critic_tail(leaves['y'], leaves['w_out'], leaves['b_out'], leaves.get('w_cls'), leaves.get('b_cls'), c.get('labels'),
                                       sum_pool)
    assert tail.last_route == 'torch' and out.shape == (3, 1)
    assert TR.rel(out[:, 0], want['out']) < 1e-12
    total = (out * c['g_out']).sum()
    if K:
        assert TR.rel(logits, want['logits']) < 1e-12 and TR.rel(ce, want['ce']) < 1e-12
        total = total + (logits * c['g_logits']).sum() + (ce * c['g_ce']).sum()
    else:
        assert logits is None and ce is None
    for (k, g), got in zip(grads.items(), torch.autograd.grad(total, list(leaves.values()))):
        assert TR.rel(got, g) < 1e-12, k
    if K:       # without labels: no cross entropy
        assert tail.critic_tail(c['y'], c['w_out'], c['b_out'], c['w_cls'], c['b_cls'], None, sum_pool)[2] is None
    else:
        with pytest.raises(ValueError, match="class head"):
            tail.critic_tail(c['y'], c['w_out'], c['b_out'], None, None, torch.zeros(3, dtype=torch.long), sum_pool)


def test_a_label_outside_the_classes_gives_nan_and_no_class_gradient():
    from wc_gan_amd import tail
    c = _case(10, seed=4)
    labels = c['labels'].clone()
    labels[1] = 10
    fwd, bwd = _reference(c, True, 10, labels=labels)
    ok, bwd_ok = _reference(c, True, 10)
    assert torch.isnan(fwd['ce'][1]) and torch.equal(fwd['ce'][[0, 2]], ok['ce'][[0, 2]])
    assert torch.equal(bwd['dlogits'][1], c['g_logits'][1]) and torch.equal(bwd['dlogits'][[0, 2]], bwd_ok['dlogits'][[0, 2]])
    y = c['y'].clone().requires_grad_(True)
    _out, _logits, ce = tail.critic_tail(y, c['w_out'], c['b_out'], c['w_cls'], c['b_cls'], labels, True)
    assert torch.isnan(ce[1]) and TR.rel(ce[[0, 2]], ok['ce'][[0, 2]]) < 1e-12
    dy, = torch.autograd.grad((ce * c['g_ce']).sum(), y)
    only_ce = TR.backward(c['y'], c['w_out'], c['w_cls'], fwd, torch.zeros(3), None, c['g_ce'], labels, True)
    assert not dy[1].any() and TR.rel(dy, only_ce['dy']) < 1e-12


def test_what_each_mistake_moves():
    """each of these moves some output by more than 1e-2 of its maximum: a bound of 1e-4 or less on the GPU sees all of them"""
    K = 10
    c = _case(K, seed=7, N=4, H=8, W=8, C=16)
    for sum_pool in (True, False):
        fwd, bwd = _reference(c, sum_pool, K)
        moved = lambda a, b, k: TR.rel(a[k], b[k])
        # a wrong pooling scale: the other pooling's
        f2, b2 = _reference(c, not sum_pool, K)
        assert moved(f2, fwd, 'feat') > 1e-2 and moved(b2, bwd, 'dy') > 1e-2
        # a label shifted by one
        f2, b2 = _reference(c, sum_pool, K, labels=(c['labels'] + 1) % K)
        assert moved(f2, fwd, 'ce') > 1e-2 and moved(b2, bwd, 'dlogits') > 1e-2 and moved(b2, bwd, 'dy') > 1e-2
        # a dropped mask: dy without the y > 0 factor
        s = 1.0 if sum_pool else 1.0 / 64
        coef = c['g_out'] * c['w_out'] + bwd['dlogits'] @ c['w_cls']
        unmasked = (s * coef).reshape(4, 1, 1, 16).expand(4, 8, 8, 16)
        assert TR.rel(unmasked, bwd['dy']) > 1e-2
        # g_logits ignored
        b2 = TR.backward(c['y'], c['w_out'], c['w_cls'], fwd, c['g_out'], None, c['g_ce'], c['labels'], sum_pool)
        assert moved(b2, bwd, 'dlogits') > 1e-2 and moved(b2, bwd, 'dy') > 1e-2 and moved(b2, bwd, 'dW_cls') > 1e-2


# ---------------------------------------------------------------------------------------------------------------------------------
# the entries, without a launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib
    return _lib.load()


def test_the_shape_gate_at_its_edges(lib):
    ok = lib.wc_critic_tail_supported
    assert ok(1, 1, 4, 0) == 1 and ok(128, 64, 128, 10) == 1
    assert ok(1, 1, 1024, 0) == 1 and ok(1, 1, 1028, 0) == 0 and ok(1, 1, 6, 0) == 0 and ok(1, 1, 0, 0) == 0
    assert ok(1, 1, 4, 1024) == 1 and ok(1, 1, 4, 1025) == 0 and ok(1, 1, 4, -1) == 0
    assert ok(0, 1, 4, 0) == 0 and ok(1, 0, 4, 0) == 0
    assert ok(2 ** 21, 1, 1024, 0) == 0 and ok(2 ** 21 - 1, 1, 1024, 0) == 1                # N HW C = 2^31 and just below
    assert ok(2 ** 20, 2 ** 9, 4, 0) == 0 and ok(2 ** 40, 2 ** 40, 4, 0) == 0


def test_argument_errors_are_codes(lib):
    import ctypes
    buf = (ctypes.c_float * 80)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, as the entries ask of y, dy and the weights
    fwd, bwd, wg = lib.wc_critic_tail_fwd_f32, lib.wc_critic_tail_bwd_f32, lib.wc_critic_tail_wgrad_f32
    NULL, SHAPE, ARG = -1, -2, -5
    assert fwd(None, p, p, None, None, None, 1, 1, 4, 0, 1, p, p, None, None, None, None) == NULL
    assert fwd(p, p, p, None, None, None, 1, 1, 4, 0, 1, p, None, None, None, None, None) == NULL
    assert fwd(p, p, p, None, None, None, 1, 1, 4, 2, 1, p, p, p, p, None, None) == NULL            # K > 0 without the class head's weight
    assert fwd(p, p, p, p, p, p, 1, 1, 4, 2, 1, p, p, p, p, None, None) == NULL                    # labels without ce
    assert fwd(p, p, p, None, None, p, 1, 1, 4, 0, 1, p, p, None, None, p, None) == ARG            # labels without a class head
    assert fwd(p, p, p, None, None, None, 1, 1, 4, 0, 2, p, p, None, None, None, None) == ARG
    assert fwd(p, p, p, None, None, None, 1, 1, 6, 0, 1, p, p, None, None, None, None) == SHAPE
    assert fwd(p + 4, p, p, None, None, None, 1, 1, 4, 0, 1, p, p, None, None, None, None) == ARG           # y is read 16 bytes at a time
    assert bwd(p, p + 8, None, p, None, None, None, None, None, 1, 1, 4, 0, 1, None, p, None) == ARG
    assert fwd(p, p, p, None, None, None, 0, 1, 4, 0, 1, p, p, None, None, None, None) == SHAPE
    assert bwd(p, p, None, None, None, None, None, None, None, 1, 1, 4, 0, 1, None, p, None) == NULL
    assert bwd(p, p, p, p, None, p, None, None, None, 1, 1, 4, 2, 1, p, p, None) == NULL            # g_ce without the saved forward
    assert bwd(p, p, None, p, p, None, None, None, None, 1, 1, 4, 0, 1, None, p, None) == ARG       # g_logits without a class head
    assert bwd(p, p, None, p, None, None, None, None, None, 1, 1, 1028, 0, 1, None, p, None) == SHAPE
    assert bwd(p, p, None, p, None, None, None, None, None, 1, 1, 4, 0, -1, None, p, None) == ARG
    assert wg(p, p, None, 1, 4, 0, p, None, None, None, None) == NULL
    assert wg(p, p, None, 1, 4, 1, p, p, p, p, None) == NULL
    assert wg(p, p, None, 1, 4, 1025, p, p, p, p, None) == SHAPE


# ---------------------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_recipes_hold_what_their_scripts_say():
    from wc_gan_amd.train import ACGAN_CONFIGS, ACGAN_SCHEDULES
    assert set(ACGAN_CONFIGS) == set(ACGAN_SCHEDULES) == {'cifar10_wgan_cond', 'cifar10_wgan_cond_sa'}
    for name, after_norm in (('cifar10_wgan_cond', 'ucconv'), ('cifar10_wgan_cond_sa', 'ufconv')):
        cfg = ACGAN_CONFIGS[name]
        assert (cfg['gan_type'], cfg['conditional'], cfg['objective'], cfg['gradient_penalty_weight']) == ('AC_GAN', False, 'wgan', 10)
        g, d = cfg['generator'], cfg['discriminator']
        assert g['block_sizes'] == (128,) * 3 and g['first_block_shape'] == (4, 4, 128) and g['gan_type'] == 'AC_GAN'
        assert (g['block_norm'], g['block_after_norm'], g['last_norm'], g['last_after_norm']) == ('d', after_norm, 'd', 'uconv')
        assert d['block_sizes'] == (128,) * 4 and d['resamples'] == ('DOWN', 'DOWN', 'SAME', 'SAME')
        assert (d['type'], d['spectral'], d['sum_pool'], d['fused_tail'], d['number_of_classes']) == ('AC_GAN', False, True, True, 10)
        assert ACGAN_SCHEDULES[name] == dict(lr_decay_schedule='linear', number_of_epochs=100)
    assert ACGAN_CONFIGS['cifar10_wgan_cond_sa']['generator']['filters_emb'] == 4
    assert 'filters_emb' not in ACGAN_CONFIGS['cifar10_wgan_cond']['generator']             # the script leaves run.py's default


def test_the_existing_tables_keep_their_keys():
    from wc_gan_amd import train
    assert set(train.CONFIGS) == {'cifar10_uncond', 'cifar10_cond', 'stl10_uncond', 'tinyimagenet_cond_sa'}
    assert set(train.DCGAN_CONFIGS) == {'cifar10_dcgan_uncond', 'stl10_dcgan_uncond'}
    assert set(train.WGAN_CONFIGS) == {'cifar10_wgan_uncond'}
    assert set(train.RECIPE_SCHEDULES) == set(train.CONFIGS) | set(train.DCGAN_CONFIGS) | set(train.WGAN_CONFIGS)
    assert all('fused_tail' not in c['discriminator'] for t in (train.CONFIGS, train.DCGAN_CONFIGS, train.WGAN_CONFIGS) for c in t.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# the module and the trainer
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


@pytest.mark.parametrize("head", [None, 'AC_GAN'])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_the_flag_changes_the_route_not_the_map(head, sum_pool):
    from wc_gan_amd import tail
    plain = _critic(type=head, sum_pool=sum_pool)
    fused = _critic(type=head, sum_pool=sum_pool, fused_tail=True)
    assert plain.fused_tail is False and fused.fused_tail is True
    g = torch.Generator().manual_seed(2)
    x = torch.rand(3, 16, 16, 3, generator=g, dtype=torch.float64) * 2 - 1
    labels = torch.tensor([0, 6, 3])
    tail.last_route = None
    a = plain(x, None) if head is None else plain(x, None, labels=labels)
    assert tail.last_route is None
    b = fused(x, None) if head is None else fused(x, None, labels=labels)
    assert tail.last_route == 'torch'
    a, b = (t if isinstance(t, tuple) else (t,) for t in (a, b))
    assert len(a) == len(b) == (1 if head is None else 3)
    for s, t in zip(a, b):
        assert s.shape == t.shape and TR.rel(t, s) < 1e-12
    if head == 'AC_GAN':
        assert TR.rel(a[2], F.cross_entropy(a[1], labels, reduction='none')) < 1e-14
        for D in (plain, fused):            # without labels: the pair it always returned
            out = D(x, None)
            assert len(out) == 2 and torch.equal(out[0], a[0]) or TR.rel(out[0], a[0]) < 1e-12
    else:
        with pytest.raises(ValueError, match="labels"):
            plain(x, None, labels=labels)
    ga = torch.autograd.grad(sum(t.sum() for t in a), list(plain.parameters()))
    gb = torch.autograd.grad(sum(t.sum() for t in b), list(fused.parameters()))
    for (n, _), s, t in zip(plain.named_parameters(), ga, gb):
        assert TR.rel(t, s) < 1e-12, n


def test_projective_dcgan_and_dropout_keep_the_torch_tail():
    from wc_gan_amd.discriminator import make_discriminator
    assert not make_discriminator(**dict(CRITIC, type='PROJECTIVE', fused_tail=True))._tail_is_fused()
    assert not make_discriminator(**dict(CRITIC, type=None, dropout=0.2, fused_tail=True))._tail_is_fused()
    assert not make_discriminator(**dict(CRITIC, type=None, arch='dcgan', resamples=('SAME', 'DOWN'), fused_tail=True))._tail_is_fused()
    assert make_discriminator(**dict(CRITIC, type=None, fused_tail=True))._tail_is_fused()
    assert not make_discriminator(**dict(CRITIC, type='AC_GAN'))._tail_is_fused()


W_D, W_G, WEIGHT = 0.7, 1.3, 10.0


def _trainer(**kw):
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import GanTrainer
    torch.manual_seed(0)
    G = make_generator(block_sizes=(8, 8), resamples=("UP", "UP"), first_block_shape=(4, 4, 8), block_norm='b', block_after_norm='ucs',
                       last_norm='b', last_after_norm='ucs').double()       # 4 x 4 -> 16 x 16, the toy generator of tests/test_penalty_cpu.py
    with torch.no_grad():
        G(torch.zeros(2, 128, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.int32))
    D = _critic(type='AC_GAN', sum_pool=True, fused_tail=True)
    kw = dict(dict(gan_type='AC_GAN', objective='wgan', gradient_penalty_weight=WEIGHT, class_loss_weight_discriminator=W_D,
                   class_loss_weight_generator=W_G, number_of_classes=7), **kw)
    tr = GanTrainer(G, D, batch_size=3, training_ratio=1, generator_batch_multiple=1, flat_buckets=True, **kw)
    g = torch.Generator().manual_seed(6)
    real, fake = (torch.rand(3, 16, 16, 3, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(2))
    eps = torch.rand(3, generator=g, dtype=torch.float64)
    return tr, real, fake, eps


def _spy(opt, module):
    seen, step = {}, opt.step

    def spy(*a, **k):
        seen.update({n: p.grad.detach().clone() for n, p in module.named_parameters()})
        return step(*a, **k)
    opt.step = spy
    return seen


def test_ac_gan_updates_equal_a_hand_written_float64_step():
    tr, real, fake, eps = _trainer()
    real_cls, fake_cls = torch.tensor([0, 6, 2], dtype=torch.int32), torch.tensor([[5], [0], [6]], dtype=torch.int32)
    twin_d, twin_g = copy.deepcopy(tr.D), copy.deepcopy(tr.G)
    twin_d.fused_tail = False
    seen = _spy(tr.opt_d, tr.D)
    loss = tr.d_step(real, real_cls=real_cls, fake=fake, cls=fake_cls, eps=eps)

    out, logits = twin_d(torch.cat([real, fake]), None)
    ce = F.cross_entropy(logits, torch.cat([real_cls, fake_cls.reshape(-1)]).long(), reduction='none')
    e = eps.view(3, 1, 1, 1)
    x_hat = (e * real + (1 - e) * fake).requires_grad_(True)
    g, = torch.autograd.grad(twin_d(x_hat, None)[0].sum(), x_hat, create_graph=True)
    pen = WEIGHT * ((g.flatten(1).norm(dim=1) - 1) ** 2).mean()
    total = out[3:].mean() - out[:3].mean() + W_D * (ce[:3].mean() + ce[3:].mean()) + pen
    grads = torch.autograd.grad(total, list(twin_d.parameters()))
    assert TR.rel(loss, total) < 1e-10 and TR.rel(tr.last_penalty, pen) < 1e-10
    assert TR.rel(tr.last_class_losses[0], ce[:3].mean()) < 1e-10 and TR.rel(tr.last_class_losses[1], ce[3:].mean()) < 1e-10
    for (n, _), want in zip(twin_d.named_parameters(), grads):
        assert (float(want.abs().max()) > 0) == (n != 'out.bias') and TR.rel(seen[n], want) < 1e-10, n       # (the Wasserstein loss's +1/n, -1/n cancel there)

    # the generator's update, through the critic the update above left
    twin_d = copy.deepcopy(tr.D)
    twin_d.fused_tail = False
    z = torch.randn(3, 128, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    seen = _spy(tr.opt_g, tr.G)
    g_loss = tr.g_step((tr.G(z, fake_cls), fake_cls))
    out, logits = twin_d(twin_g(z, fake_cls), None)
    ce_g = F.cross_entropy(logits, fake_cls.reshape(-1).long(), reduction='none').mean()
    total = -out.mean() + W_G * ce_g
    grads = torch.autograd.grad(total, [p for p in twin_g.parameters() if p.requires_grad], allow_unused=True)
    assert TR.rel(g_loss, total) < 1e-10 and TR.rel(tr.last_class_losses[2], ce_g) < 1e-10
    names = [n for n, p in twin_g.named_parameters() if p.requires_grad]
    checked = 0
    top = max(float(w.abs().max()) for w in grads if w is not None)
    for n, want in zip(names, grads):
        if want is None or n not in seen:
            continue
        if float(want.abs().max()) < 1e-12 * top:       # a bias in front of a batch norm: zero but for rounding, in both
            assert float(seen[n].abs().max()) < 1e-12 * top, n
            continue
        assert TR.rel(seen[n], want) < 1e-10, n
        checked += 1
    assert checked >= 4
    assert all(p.requires_grad for p in tr.D.parameters())


def test_ac_gan_needs_labels_and_a_class_head():
    from wc_gan_amd.train import GanTrainer
    tr, real, fake, eps = _trainer()
    with pytest.raises(ValueError, match="real_labels"):
        tr.step([real])
    with pytest.raises(ValueError, match="real_cls"):
        tr.d_step(real, fake=fake, cls=torch.zeros(3, 1, dtype=torch.int32), eps=eps)
    with pytest.raises(ValueError, match="class head"):
        GanTrainer(tr.G, _critic(type=None, sum_pool=True), gan_type='AC_GAN')
    with pytest.raises(ValueError, match="gan_type"):
        GanTrainer(tr.G, tr.D, gan_type='PROJECTIVE')
    plain = GanTrainer(tr.G, _critic(type=None, sum_pool=True))
    assert plain.gan_type is None and plain.last_class_losses == [None, None, None]


def test_build_trainer_forwards_gan_type():
    from wc_gan_amd.train import ACGAN_CONFIGS, build_trainer
    cfg = copy.deepcopy(ACGAN_CONFIGS['cifar10_wgan_cond'])
    cfg['generator'].update(block_sizes=(8,), resamples=("UP",), first_block_shape=(4, 4, 8), block_norm='b', last_norm='b',
                            block_after_norm='ucs', last_after_norm='ucs')
    cfg['discriminator'].update(input_image_shape=(8, 8, 3), block_sizes=(8, 8), resamples=('DOWN', 'SAME'))
    t = build_trainer(cfg, device='cpu')
    assert (t.gan_type, t.objective, t.gp_weight, t.conditional, t.w_cls_d, t.w_cls_g) == ('AC_GAN', 'wgan', 10.0, False, 1.0, 1.0)
    assert t.D.fused_tail is True and t.D.type == 'AC_GAN'
