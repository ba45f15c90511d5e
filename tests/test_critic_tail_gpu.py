"""The critic's tail on the HIP route (csrc/wc_tail.hip through wc_gan_amd/tail.py) against tests/tail_reference.py in float64 on the same
fp32 inputs; the AC_GAN critic of the conditional WGAN-GP recipes with the fused tail against tests/critic_reference.Critic; and
GanTrainer(gan_type='AC_GAN'): one critic update and one generator update against a float64 step, then a captured step.

BOUNDS (kernel rows): per tensor, relative to the reference tensor's maximum; four times the worse error of the two fp32 routes -- the
kernels, and torch's fp32 composition relu -> sum/mean -> linear -> cross_entropy on the same GPU -- against float64 over the rows below,
rounded up to one digit, capped at the project's 1e-4 (the rule of tests/test_critic_gpu.py).  `PYTHONPATH=. python
tests/test_critic_tail_gpu.py` prints the table (profiles/tail_parity.txt).  dy is additionally exact zero wherever y <= 0."""
import pytest
import torch
import torch.nn.functional as F

import critic_reference as R
import penalty_reference as PR
import tail_reference as TR
from _poison import run_patterns, same_bits

CEILING = 1e-4
MASK_BAND = 1e-4
# worst over the rows of profiles/tail_parity.txt, the larger of the two routes, x 4, rounded up to one digit:
#   feat     hip 5.52e-08  torch fp32 1.37e-07  -> 5.5e-07 -> 6e-07
#   out      hip 2.40e-07  torch fp32 2.99e-06  -> 1.2e-05 -> 2e-05
#   logits   hip 1.08e-07  torch fp32 6.76e-07  -> 2.7e-06 -> 3e-06
#   lse      hip 1.08e-07  torch fp32 6.76e-07  -> 2.7e-06 -> 3e-06
#   ce       hip 1.65e-07  torch fp32 2.52e-07  -> 1.1e-06 -> 2e-06
#   dlogits  hip 5.39e-07  torch fp32 1.50e-06  -> 6.0e-06 -> 6e-06
#   dy       hip 2.89e-07  torch fp32 1.01e-06  -> 4.04e-06 -> 5e-06
#   dw_out   hip 1.36e-07  torch fp32 6.66e-07  -> 2.7e-06 -> 3e-06
#   db_out   hip 4.92e-08  torch fp32 3.30e-06  -> 1.3e-05 -> 2e-05
#   dW_cls   hip 5.53e-07  torch fp32 1.52e-06  -> 6.1e-06 -> 7e-06
#   db_cls   hip 4.36e-07  torch fp32 6.92e-06  -> 2.8e-05 -> 3e-05
BOUNDS = dict(feat=6e-7, out=2e-5, logits=3e-6, lse=3e-6, ce=2e-6, dlogits=6e-6, dy=5e-6, dw_out=3e-6, db_out=2e-5, dW_cls=7e-6, db_cls=3e-5)
assert all(b <= CEILING for b in BOUNDS.values())
KINDS = tuple(BOUNDS)

SHAPES = [(1, 1, 4), (3, 36, 132), (8, 64, 128), (128, 64, 128), (5, 144, 256), (4, 64, 1024)]      # (N, HW, C); (128, 64, 128) is the recipe's
GRID = {1: (1, 1), 36: (6, 6), 64: (8, 8), 144: (12, 12)}
CLASSES = [0, 1, 10, 200, 1024]


def _case(N, HW, C, K, sum_pool, seed, big_logits=False):
    """fp32 inputs on the GPU; the heads' weights sized so that out and the logits are of order one (big_logits: the logits reach +-200)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    H, W = GRID[HW]
    size = (0.4 * HW if sum_pool else 0.4) * C ** 0.5
    c = dict(y=rn(N, H, W, C), w_out=rn(C) / size, b_out=0.1 * rn(1), g_out=rn(N))
    if K:
        labels = torch.randint(0, K, (N,), generator=g, dtype=torch.int32)
        labels[0], labels[-1] = 0, K - 1
        c.update(w_cls=rn(K, C) / size, b_cls=0.1 * rn(K), g_logits=rn(N, K), g_ce=rn(N), labels=labels)
        if big_logits:
            fwd = TR.forward(c['y'], c['w_out'], c['b_out'], c['w_cls'], c['b_cls'], None, sum_pool)
            c['w_cls'] = (c['w_cls'].double() * (200.0 / float((fwd['logits'] - c['b_cls'].double()).abs().max()))).float()
    return {k: v.cuda() for k, v in c.items()}


def _hip(c, sum_pool, g_logits=True):
    """every tensor the three entries write, by name"""
    from wc_gan_amd import tail
    K = 'w_cls' in c
    feat, out, logits, lse, ce = tail.hip_forward(c['y'], c['w_out'], c['b_out'], c.get('w_cls'), c.get('b_cls'), c.get('labels'), sum_pool)
    dlogits, dy = tail.hip_backward(c['y'], c['w_out'], c.get('w_cls'), c['g_out'], c['g_logits'] if (K and g_logits) else None, c.get('g_ce'),
                                    logits, lse, c.get('labels'), sum_pool)
    dw_out, db_out, dW_cls, db_cls = tail.hip_wgrad(feat, c['g_out'], dlogits)
    r = dict(feat=feat, out=out[:, 0], dy=dy, dw_out=dw_out, db_out=db_out[0])
    if K:
        r.update(logits=logits, lse=lse, ce=ce, dlogits=dlogits, dW_cls=dW_cls, db_cls=db_cls)
    return r


def _torch_fp32(c, sum_pool, g_logits=True):
    """torch's composition of the same tail in fp32 on the GPU, differentiated by autograd: what an AC_GAN critic runs without the flag"""
    K = 'w_cls' in c
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('y', 'w_out', 'b_out') + (('w_cls', 'b_cls') if K else ())}
    f = F.relu(leaves['y'])
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, leaves['w_out'][None], leaves['b_out'])[:, 0]
    total = (out * c['g_out']).sum()
    r = dict(feat=f.detach(), out=out.detach())
    if K:
        logits = F.linear(f, leaves['w_cls'], leaves['b_cls'])
        logits.retain_grad()
        ce = F.cross_entropy(logits, c['labels'].long(), reduction='none')
        total = total + (ce * c['g_ce']).sum() + ((logits * c['g_logits']).sum() if g_logits else 0.0)
        r.update(logits=logits.detach(), lse=torch.logsumexp(logits.detach(), dim=1), ce=ce.detach())
    total.backward()
    r.update(dy=leaves['y'].grad, dw_out=leaves['w_out'].grad, db_out=leaves['b_out'].grad[0])
    if K:
        r.update(dlogits=logits.grad, dW_cls=leaves['w_cls'].grad, db_cls=leaves['b_cls'].grad)
    return r


def _reference(c, sum_pool, g_logits=True):
    K = 'w_cls' in c
    fwd = TR.forward(c['y'], c['w_out'], c['b_out'], c.get('w_cls'), c.get('b_cls'), c.get('labels'), sum_pool)
    bwd = TR.backward(c['y'], c['w_out'], c.get('w_cls'), fwd, c['g_out'], c['g_logits'] if (K and g_logits) else None, c.get('g_ce'),
                      c.get('labels'), sum_pool)
    return dict(fwd, **bwd)


def _errors(got, ref):
    for k in got:
        assert got[k].shape == ref[k].shape, k
    return {k: TR.rel(got[k], ref[k]) for k in got}


def _rows(shape):
    """(label, case, sum_pool, g_logits given) of one shape: every K and both poolings; g_logits absent, an all-negative sample and logits of
    +-200 at K = 10"""
    N, HW, C = shape
    rows = []
    for K in CLASSES:
        for sum_pool in (True, False):
            rows.append((f"K={K} {'sum' if sum_pool else 'mean'}", _case(N, HW, C, K, sum_pool, 100 + K), sum_pool, True))
    rows.append(("K=10 sum no g_logits", _case(N, HW, C, 10, True, 7), True, False))
    c = _case(N, HW, C, 10, False, 8)
    c['y'][0] = -c['y'][0].abs()
    rows.append(("K=10 mean sample 0 negative", c, False, True))
    rows.append(("K=10 sum logits +-200", _case(N, HW, C, 10, True, 9, big_logits=True), True, True))
    return rows


def _check(errs, label):
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (label, k, v, BOUNDS[k])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64(shape):
    for label, c, sum_pool, gl in _rows(shape):
        got, ref = _hip(c, sum_pool, gl), _reference(c, sum_pool, gl)
        assert all(torch.isfinite(t).all() for t in got.values()), label
        _check(_errors(got, ref), f"tail {shape} {label}")
        assert not got['dy'][c['y'] <= 0].any(), label                       # the mask, exactly
        if 'negative' in label:
            assert not got['feat'][0].any() and not got['dy'][0].any()
        if '+-200' in label:
            assert float(got['logits'].abs().max()) > 190
        again = _hip(c, sum_pool, gl)
        for k in got:
            assert same_bits(got[k], again[k]), (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 36, 132), (8, 64, 128)], ids=lambda s: "x".join(map(str, s)))
def test_a_label_equal_to_k_gives_nan_and_changes_nothing_else(shape):
    N, HW, C = shape
    K = 10
    c = _case(N, HW, C, K, True, 21)
    good = _hip(c, True)
    bad_c = dict(c, labels=c['labels'].clone())
    bad_c['labels'][1] = K
    bad = _hip(bad_c, True)
    keep = [n for n in range(N) if n != 1]
    assert torch.isnan(bad['ce'][1]) and torch.isfinite(bad['ce'][keep]).all()
    for k in ('feat', 'out', 'logits', 'lse'):
        assert same_bits(good[k], bad[k]), k
    for k in ('ce', 'dlogits', 'dy'):
        assert same_bits(good[k][keep], bad[k][keep]), k
    assert same_bits(bad['dlogits'][1], c['g_logits'][1])                     # no class gradient for that sample
    ref = _reference(bad_c, True)
    errs = _errors({k: v for k, v in bad.items() if k != 'ce'}, ref)
    errs['ce'] = TR.rel(bad['ce'][keep], ref['ce'][keep])
    _check(errs, f"tail {shape} label = K")


def _autograd_call(c, sum_pool, leaves=None):
    """tail.critic_tail + backward -> every output and gradient by name"""
    from wc_gan_amd import tail
    names = ('y', 'w_out', 'b_out', 'w_cls', 'b_cls')
    leaves = leaves or {k: c[k].detach().requires_grad_(True) for k in names}
    out, logits, ce = tail.critic_tail(leaves['y'], leaves['w_out'], leaves['b_out'], leaves['w_cls'], leaves['b_cls'], c['labels'], sum_pool)
    assert tail.last_route == 'hip'
    total = (out[:, 0] * c['g_out']).sum() + (logits * c['g_logits']).sum() + (ce * c['g_ce']).sum()
    grads = torch.autograd.grad(total, [leaves[k] for k in names])
    return dict(zip(('dy', 'dw_out', 'db_out', 'dW_cls', 'db_cls'), grads), out=out, logits=logits, ce=ce)


@pytest.mark.gpu
def test_autograd_node_under_poisoned_allocations():
    c = _case(3, 36, 132, 10, False, 31)
    ref = _reference(c, False)

    def run(P):
        g = {k: P.guarded(v) for k, v in c.items()}
        return _autograd_call(g, False)
    outs = run_patterns(run)
    for got in outs.values():
        got = dict(got, out=got['out'][:, 0], db_out=got['db_out'][0])
        _check(_errors(got, {k: ref[k].cpu() for k in got}), "tail poisoned")


@pytest.mark.gpu
def test_captured_forward_and_backward_replay_the_eager_bits():
    c = _case(8, 64, 128, 10, True, 41)
    eager = {k: v.clone() for k, v in _autograd_call(c, True).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _autograd_call(c, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _autograd_call(c, True)
    for _ in range(2):
        for t in static.values():
            t.detach().fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert same_bits(eager[k].detach(), static[k].detach()), k


# ---------------------------------------------------------------------------------------------------------------------------------
# the network: the cifar10_wgan_cond critic at batch 4 (eight images through the pass: N H W a multiple of 128 at every layer)
# ---------------------------------------------------------------------------------------------------------------------------------
NET = dict(out=3e-6, dx=4e-6, conv_w=6e-6, bias=2e-6, head=5e-6)        # tests/test_critic_gpu.py's BOUNDS, restated


def _kind(name):
    if name.startswith('blocks.'):
        return 'conv_w' if name.endswith('.weight') else 'bias'
    return 'head'


def _critic(kw, seed=5):
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(seed)
    D = make_discriminator(**kw)
    with torch.no_grad():
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.cuda()


class _Signs:
    """forward hooks that keep the fp32 tensors the critic applies its ReLUs to (the identity bn1 / bn2 sites and the last block's output,
    which the fused tail masks by `y > 0` itself)"""

    def __init__(self, D):
        self.D, self.rec, self.handles = D, {}, []
        for i, blk in enumerate(D.blocks):
            for part in ('bn1', 'bn2'):
                self.handles.append(getattr(blk, part).register_forward_hook(lambda _m, _i, out, key=f'{i}.{part}': self.rec.__setitem__(key, out.detach())))
        self.handles.append(D.blocks[-1].register_forward_hook(lambda _m, _i, out: self.rec.__setitem__('last', out.detach())))

    def masks(self):
        keys = [k for i in range(len(self.D.blocks)) for k in ((f'{i}.bn1',) if i else ()) + (f'{i}.bn2',)] + ['last']
        return [self.rec[k] > 0 for k in keys]

    def close(self):
        for h in self.handles:
            h.remove()


def _network_call(D, x, labels, weights):
    signs = _Signs(D)
    try:
        xg = x.detach().clone().requires_grad_(True)
        out, logits, ce = D(xg, None, labels=labels)
        total = (out * weights[0]).sum() + (logits * weights[1]).sum() + (ce * weights[2]).sum()
        names = [n for n, _ in D.named_parameters()]
        grads = dict(zip(['x'] + names, torch.autograd.grad(total, [xg] + list(D.parameters()))))
        return dict(out=out.detach(), logits=logits.detach(), ce=ce.detach()), grads, signs.masks()
    finally:
        signs.close()


def _network_reference(state, kw, x, labels, weights, masks):
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=0, masks=masks, **{k: v for k, v in kw.items() if k != 'fused_tail'})
    x64 = x.detach().double().requires_grad_(True)
    out, logits = critic(x64, None)
    ce = F.cross_entropy(logits, labels.reshape(-1).long(), reduction='none')
    total = (out * weights[0].double()).sum() + (logits * weights[1].double()).sum() + (ce * weights[2].double()).sum()
    names = list(params)
    grads = dict(zip(['x'] + names, torch.autograd.grad(total, [x64] + [params[n] for n in names])))
    worst, count = R.mask_disagreement(masks, critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    return dict(out=out.detach(), logits=logits.detach(), ce=ce.detach()), grads


@pytest.mark.gpu
def test_recipe_critic_with_and_without_the_fused_tail():
    from wc_gan_amd import tail
    from wc_gan_amd.train import ACGAN_CONFIGS
    kw = dict(ACGAN_CONFIGS['cifar10_wgan_cond']['discriminator'])
    assert kw['fused_tail'] is True
    fused, plain = _critic(kw), _critic(dict(kw, fused_tail=False))
    plain.load_state_dict(fused.state_dict())
    state = {k: v.detach().clone() for k, v in fused.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(8, 32, 32, 3, generator=g) * 2 - 1).cuda()
    labels = torch.randint(0, 10, (8, 1), generator=g, dtype=torch.int32).cuda()
    weights = (torch.randn(8, 1, generator=g).cuda(), torch.randn(8, 10, generator=g).cuda(), torch.randn(8, generator=g).cuda())
    results = {}
    for name, D in (('fused', fused), ('plain', plain)):
        tail.last_route = None
        outs, grads, masks = _network_call(D, x, labels, weights)
        assert tail.last_route == ('hip' if name == 'fused' else None)
        outs64, grads64 = _network_reference(state, kw, x, labels, weights, masks)
        errs = dict.fromkeys(NET, 0.0)
        for k in outs:
            assert outs[k].shape == outs64[k].shape
            errs['out'] = max(errs['out'], TR.rel(outs[k], outs64[k]))
        assert set(grads) == set(grads64)
        for n, gr in grads.items():
            kind = 'dx' if n == 'x' else _kind(n)
            errs[kind] = max(errs[kind], TR.rel(gr, grads64[n]))
        print(f"critic cifar10_wgan_cond {name}", {k: f"{v:.2e}" for k, v in errs.items()})
        for k, v in errs.items():
            assert v < NET[k], (name, k, v, NET[k])
        results[name] = (outs, grads, outs64, grads64)
    # the two routes against each other: each within its bound of (nearly) the same reference
    (fo, fg, ref_o, ref_g), (po, pg, _, _) = results['fused'], results['plain']
    for k in fo:
        assert float((fo[k] - po[k]).abs().max()) <= 2 * NET['out'] * float(ref_o[k].abs().max()), k
    for n in fg:
        kind = 'dx' if n == 'x' else _kind(n)
        assert float((fg[n] - pg[n]).abs().max()) <= 2 * NET[kind] * float(ref_g[n].abs().max()), n


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
PEN = dict(conv_w=2e-5, head=2e-6, norms=6e-7, penalty=6e-7)             # tests/test_penalty_gpu.py's BOUNDS, restated
WEIGHT = 10.0


def _spy(opt, module):
    seen, step = {}, opt.step

    def spy(*a, **k):
        seen.update({n: p.grad.detach().clone() for n, p in module.named_parameters()})
        return step(*a, **k)
    opt.step = spy
    return seen, step


@pytest.mark.gpu
@pytest.mark.parametrize("name", ['cifar10_wgan_cond', 'cifar10_wgan_cond_sa'])
def test_ac_gan_trainer_updates_against_float64(name):
    from wc_gan_amd import penalty, tail
    from wc_gan_amd.train import ACGAN_CONFIGS, build_trainer
    cfg = ACGAN_CONFIGS[name]
    n = 4
    tr = build_trainer(cfg, 'cuda', batch_size=n, training_ratio=1, seed=3)
    assert (tr.gan_type, tr.objective, tr.gp_weight, tr.D.fused_tail) == ('AC_GAN', 'wgan', 10.0, True)
    with torch.no_grad():
        for pname, p in tr.D.named_parameters():
            if pname.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(8)
    real, fake = ((torch.rand(n, 32, 32, 3, generator=g) * 2 - 1).cuda() for _ in range(2))
    eps = torch.rand(n, generator=g).cuda()
    real_cls = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).cuda()
    fake_cls = torch.randint(0, 10, (n, 1), generator=g, dtype=torch.int32).cuda()
    labels = torch.cat([real_cls, fake_cls.reshape(-1)])
    state = {k: v.detach().clone() for k, v in tr.D.state_dict().items()}
    kw = {k: v for k, v in cfg['discriminator'].items() if k != 'fused_tail'}

    signs = _Signs(tr.D)
    seen, step = _spy(tr.opt_d, tr.D)
    tail.last_route = None
    loss = tr.d_step(real, real_cls=real_cls, fake=fake, cls=fake_cls, eps=eps)
    tr.opt_d.step = step
    signs.close()
    assert tail.last_route == 'hip'
    # the float64 step: the Wasserstein and the class loss through critic_reference.Critic with that pass's signs, the penalty with the engine's
    w_masks = signs.masks()
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=0, masks=w_masks, **kw)
    out64, logits64 = critic(torch.cat([real, fake]).double(), None)
    worst, count = R.mask_disagreement(w_masks, critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    ce64 = F.cross_entropy(logits64, labels.long(), reduction='none')
    plist = list(params.values())
    parts = [out64[n:].mean(), out64[:n].mean(), ce64[:n].mean(), ce64[n:].mean()]
    pg = [torch.autograd.grad(p, plist, retain_graph=True, allow_unused=True) for p in parts]
    pg = [[torch.zeros_like(q) if t is None else t for q, t in zip(plist, row)] for row in pg]
    want_pass = {k: a - b + c + d for k, a, b, c, d in zip(params, *pg)}
    size_pass = {k: float(sum(t.abs().max() for t in row)) for k, *row in zip(params, *pg)}
    x_hat = penalty.interpolate(real, fake, eps)
    pen64, norms64, grads64, pcritic = PR.reference_penalty(state, kw, x_hat, None, WEIGHT, penalty.last_masks)
    worst, count = R.mask_disagreement(penalty.last_masks, pcritic.pre)
    assert worst <= MASK_BAND, (worst, count)
    assert PR.rel(tr.last_penalty, pen64) < PEN['penalty'] and PR.rel(tr.last_grad_norms, norms64) < PEN['norms']
    ce_scale = float(ce64.abs().max())
    for got, want in zip(tr.last_class_losses[:2], (ce64[:n].mean(), ce64[n:].mean())):
        assert abs(float(got) - float(want)) < NET['out'] * ce_scale
    total64 = float(parts[0] - parts[1] + parts[2] + parts[3] + pen64)
    assert abs(float(loss) - total64) < 2 * NET['out'] * (float(out64.abs().max()) + ce_scale) + PEN['penalty'] * float(pen64)
    for pname, _p in tr.D.named_parameters():
        want = want_pass[pname].detach() + grads64[pname]
        kind = _kind(pname)
        tol = NET[kind] * size_pass[pname] + PEN.get(kind, 0.0) * float(grads64[pname].abs().max())
        err = float((seen[pname].double() - want).abs().max())
        print(f"  {pname}: error {err:.2e}, allowed {tol:.2e}")
        assert err <= tol, (pname, err, tol)
    assert float(want_pass['cls_out.weight'].abs().max()) > 0 and not grads64['cls_out.weight'].any()      # the penalty is on the adversarial head

    # the generator's update: its loss and class loss against the float64 critic on the batch it generated
    state = {k: v.detach().clone() for k, v in tr.D.state_dict().items()}
    z, cls = tr._noise(n * tr.gbm)
    with torch.no_grad():
        batch = tr.G(z, cls).detach().clone()
    signs = _Signs(tr.D)
    before = [p.detach().clone() for p in tr.G.parameters()]
    g_loss = tr.g_step((tr.G(z, cls), cls))
    signs.close()
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=0, masks=signs.masks(), **kw)
    out64, logits64 = critic(batch.double(), None)
    worst, count = R.mask_disagreement(signs.masks(), critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    ce64 = F.cross_entropy(logits64, cls.reshape(-1).long(), reduction='none')
    scale = float(out64.abs().max()) + float(ce64.abs().max())
    assert abs(float(tr.last_class_losses[2]) - float(ce64.mean())) < NET['out'] * float(ce64.abs().max())
    assert abs(float(g_loss) - float(-out64.mean() + ce64.mean())) < 2 * NET['out'] * scale
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, tr.G.parameters()))
    assert all(p.requires_grad for p in tr.D.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ['cifar10_wgan_cond', 'cifar10_wgan_cond_sa'])
def test_captured_ac_gan_step_replays(name):
    """lr = 0: the weights stand still, so a replay and an eager step from the same generator seed see the same inputs"""
    from wc_gan_amd.train import ACGAN_CONFIGS, build_trainer
    n = 4
    tr = build_trainer(ACGAN_CONFIGS[name], 'cuda', batch_size=n, training_ratio=1, seed=3, lr=0.0)
    g = torch.Generator().manual_seed(9)
    real = (torch.rand(n, 32, 32, 3, generator=g) * 2 - 1).cuda()
    real_cls = torch.randint(0, 10, (n,), generator=g, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="real_labels"):
        tr.step([real])
    replay = tr.capture([real], [real_cls])
    weights = [p.detach().clone() for p in list(tr.D.parameters()) + list(tr.G.parameters())]
    got = []
    for seed in (50, 51):
        torch.cuda.manual_seed(seed)
        d_loss, g_loss = replay()
        torch.cuda.synchronize()
        got.append([float(d_loss), float(g_loss), float(tr.last_penalty)] + [float(t) for t in tr.last_class_losses])
    assert all(torch.isfinite(torch.tensor(row)).all() for row in got)
    assert got[0] != got[1]                                                 # fresh noise in every replay
    assert all(torch.equal(a, p.detach()) for a, p in zip(weights, list(tr.D.parameters()) + list(tr.G.parameters())))
    torch.cuda.manual_seed(51)
    d_loss, g_loss = tr.step([real], [real_cls])
    eager = [float(d_loss), float(g_loss), float(tr.last_penalty)] + [float(t) for t in tr.last_class_losses]
    # d_loss = Wasserstein + class + penalty, g_loss = -mean out + class: each part within its bound in both runs, relative to the sizes
    # of the critic's outputs (the largest of 1, the adversarial output on the real batch and the class losses)
    with torch.no_grad():
        size = max(1.0, float(tr.D(real, None)[0].abs().max()), *eager[3:])
    tol = [2 * (2 * NET['out'] * 2 * size + PEN['penalty'] * eager[2]), 2 * 2 * NET['out'] * 2 * size, 2 * PEN['penalty'] * eager[2]] + \
        [2 * NET['out'] * size] * 3
    print("replay", got[1], "eager", eager, "allowed", tol)
    for a, b, t in zip(got[1], eager, tol):
        assert abs(a - b) <= t, (got[1], eager, tol)


if __name__ == '__main__':
    print(f"{'row':<44}{'route':<12}" + ''.join(f"{k:>10}" for k in KINDS), flush=True)
    worst = {route: dict.fromkeys(KINDS, 0.0) for route in ('hip', 'torch fp32')}
    for shape in SHAPES:
        for label, c, sum_pool, gl in _rows(shape):
            ref = _reference(c, sum_pool, gl)
            for route, fn in (('hip', _hip), ('torch fp32', _torch_fp32)):
                errs = _errors(fn(c, sum_pool, gl), ref)
                print(f"{str(shape) + ' ' + label:<44}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" if k in errs else f"{'-':>10}" for k in KINDS), flush=True)
                for k, v in errs.items():
                    worst[route][k] = max(worst[route][k], v)
    for route in worst:
        print(f"{'worst':<44}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in KINDS), flush=True)
