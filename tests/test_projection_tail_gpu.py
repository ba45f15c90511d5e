"""The projection critic's tail on the HIP route (csrc/wc_tail.hip through wc_gan_amd/tail.py: projection_tail) against
tests/projection_reference.py in float64 on the same fp32 inputs; SN PROJECTIVE critics with `fused_projection` against
tests/critic_reference.Critic; and the trainer on a shrunken cifar100_cond_sa: one critic and one generator update against a float64
hinge step, then a captured step.

BOUNDS (kernel rows): per tensor, relative to the reference tensor's maximum; four times the worse error of the two fp32 routes -- the
kernels, and torch's fp32 composition relu -> sum/mean -> linear + embedding * f on the same GPU -- against float64 over the rows of
projection_reference.rows, rounded up to one digit, capped at the project's 1e-4 (the rule of tests/test_critic_gpu.py).  `PYTHONPATH=.
python tests/test_projection_tail_gpu.py` prints the table into profiles/projection_tail_parity.txt.  Beyond the bounds: dy is exactly
zero wherever y <= 0, and the dE row of a class no sample carries is exactly zero."""
import copy

import pytest
import torch
import torch.nn.functional as F

import critic_reference as R
import projection_reference as PRJ
from _poison import run_patterns, same_bits
from projection_reference import rel

CEILING = 1e-4
MASK_BAND = 1e-4
# worst over the rows of profiles/projection_tail_parity.txt, the larger of the two routes, x 4, rounded up to one digit:
#   feat     hip 5.52e-08  torch fp32 1.36e-07  -> 5.5e-07 -> 6e-07
#   out      hip 6.06e-07  torch fp32 3.21e-06  -> 1.3e-05 -> 2e-05
#   dy       hip 5.51e-08  torch fp32 1.15e-07  -> 4.6e-07 -> 5e-07
#   dw_out   hip 1.52e-07  torch fp32 8.40e-07  -> 3.4e-06 -> 4e-06
#   db_out   hip 5.57e-08  torch fp32 7.96e-07  -> 3.2e-06 -> 4e-06
#   dE       hip 1.17e-07  torch fp32 5.70e-07  -> 2.3e-06 -> 3e-06
BOUNDS = dict(feat=6e-7, out=2e-5, dy=5e-7, dw_out=4e-6, db_out=4e-6, dE=3e-6)
assert all(b <= CEILING for b in BOUNDS.values())
KINDS = tuple(BOUNDS)
IDS = lambda s: "x".join(map(str, s))


def _cuda(c):
    return {k: (None if v is None else v.cuda()) for k, v in c.items()}


def _hip(c, sum_pool):
    """every tensor the three entries write, by name"""
    from wc_gan_amd import tail
    feat, out = tail.hip_projection_forward(c['y'], c['w_out'], c['b_out'], c['emb'], c['cls'], sum_pool)
    dy = tail.hip_projection_backward(c['y'], c['w_out'], c['emb'], c['cls'], c['g_out'], sum_pool)
    dw_out, db_out, dE = tail.hip_projection_wgrad(feat, c['g_out'], c['cls'], c['emb'].shape[0])
    return dict(feat=feat, out=out[:, 0], dy=dy, dw_out=dw_out, db_out=db_out[0], dE=dE)


def _torch_fp32(c, sum_pool):
    """torch's composition of the same tail in fp32 on the GPU, differentiated by autograd: what a PROJECTIVE critic runs without the flag"""
    leaves = {k: c[k].clone().requires_grad_(True) for k in ('y', 'w_out', 'b_out', 'emb') if c[k] is not None}
    f = F.relu(leaves['y'])
    f = f.sum(dim=(1, 2)) if sum_pool else f.mean(dim=(1, 2))
    out = F.linear(f, leaves['w_out'][None], leaves.get('b_out'))
    out = (out + (F.embedding(c['cls'].long(), leaves['emb']) * f).sum(dim=1, keepdim=True))[:, 0]
    (out * c['g_out']).sum().backward()
    db = leaves['b_out'].grad[0] if 'b_out' in leaves else c['g_out'].sum()
    return dict(feat=f.detach(), out=out.detach(), dy=leaves['y'].grad, dw_out=leaves['w_out'].grad, db_out=db, dE=leaves['emb'].grad)


def _errors(got, ref):
    for k in got:
        assert got[k].shape == ref[k].shape, k
    return {k: rel(got[k], ref[k]) for k in got}


def _check(errs, label):
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (label, k, v, BOUNDS[k])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PRJ.SHAPES, ids=IDS)
def test_kernels_against_float64(shape):
    N, HW, C, K = shape
    for label, c, sum_pool in PRJ.rows(shape):
        c = _cuda(c)
        got, ref = _hip(c, sum_pool), PRJ.reference(c, sum_pool)
        assert all(torch.isfinite(t).all() for t in got.values()), label
        _check(_errors(got, ref), f"projection {shape} {label}")
        assert not got['dy'][c['y'] <= 0].any(), label                          # the mask, exactly
        absent = torch.ones(K, dtype=torch.bool, device='cuda')
        absent[c['cls'].long()] = False
        assert not got['dE'][absent].any(), label                               # written in full: no row is left to a memset
        assert int(absent.sum()) >= K - N
        if 'equal' in label:
            assert int(absent.sum()) == K - 1
        if 'distinct' in label:
            assert int(absent.sum()) == K - N
        if 'negative' in label:
            assert not got['feat'][0].any() and not got['dy'][0].any()
        again = _hip(c, sum_pool)
        for k in got:
            assert same_bits(got[k], again[k]), (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 36, 132, 7), (8, 64, 128, 10)], ids=IDS)
def test_labels_outside_the_classes_give_nan_and_change_nothing_else(shape):
    """a label equal to K and a label of -1, through the entries and the reference alone"""
    N, HW, C, K = shape
    c = _cuda(PRJ.case(N, HW, C, K, True, 21))
    good = _hip(c, True)
    bad_c = dict(c, cls=c['cls'].clone())
    bad_c['cls'][1], bad_c['cls'][2] = K, -1
    bad = _hip(bad_c, True)
    keep = [n for n in range(N) if n not in (1, 2)]
    assert torch.isnan(bad['out'][[1, 2]]).all() and torch.isfinite(bad['out'][keep]).all()
    for k in ('feat', 'dw_out', 'db_out'):
        assert same_bits(good[k], bad[k]), k
    for k in ('out', 'dy'):
        assert same_bits(good[k][keep], bad[k][keep]), k
    untouched = [k for k in range(K) if k not in (int(c['cls'][1]), int(c['cls'][2]))]
    assert same_bits(good['dE'][untouched], bad['dE'][untouched])
    ref = PRJ.reference(bad_c, True)
    errs = _errors({k: v for k, v in bad.items() if k != 'out'}, ref)
    errs['out'] = rel(bad['out'][keep], ref['out'][keep])
    _check(errs, f"projection {shape} labels K and -1")
    assert not bad['dy'][bad_c['y'] <= 0].any()


def _autograd_call(c, sum_pool):
    """tail.projection_tail + backward -> the output and every gradient by name"""
    from wc_gan_amd import tail
    names = ('y', 'w_out', 'b_out', 'emb')
    leaves = {k: c[k].detach().requires_grad_(True) for k in names}
    out = tail.projection_tail(leaves['y'], leaves['w_out'], leaves['b_out'], leaves['emb'], c['cls'], sum_pool)
    assert tail.last_route == 'hip' and out.shape == (c['y'].shape[0], 1)
    grads = torch.autograd.grad((out[:, 0] * c['g_out']).sum(), [leaves[k] for k in names])
    return dict(zip(('dy', 'dw_out', 'db_out', 'dE'), grads), out=out)


@pytest.mark.gpu
def test_autograd_node_under_poisoned_allocations():
    c = PRJ.case(3, 36, 132, 7, False, 31)
    ref = PRJ.reference(c, False)

    def run(P):
        g = {k: P.guarded(v) for k, v in c.items()}
        first = _autograd_call(g, False)
        again = _autograd_call(g, False)
        for k in first:
            assert same_bits(first[k], again[k]), k
        return first
    outs = run_patterns(run)
    for got in outs.values():
        got = dict(got, out=got['out'][:, 0], db_out=got['db_out'][0])
        _check(_errors(got, {k: ref[k] for k in got}), "projection poisoned")


@pytest.mark.gpu
def test_captured_forward_and_backward_replay_the_eager_bits():
    c = _cuda(PRJ.case(8, 64, 128, 10, True, 41))
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
# the network: tests/test_critic_gpu.py's comparison (the float64 critic on the HIP route's ReLU signs; output, input gradient and every
# parameter gradient, emb.weight under kind 'head'; one eval call and two training calls, so that the power iteration advances)
# ---------------------------------------------------------------------------------------------------------------------------------
NET = dict(out=3e-6, dx=4e-6, conv_w=6e-6, bias=2e-6, head=5e-6)        # tests/test_critic_gpu.py's BOUNDS, restated
SYNTHETIC = dict(input_image_shape=(16, 16, 3), block_sizes=(128, 256), resamples=('DOWN', 'SAME'), number_of_classes=10, type='PROJECTIVE',
                 spectral=True, sum_pool=True, conv_singular=False)


def _network(kw, batch, label, route):
    import test_critic_gpu as TC
    from wc_gan_amd import tail
    assert TC.BOUNDS == NET
    for training in (False, True):
        tail.last_route = None
        calls = TC._critic_errors(kw, batch, training)
        assert tail.last_route == route
        for call, errs in enumerate(calls):
            name = f"critic {label} {'train call ' + str(call + 1) if training else 'eval'}"
            print(name, {k: f"{v:.2e}" for k, v in errs.items()})
            for k, v in errs.items():
                assert v < NET[k], (name, k, v, NET[k])


@pytest.mark.gpu
@pytest.mark.parametrize("sum_pool", [True, False])
def test_sn_projection_critic_on_the_fused_route(sum_pool):
    _network(dict(SYNTHETIC, sum_pool=sum_pool, fused_projection=True), 8, f"synthetic {'sum' if sum_pool else 'mean'}", 'hip')


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [True, False])
def test_recipe_critic_with_and_without_the_flag(flag):
    from wc_gan_amd.train import CONFIGS
    _network(dict(CONFIGS['cifar10_cond']['discriminator'], fused_projection=flag), 2, f"cifar10_cond flag {flag}", 'hip' if flag else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer: cifar100_cond_sa shrunk to 16 x 16 images (two generator blocks, critic blocks (128, 256) DOWN SAME), batch 8
# ---------------------------------------------------------------------------------------------------------------------------------
def _shrunken():
    from wc_gan_amd.train import PROJECTION_CONFIGS, fused_projection_config
    cfg = fused_projection_config(PROJECTION_CONFIGS['cifar100_cond_sa'])
    cfg['generator'].update(block_sizes=(128, 128), resamples=("UP", "UP"))
    cfg['discriminator'].update(input_image_shape=(16, 16, 3), block_sizes=(128, 256), resamples=('DOWN', 'SAME'))
    cfg['image_shape'] = (16, 16, 3)
    return cfg


def _spy(opt, module):
    seen, step = {}, opt.step

    def spy(*a, **k):
        seen.update({n: p.grad.detach().clone() for n, p in module.named_parameters()})
        return step(*a, **k)
    opt.step = spy
    return seen, step


def _float64_critic(state, kw, x, cls, masks):
    params, buffers = R.leaves(state)
    critic = R.Critic(params, buffers, iterations=1, masks=masks, **kw)         # training mode: one power iteration, as the pass ran
    out = critic(x.double(), cls)
    worst, count = R.mask_disagreement(masks, critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    return params, out


@pytest.mark.gpu
def test_projection_trainer_updates_against_float64():
    import test_critic_gpu as TC
    from wc_gan_amd import tail
    from wc_gan_amd.train import build_trainer
    cfg = _shrunken()
    n = 8
    tr = build_trainer(cfg, 'cuda', batch_size=n, training_ratio=1, seed=3)
    assert (tr.gan_type, tr.objective, tr.conditional, tr.D.fused_projection, tr.K) == (None, 'hinge', True, True, 100)
    with torch.no_grad():
        for pname, p in tr.D.named_parameters():
            if pname.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(8)
    real, fake = ((torch.rand(n, 16, 16, 3, generator=g) * 2 - 1).cuda() for _ in range(2))
    real_cls = torch.randint(0, 100, (n,), generator=g, dtype=torch.int32).cuda()
    fake_cls = torch.randint(0, 100, (n, 1), generator=g, dtype=torch.int32).cuda()
    both = torch.cat([real_cls.reshape(-1, 1), fake_cls])
    state = {k: v.detach().clone() for k, v in tr.D.state_dict().items()}
    kw = cfg['discriminator']

    probe = TC._Probe(tr.D)
    seen, step = _spy(tr.opt_d, tr.D)
    tail.last_route = None
    loss = tr.d_step(real, real_cls=real_cls, fake=fake, cls=fake_cls)
    tr.opt_d.step = step
    probe.close()
    assert tail.last_route == 'hip'
    params, out64 = _float64_critic(state, kw, torch.cat([real, fake]), both, probe.masks())
    margin = float(torch.minimum((1 - out64[:n]).abs().min(), (1 + out64[n:]).abs().min()).detach())
    assert margin > 10 * NET['out'] * float(out64.abs().max()), margin          # no sample sits on the hinge's kink
    parts = [F.relu(1.0 - out64[:n]).mean(), F.relu(1.0 + out64[n:]).mean()]
    assert float(parts[0]) > 0 and float(parts[1]) > 0
    plist = list(params.values())
    pg = [torch.autograd.grad(p, plist, retain_graph=True, allow_unused=True) for p in parts]
    pg = [[torch.zeros_like(q) if t is None else t for q, t in zip(plist, row)] for row in pg]
    assert abs(float(loss) - float(parts[0] + parts[1])) < 2 * NET['out'] * float(out64.abs().max())
    assert set(seen) == set(params)
    for pname, a, b in zip(params, *pg):
        kind = TC._kind(pname)
        tol = NET[kind] * float(a.abs().max() + b.abs().max())
        err = float((seen[pname].double() - (a + b)).abs().max())
        print(f"  {pname}: error {err:.2e}, allowed {tol:.2e}")
        assert err <= tol, (pname, err, tol)
    demb = seen['emb.weight']
    carried = torch.zeros(100, dtype=torch.bool, device='cuda')
    carried[both.reshape(-1).long()] = True
    assert float(demb.abs().max()) > 0 and not demb[~carried].any()             # dense, and exactly zero where no sample's class is

    # the generator's update: its loss against the float64 critic on the batch it generated
    state = {k: v.detach().clone() for k, v in tr.D.state_dict().items()}
    z, cls = tr._noise(n * tr.gbm)
    with torch.no_grad():
        batch = tr.G(z, cls).detach().clone()
    probe = TC._Probe(tr.D)
    before = [p.detach().clone() for p in tr.G.parameters()]
    g_loss = tr.g_step((tr.G(z, cls), cls))
    probe.close()
    _, out64 = _float64_critic(state, kw, batch, cls, probe.masks())
    assert abs(float(g_loss) - float(-out64.mean())) < 2 * NET['out'] * float(out64.abs().max())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, tr.G.parameters()))
    assert all(p.requires_grad for p in tr.D.parameters())


@pytest.mark.gpu
def test_captured_projection_step_replays():
    """lr = 0 keeps the weights; the buffers a step moves (the power iteration's u and v, the generator's running statistics) are put back
    before the eager step, so that it starts from the state the first replay started from"""
    from wc_gan_amd import tail
    from wc_gan_amd.train import build_trainer
    n = 8
    tr = build_trainer(_shrunken(), 'cuda', batch_size=n, training_ratio=1, seed=3, lr=0.0)
    g = torch.Generator().manual_seed(9)
    real = (torch.rand(n, 16, 16, 3, generator=g) * 2 - 1).cuda()
    real_cls = torch.randint(0, 100, (n,), generator=g, dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match="real_labels"):
        tr.step([real])
    tail.last_route = None
    replay = tr.capture([real], [real_cls])
    assert tail.last_route == 'hip'
    saved = [copy.deepcopy(m.state_dict()) for m in (tr.D, tr.G)]
    got = []
    for seed in (50, 51):
        torch.cuda.manual_seed(seed)
        d_loss, g_loss = replay()
        torch.cuda.synchronize()
        got.append([float(d_loss), float(g_loss)])
    assert all(torch.isfinite(torch.tensor(row)).all() for row in got)
    assert got[0] != got[1]                                                 # fresh noise in every replay
    for m, sd in zip((tr.D, tr.G), saved):
        assert all(torch.equal(sd[k], p.detach()) for k, p in m.named_parameters())
        m.load_state_dict(sd)
    torch.cuda.manual_seed(50)
    d_loss, g_loss = tr.step([real], [real_cls])
    eager = [float(d_loss), float(g_loss)]
    # both runs are fp32 evaluations of one map from one state, each within the network's output bound of the float64 value, relative to
    # the size of the critic's outputs (at least 1, the hinge's offset); d_loss has two such terms
    with torch.no_grad():
        size = max(1.0, float(tr.D(real, real_cls.reshape(-1, 1)).abs().max()))
    tol = [2 * 2 * NET['out'] * 2 * size, 2 * NET['out'] * 2 * size]
    print("replay", got[0], "eager", eager, "allowed", tol)
    for a, b, t in zip(got[0], eager, tol):
        assert abs(a - b) <= t, (got[0], eager, tol)


if __name__ == '__main__':
    import os
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                              'projection_tail_parity.txt')
    lines = [f"{'row':<60}{'route':<12}" + ''.join(f"{k:>10}" for k in KINDS)]
    worst = {route: dict.fromkeys(KINDS, 0.0) for route in ('hip', 'torch fp32')}
    for shape in PRJ.SHAPES:
        for label, c, sum_pool in PRJ.rows(shape):
            c = _cuda(c)
            ref = PRJ.reference(c, sum_pool)
            for route, fn in (('hip', _hip), ('torch fp32', _torch_fp32)):
                errs = _errors(fn(c, sum_pool), ref)
                lines.append(f"{str(shape) + ' ' + label:<60}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" for k in KINDS))
                for k, v in errs.items():
                    worst[route][k] = max(worst[route][k], v)
    for route in worst:
        lines.append(f"{'worst':<60}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in KINDS))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines), flush=True)
