"""optim.ScheduledAdam on the HIP route (csrc/wc_adam.hip: wc_adam_tick + wc_adam_update_f32) against the float64 numpy reference
(tests/adam_reference.py), on guarded, poisoned device memory.

Tolerance.  Storing an fp32 value rounds it once per step, so no implementation beats T x 2^-24 x max|ref| after T steps.  Beyond that
floor the yardstick is torch's own fp32 fused Adam, run in the same test from the same start on the same gradients: its worst error
against the reference, per tensor kind (parameter, exp_avg_sq, exp_avg).  The HIP route is allowed 4 x that error or the floor, whichever is
larger -- never a figure taken from the HIP route itself.  `PYTHONPATH=. python tests/test_optim_gpu.py` prints both routes' errors, the
table kept in profiles/adam_parity.txt."""
import numpy as np
import pytest
import torch

import adam_reference as AR
from _poison import Poison, same_bits

LR, B2, EPS = 2e-4, 0.9, 1e-8
STEPS, TOTAL = 4, 3            # 'linear' over 3 updates: the multipliers are 1, 2/3, 1/3 and 0
KINDS = ('param', 'exp_avg_sq', 'exp_avg')


def _ragged_numels():
    from wc_gan_amd import _lib, optim
    c = optim.CHUNK
    head = [1, 3, 4, 5, 127, 128, 129, c - 1, c, c + 1, 2 * c + 7]
    return head + [1] * (_lib.ADAM_CAPACITY - len(head) + 3)          # three tensors more than one table holds: a second launch


def _values(numels, steps, seed):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in numels]
    grads = [[(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for n in numels] for _ in range(steps)]
    return params, grads


def _err(t, ref):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64).reshape(-1) - np.asarray(ref).reshape(-1)).max())


class _Errors:
    """worst absolute error per kind and route, and the largest reference magnitude per kind (the floor's scale)"""

    def __init__(self):
        self.worst = {r: dict.fromkeys(KINDS, 0.0) for r in ('hip', 'torch')}
        self.scale = dict.fromkeys(KINDS, 0.0)

    def add(self, route, kind, t, ref):
        self.worst[route][kind] = max(self.worst[route][kind], _err(t, ref))
        self.scale[kind] = max(self.scale[kind], float(np.abs(ref).max()))

    def check(self, steps, label):
        for kind in KINDS:
            hip, tor = self.worst['hip'][kind], self.worst['torch'][kind]
            floor = steps * 2.0 ** -24 * self.scale[kind]
            print(f"{label:<34}{kind:<12}hip {hip:9.3e}   torch fp32 {tor:9.3e}   floor {floor:9.3e}", flush=True)
        for kind in KINDS:
            hip, tor = self.worst['hip'][kind], self.worst['torch'][kind]
            assert hip <= max(4.0 * tor, steps * 2.0 ** -24 * self.scale[kind]), (label, kind, hip, tor)


def _torch_route(params, beta1):
    tp = [torch.tensor(p, device='cuda').requires_grad_(True) for p in params]
    return tp, torch.optim.Adam(tp, lr=LR, betas=(beta1, B2), eps=EPS, fused=True)


def _ragged(beta1, views, errors=None, label=''):
    from wc_gan_amd.optim import ScheduledAdam
    numels = _ragged_numels()
    params, grads = _values(numels, STEPS, seed=3 + views)
    ref = AR.Adam64(params, LR, (beta1, B2), EPS, 'linear', TOTAL)
    tp, topt = _torch_route(params, beta1)
    errors = errors or _Errors()
    with Poison(0x7B) as P:
        hp = [P.guarded(p).requires_grad_(True) for p in params]
        if views:
            # every gradient a view at an ODD element offset of one flat buffer: 4-byte aligned and no more, as in a flat bucket
            offs, off = [], 1
            for n in numels:
                offs.append(off)
                off += n + (n % 2 == 1)
            flat = P.guarded(np.zeros(off + 1, dtype=np.float32))
            for p, o, n in zip(hp, offs, numels):
                assert (flat.data_ptr() + 4 * o) % 8 == 4
                p.grad = flat[o:o + n]
        opt = ScheduledAdam(hp, LR, (beta1, B2), EPS, schedule='linear', total_iters=TOTAL)
        assert opt.hip
        before = None
        for s in range(STEPS):
            for i, g in enumerate(grads[s]):
                if views:
                    hp[i].grad.copy_(torch.from_numpy(g))
                else:
                    hp[i].grad = P.guarded(g)          # a fresh gradient tensor every step, as eager autograd hands them out
                tp[i].grad = torch.tensor(g, device='cuda')
            topt.param_groups[0]['lr'] = LR * AR.multiplier('linear', s, TOTAL)
            topt.step()
            if s == STEPS - 1:
                before = ([p.detach().clone() for p in hp], opt.exp_avg_sq.clone())
            opt.step()
            ref.step(grads[s])
            assert len(opt._tables) == 2
            for i, p in enumerate(hp):
                errors.add('hip', 'param', p, ref.p[i]); errors.add('torch', 'param', tp[i], ref.p[i])
                errors.add('hip', 'exp_avg_sq', opt.state[p]['exp_avg_sq'], ref.v[i])
                errors.add('torch', 'exp_avg_sq', topt.state[tp[i]]['exp_avg_sq'], ref.v[i])
                if beta1:
                    errors.add('hip', 'exp_avg', opt.state[p]['exp_avg'], ref.m[i])
                    errors.add('torch', 'exp_avg', topt.state[tp[i]]['exp_avg'], ref.m[i])
                else:
                    assert 'exp_avg' not in opt.state[p]
        P.check_guards()
        errors.check(STEPS, label)
        # the fourth update ran at multiplier 0: the parameters keep their bits, the second moment moved
        assert all(same_bits(p.detach(), b) for p, b in zip(hp, before[0]))
        assert not torch.equal(opt.exp_avg_sq, before[1])
        assert int(opt.counter) == STEPS and opt.current_lr() == 0.0
        # the padding between the segments of the flat moment buffers is never written
        used = torch.zeros_like(opt.exp_avg_sq, dtype=torch.bool)
        for o, n in zip(opt._offsets, numels):
            used[o:o + n] = True
        assert not opt.exp_avg_sq[~used].any()
    return errors


@pytest.mark.gpu
@pytest.mark.parametrize('views', [0, 1], ids=['own-gradients', 'views-at-odd-offsets'])
@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_ragged_set_matches_the_reference(beta1, views):
    _ragged(beta1, views, label=f"ragged beta1={beta1} {'views' if views else 'own'}")


def _layout(contiguous_grad, errors=None, label=''):
    from wc_gan_amd.optim import ScheduledAdam
    rng = np.random.default_rng(11)
    w0 = rng.standard_normal((8, 4, 3, 3)).astype(np.float32)
    gs = [rng.standard_normal((8, 4, 3, 3)).astype(np.float32) for _ in range(2)]
    ref = AR.Adam64([w0], LR, (0.5, B2), EPS)
    tp, topt = _torch_route([w0], 0.5)
    errors = errors or _Errors()
    with Poison(0xFF) as P:
        w = torch.tensor(w0, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
        assert w.stride() == (36, 1, 12, 4)
        opt = ScheduledAdam([w], LR, (0.5, B2), EPS)
        for g in gs:
            gt = P.guarded(g)
            w.grad = gt if contiguous_grad else gt.contiguous(memory_format=torch.channels_last)
            assert (w.grad.stride() == w.stride()) == (not contiguous_grad)
            tp[0].grad = torch.tensor(g, device='cuda')
            opt.step(); topt.step(); ref.step([g])
            assert (0 in opt._restrided) == bool(contiguous_grad)
            errors.add('hip', 'param', w.detach().contiguous(), ref.p[0]); errors.add('torch', 'param', tp[0], ref.p[0])
            errors.add('hip', 'exp_avg_sq', opt.state[w]['exp_avg_sq'].contiguous(), ref.v[0])
            errors.add('torch', 'exp_avg_sq', topt.state[tp[0]]['exp_avg_sq'], ref.v[0])
            errors.add('hip', 'exp_avg', opt.state[w]['exp_avg'].contiguous(), ref.m[0])
            errors.add('torch', 'exp_avg', topt.state[tp[0]]['exp_avg'], ref.m[0])
        P.check_guards()
        errors.check(2, label)
    return errors


@pytest.mark.gpu
@pytest.mark.parametrize('contiguous_grad', [0, 1], ids=['matching-strides', 'host-restride'])
def test_channels_last_weight(contiguous_grad):
    _layout(contiguous_grad, label='channels-last ' + ('restrided' if contiguous_grad else 'matching'))


@pytest.mark.gpu
@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_zero_gradient_leaves_the_parameter_alone(beta1):
    from wc_gan_amd.optim import ScheduledAdam
    rng = np.random.default_rng(5)
    with Poison(0x7B) as P:
        vals = [rng.standard_normal(n).astype(np.float32) for n in (5, 2055)]
        vals[0][0] = -0.0
        ps = [P.guarded(v).requires_grad_(True) for v in vals]
        for p in ps:
            p.grad = P.guarded(np.zeros(p.numel(), dtype=np.float32))
        opt = ScheduledAdam(ps, LR, (beta1, B2), EPS)
        opt.step(); opt.step()
        P.check_guards()
        assert all(same_bits(p.detach().cpu(), torch.from_numpy(v)) for p, v in zip(ps, vals))
        assert not opt.exp_avg_sq.any() and int(opt.counter) == 2


@pytest.mark.gpu
def test_none_gradient_is_skipped_and_its_neighbours_are_not():
    from wc_gan_amd.optim import ScheduledAdam
    numels = [6, 2049, 3, 130]
    params, grads = _values(numels, 2, seed=9)
    ref = AR.Adam64(params, LR, (0.0, B2), EPS)
    with Poison(0x7B) as P:
        ps = [P.guarded(p).requires_grad_(True) for p in params]
        opt = ScheduledAdam(ps, LR, (0.0, B2), EPS)
        for s, skipped in enumerate((1, 2)):
            gs = [None if i == skipped else g for i, g in enumerate(grads[s])]
            for p, g in zip(ps, gs):
                p.grad = None if g is None else P.guarded(g)
            keep = (ps[skipped].detach().clone(), opt.state[ps[skipped]]['exp_avg_sq'].clone())
            opt.step(); ref.step(gs)
            assert same_bits(ps[skipped].detach(), keep[0]) and same_bits(opt.state[ps[skipped]]['exp_avg_sq'], keep[1])
            assert len(opt._tables) == 1 and opt._tables[0].count == 3
            # torch is no yardstick here (it keeps a counter per parameter, so a parameter that sat out a step has another bias
            # correction there): the bound is the floor itself -- one rounding of each stored value per step, 2^-24 relative at the
            # most -- plus, for the parameter, the fp32 arithmetic of the update: |update| <= lr / sqrt(1 - beta2) = 6.3e-4 times
            # ~8 roundings of 2^-24 each = 3e-10, taken as 1e-9.  exp_avg_sq is formed in float64 and rounded once.
            for i, p in enumerate(ps):
                floor = (s + 1) * 2.0 ** -24
                assert _err(p, ref.p[i]) <= floor * np.abs(ref.p[i]).max() + 1e-9, (s, i)
                assert _err(opt.state[p]['exp_avg_sq'], ref.v[i]) <= floor * np.abs(ref.v[i]).max(), (s, i)
        P.check_guards()
        assert int(opt.counter) == 2
        for p in ps:
            p.grad = None
        opt.step()                       # nothing to update: the counter alone moves
        assert int(opt.counter) == 3


@pytest.mark.gpu
@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_graph_replays_advance_the_device_counter(beta1):
    """one captured step() over static gradients, replayed three times == four eager steps, bit for bit, under 'linear' over 8 updates: the
    four updates run at four different rates, which a host-side rate baked into the capture would not give"""
    from wc_gan_amd.optim import ScheduledAdam
    numels = [5, 2049, 128, 1, 4103]
    params, grads = _values(numels, 1, seed=21)

    def make():
        ps = [torch.tensor(p, device='cuda').requires_grad_(True) for p in params]
        for p, g in zip(ps, grads[0]):
            p.grad = torch.tensor(g, device='cuda')
        return ps, ScheduledAdam(ps, LR, (beta1, B2), EPS, schedule='linear', total_iters=8)

    ps_e, opt_e = make()
    rates = []
    for _ in range(4):
        rates.append(opt_e.current_lr())
        opt_e.step()
    assert rates == [pytest.approx(LR * (1 - i / 8)) for i in range(4)]

    ps_g, opt_g = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt_g.step()                     # the eager first step: tables built, nothing left to allocate
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    torch.cuda.synchronize()
    assert int(opt_g.counter) == 1       # capturing ran nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(opt_g.counter) == 4 and int(opt_e.counter) == 4
    assert all(same_bits(a.detach(), b.detach()) for a, b in zip(ps_g, ps_e))
    assert same_bits(opt_g.exp_avg_sq, opt_e.exp_avg_sq)
    if beta1:
        assert same_bits(opt_g.exp_avg, opt_e.exp_avg)
    assert float(opt_g.record[3]) == pytest.approx(1 - 3 / 8) and opt_g.current_lr() == pytest.approx(LR * 0.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def _config():
    """the unconditional CIFAR-10 recipe at a sixteenth of its widths (the networks of test_layers_gpu.test_generator_step_runs_and_trains)"""
    from wc_gan_amd.train import CIFAR10_UNCOND
    cfg = dict(CIFAR10_UNCOND)
    cfg['generator'] = dict(cfg['generator'], block_sizes=(64, 64, 64), first_block_shape=(4, 4, 64))
    cfg['discriminator'] = dict(cfg['discriminator'], block_sizes=(32, 32, 32, 32))
    return cfg


BATCH = 8


def _trainer(**kw):
    from wc_gan_amd.train import build_trainer
    torch.manual_seed(4)
    return build_trainer(_config(), 'cuda', batch_size=BATCH, training_ratio=1, seed=7, **kw)


def _reals():
    g = torch.Generator().manual_seed(2)
    return [(torch.rand(BATCH, 32, 32, 3, generator=g) * 2 - 1).cuda()]


def _spy(tr):
    """(parameters before, gradients as the optimiser meets them) of both networks' updates"""
    seen = {}
    for name, opt, bucket in (('d', tr.opt_d, tr.d_bucket), ('g', tr.opt_g, tr.g_bucket)):
        def spy(step=opt.step, name=name, bucket=bucket):
            seen[name] = ([p.detach().clone() for p in bucket.params], [p.grad.detach().clone() for p in bucket.params])
            return step()
        opt.step = spy
    return seen


def _trainer_errors(errors=None, label='trainer, one step'):
    """each trainer's first step against the float64 reference applied to the gradients THAT trainer's optimiser met (the networks' gradient
    kernels need not repeat their bits from run to run; the optimisers are what is compared)"""
    errors = errors or _Errors()
    after = {}
    for route, kw in (('hip', dict(optimizer='hip')), ('torch', dict())):
        tr = _trainer(**kw)
        assert (type(tr.opt_d) is torch.optim.Adam) == (route == 'torch')
        seen = _spy(tr)
        d_loss, g_loss = tr.step(_reals())
        torch.cuda.synchronize()
        assert torch.isfinite(d_loss) and torch.isfinite(g_loss)
        after[route] = {}
        for name, bucket in (('d', tr.d_bucket), ('g', tr.g_bucket)):
            p0, gr = seen[name]
            ref = AR.Adam64([p.cpu().numpy().astype(np.float64) for p in p0], LR, (0.0, B2), EPS)
            ref.step([g.cpu().numpy().astype(np.float64) for g in gr])
            for i, p in enumerate(bucket.params):
                errors.add(route, 'param', p.detach().cpu().contiguous(), np.ascontiguousarray(ref.p[i]))
                opt = tr.opt_d if name == 'd' else tr.opt_g
                errors.add(route, 'exp_avg_sq', opt.state[p]['exp_avg_sq'].detach().cpu().contiguous(), np.ascontiguousarray(ref.v[i]))
            after[route][name] = ([p.detach().clone() for p in bucket.params], gr)
    errors.check(1, label)
    # where both runs met the same gradient bits, the two routes' parameters agree within the sum of their allowances
    bound = max(4.0 * errors.worst['torch']['param'], 2.0 ** -24 * errors.scale['param']) + errors.worst['torch']['param']
    for name in ('d', 'g'):
        (ph, gh), (pt, gt) = after['hip'][name], after['torch'][name]
        for a, b, x, y in zip(ph, pt, gh, gt):
            if same_bits(x, y):
                assert float((a - b).abs().max()) <= bound
    return errors


@pytest.mark.gpu
def test_trainer_hip_optimiser_agrees_with_the_default():
    _trainer_errors()


@pytest.mark.gpu
def test_trainer_schedule_reaches_zero_and_the_step_is_capturable():
    tr = _trainer(lr_decay_schedule='linear', schedule_iters=1)
    reals = _reals()
    tr.step(reals)
    first = [p.detach().clone() for p in list(tr.G.parameters()) + list(tr.D.parameters())]
    tr.step(reals)                       # both networks' second update: multiplier 0
    torch.cuda.synchronize()
    assert all(same_bits(p.detach(), b) for p, b in zip(list(tr.G.parameters()) + list(tr.D.parameters()), first))
    assert int(tr.opt_d.counter) == 2 and int(tr.opt_g.counter) == 2

    tr = _trainer(lr_decay_schedule='linear', schedule_iters=100)
    replay = tr.capture(reals)
    torch.cuda.synchronize()
    done = int(tr.opt_g.counter)         # the warm-up steps; recording the graph ran nothing
    assert done == int(tr.opt_d.counter) == 3
    before = [p.detach().clone() for p in tr.G.parameters()]
    d_loss, g_loss = replay()
    torch.cuda.synchronize()
    assert torch.isfinite(d_loss) and torch.isfinite(g_loss)
    assert int(tr.opt_g.counter) == done + 1 and int(tr.opt_d.counter) == done + 1
    assert tr.opt_g.current_lr() == pytest.approx(LR * (1 - (done + 1) / 100))
    assert any(not torch.equal(p.detach(), b) for p, b in zip(tr.G.parameters(), before))


if __name__ == '__main__':
    for beta1 in (0.0, 0.5):
        for views in (0, 1):
            _ragged(beta1, views, label=f"ragged beta1={beta1} {'views' if views else 'own'}")
    for c in (0, 1):
        _layout(c, label='channels-last ' + ('restrided' if c else 'matching'))
    _trainer_errors()
