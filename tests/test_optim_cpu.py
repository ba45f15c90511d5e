"""wc_gan_amd/optim.py on the CPU: the schedules' hand-derivable values, ScheduledAdam's torch-op path in float64 against the numpy
reference (tests/adam_reference.py), the host-side packing of the update launches, and the trainer's wiring."""
import itertools

import numpy as np
import pytest
import torch

import adam_reference as AR

LR, B2 = 2e-4, 0.9
SCHEDULES = [(None, None, 1), ('linear', 3, 1), ('half-linear', 4, 1), ('linear-end', 5, 1), ('dropat0', 6, 1), ('dropat1', 10000, 5)]


def _rel(a, ref):
    return float(np.abs(np.asarray(a) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _problem(seed=0, steps=5, shapes=((3, 5), (7,), (1,), (2, 3, 2))):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(s) for s in shapes]
    grads = [[rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2) for s in shapes] for _ in range(steps)]
    return params, grads


@pytest.mark.parametrize('beta1', [0.0, 0.5])
def test_the_reference_is_torch_adam_in_float64(beta1):
    params, grads = _problem()
    ref = AR.Adam64(params, LR, (beta1, B2))
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    opt = torch.optim.Adam(tp, lr=LR, betas=(beta1, B2))
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref.step(gs)
        for i, p in enumerate(tp):
            assert _rel(p.detach().numpy(), ref.p[i]) < 1e-12
            assert _rel(opt.state[p]['exp_avg_sq'].numpy(), ref.v[i]) < 1e-12
            assert _rel(opt.state[p]['exp_avg'].numpy(), ref.m[i]) < 1e-12


def test_lr_multiplier_hand_values():
    from wc_gan_amd.optim import lr_multiplier as f
    assert [f(None, it, None) for it in (0, 10 ** 9)] == [1.0, 1.0]
    assert [f('linear', it, 1000) for it in (0, 250, 1000, 1500)] == [1.0, 0.75, 0.0, 0.0]
    # dropat30, generator, 50 epochs: total 50000, the drop at 30000
    assert f('dropat30', 29999, 50000) == pytest.approx(1 - 29999 / 50000, rel=1e-15)
    assert f('dropat30', 30000, 50000) == pytest.approx(0.04, rel=1e-15)
    # ... the critic at training_ratio 5: total 250000, the drop at 150000
    assert f('dropat30', 149999, 250000, ratio=5) == pytest.approx(1 - 149999 / 250000, rel=1e-15)
    assert f('dropat30', 150000, 250000, ratio=5) == pytest.approx(0.1 * 0.4, rel=1e-15)
    assert [f('half-linear', it, 1000) for it in (499, 500, 900)] == [pytest.approx(0.501, rel=1e-15), 0.5, 0.5]
    assert f('linear-end', 828, 1000) == 1.0 and f('linear-end', 0, 1000) == 1.0 and f('linear-end', 1000, 1000) == 0.0
    assert f('linear-end', 914, 1000) == pytest.approx(0.5, rel=1e-12)
    assert f('linear-end', 2000, 1000) == 0.0
    with pytest.raises(ValueError):
        f('cosine', 0, 10)
    with pytest.raises(ValueError):
        f('linear', 0, 0)


@pytest.mark.parametrize('kind,total,ratio', SCHEDULES)
def test_lr_multiplier_is_the_references(kind, total, ratio):
    from wc_gan_amd.optim import lr_multiplier
    for it in range(0, 12):
        scale = 1 if total is None or total < 100 else 1000
        assert lr_multiplier(kind, it * scale, total, ratio) == pytest.approx(AR.multiplier(kind, it * scale, total, ratio), rel=1e-14, abs=1e-300)


@pytest.mark.parametrize('beta1', [0.0, 0.5])
@pytest.mark.parametrize('kind,total,ratio', SCHEDULES)
def test_scheduled_adam_float64_matches_the_reference(kind, total, ratio, beta1):
    """every kind, with a parameter whose gradient is None at two of the steps and a state_dict round trip in the middle of the run"""
    from wc_gan_amd.optim import ScheduledAdam
    params, grads = _problem(seed=1, steps=7)
    grads[1][2] = None
    grads[4][0] = None
    if kind == 'dropat1':           # cross the drop (5000 updates at ratio 5) inside the run
        start = 4997
    else:
        start = 0
    ref = AR.Adam64(params, LR, (beta1, B2), schedule=kind, total_iters=total, ratio=ratio)
    ref.t = start

    def make():
        tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
        return tp, ScheduledAdam(tp, LR, (beta1, B2), schedule=kind, total_iters=total, ratio=ratio)

    tp, opt = make()
    opt.counter.fill_(start)
    assert not opt.hip
    for s, gs in enumerate(grads):
        if s == 3:                  # resume: a fresh optimiser over the current parameters, loaded from the old one's state
            sd = opt.state_dict()
            cur = [p.detach().clone() for p in tp]
            tp, opt = make()
            with torch.no_grad():
                for p, c in zip(tp, cur):
                    p.copy_(c)
            opt.load_state_dict(sd)
        assert opt.current_lr() == pytest.approx(ref.rate(), rel=1e-14, abs=1e-300)
        for p, g in zip(tp, gs):
            p.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        opt.step()
        ref.step(gs)
        assert int(opt.counter) == ref.t
        for i, p in enumerate(tp):
            assert _rel(p.detach().numpy(), ref.p[i]) < 1e-12, (s, i)
            assert _rel(opt.state[p]['exp_avg_sq'].numpy(), ref.v[i]) < 1e-12 or not ref.v[i].any(), (s, i)
            assert ('exp_avg' in opt.state[p]) == (beta1 != 0.0)
            if beta1:
                assert _rel(opt.state[p]['exp_avg'].numpy(), ref.m[i]) < 1e-12 or not ref.m[i].any(), (s, i)
            assert opt.state[p]['step'] is opt.counter


def test_scheduled_adam_layouts_and_refusals():
    from wc_gan_amd.optim import ScheduledAdam
    w = torch.randn(8, 4, 3, 3, dtype=torch.float64).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ref = AR.Adam64([w.detach().numpy()], LR, (0.5, B2))
    opt = ScheduledAdam([w], LR, (0.5, B2))
    assert opt.state[w]['exp_avg_sq'].stride() == w.stride()
    g = torch.randn(8, 4, 3, 3, dtype=torch.float64)          # contiguous: other strides than the parameter's
    w.grad = g
    opt.step()
    ref.step([g.numpy()])
    assert _rel(w.detach().numpy(), ref.p[0]) < 1e-12 and _rel(opt.state[w]['exp_avg_sq'].numpy(), ref.v[0]) < 1e-12
    with pytest.raises(ValueError, match='dense'):
        ScheduledAdam([torch.zeros(4, 6)[:, ::2].requires_grad_(True)], LR, (0.0, B2))
    with pytest.raises(ValueError, match='total_iters'):
        ScheduledAdam([torch.zeros(4, requires_grad=True)], LR, (0.0, B2), schedule='linear')
    with pytest.raises(ValueError):
        ScheduledAdam([torch.zeros(4, requires_grad=True)], LR, (0.0, B2), schedule='cosine', total_iters=5)


def test_pack_covers_every_element_exactly_once():
    from wc_gan_amd.optim import _pack
    c, cap = 8, 5
    sizes = [1, 3, c - 1, c, c + 1, 2 * c + 7]
    cases = [list(p) for r in range(1, 4) for p in itertools.product(sizes, repeat=r)]
    cases += [sizes, sizes[::-1], [1] * (cap - 1), [1] * cap, [1] * (cap + 1), sizes + [1] * cap, [1] * (2 * cap + 1)]
    for numels in cases:
        launches = _pack(numels, c, cap)
        seen = [np.zeros(n, dtype=np.int64) for n in numels]
        for idx, start in launches:
            assert 1 <= len(idx) <= cap and len(start) == len(idx) + 1 and start[0] == 0
            for wg in range(start[-1]):               # what a workgroup of the kernel does with the table
                j = max(k for k in range(len(idx)) if start[k] <= wg)
                assert wg < start[j + 1]
                n = numels[idx[j]]
                begin = (wg - start[j]) * c
                assert begin < n, "a workgroup without work"
                seen[idx[j]][begin:min(n, begin + c)] += 1
        assert all((s == 1).all() for s in seen), numels
        assert sorted(i for idx, _ in launches for i in idx) == list(range(len(numels)))
    assert _pack([], c, cap) == []
    with pytest.raises(ValueError):
        _pack([4, 0], c, cap)


def test_binding_table_matches_the_header():
    import ctypes
    import os
    import re
    from wc_gan_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'wc_hip.h')).read()
    assert int(re.search(r'#define WC_ADAM_CAPACITY (\d+)', src).group(1)) == _lib.ADAM_CAPACITY
    cap = _lib.ADAM_CAPACITY
    assert ctypes.sizeof(_lib.AdamTable) == cap * (8 + 8 + 8 + 4) + (cap + 1) * 4 + 8 + 4       # (+ 4: padded to the pointers' alignment)
    assert ctypes.sizeof(_lib.AdamTable) + 64 <= 4096, "the by-value table and the other arguments fit the 4 KiB kernel-argument segment"


def test_update_entry_checks_its_table_without_touching_the_gpu():
    import ctypes
    from wc_gan_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    lib = _lib.load()
    assert lib.wc_adam_capacity() == _lib.ADAM_CAPACITY
    one = ctypes.c_void_p(1 << 20)

    def table(numel=10, chunks=1, off=0, chunk=2048, count=1):
        t = _lib.AdamTable()
        t.param[0], t.grad[0], t.moment_off[0], t.numel[0] = 1 << 20, 1 << 21, off, numel
        t.chunk_start[1] = chunks
        t.count, t.chunk = count, chunk
        return ctypes.byref(t)
    call = lambda t, m=None, elems=12, b1=0.0: lib.wc_adam_update_f32(t, m, one, elems, one, b1, 0.9, 1e-8, None)
    assert call(None) == -1
    assert call(table(), b1=0.5) == -1                          # beta1 != 0 needs exp_avg
    assert call(table(chunks=2)) == -2                          # more workgroups than ceil(numel / chunk)
    assert call(table(numel=4097, chunks=2)) == -2              # ... or fewer: 4097 elements are three chunks
    assert call(table(off=4)) == -2                             # the segment ends beyond the moment buffer
    assert call(table(off=2)) == -2                             # segment offsets are multiples of four
    assert call(table(chunk=1000)) == -5 and call(table(count=0)) == -5 and call(table(count=_lib.ADAM_CAPACITY + 1)) == -5
    assert lib.wc_adam_tick(None, one, 1e-3, 0.0, 0.9, 0, 0.0, 0.0, None) == -1
    assert lib.wc_adam_tick(one, one, 1e-3, 0.0, 0.9, 1, 0.0, 0.0, None) == -5          # a schedule without its total
    assert lib.wc_adam_tick(one, one, 1e-3, 0.0, 1.0, 0, 0.0, 0.0, None) == -5
    assert lib.wc_adam_tick(one, one, 1e-3, 0.0, 0.9, 5, 10.0, 0.0, None) == -5


def _cpu_trainer(**kw):
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import GanTrainer
    torch.manual_seed(0)
    G = make_generator(block_sizes=(8,), resamples=("UP",), first_block_shape=(4, 4, 8), block_norm='b', block_after_norm='ucs',
                       last_norm='b', last_after_norm='ucs')
    D = make_discriminator(input_image_shape=(8, 8, 3), block_sizes=(8, 8), resamples=('DOWN', 'SAME'), type=None, spectral=False,
                           sum_pool=True)
    with torch.no_grad():
        G(torch.zeros(2, 128), torch.zeros(2, 1, dtype=torch.int32))
    return GanTrainer(G, D, batch_size=2, training_ratio=2, **kw)


def test_trainer_counts_each_networks_updates_and_uses_its_rate():
    from wc_gan_amd.optim import ScheduledAdam
    tr = _cpu_trainer(lr_decay_schedule='linear', schedule_iters=4, generator_lr=3e-4, discriminator_lr=5e-4)
    assert type(tr.opt_d) is ScheduledAdam and type(tr.opt_g) is ScheduledAdam
    assert (tr.opt_g.total_iters, tr.opt_d.total_iters) == (4.0, 8.0) and (tr.opt_g.lr, tr.opt_d.lr) == (3e-4, 5e-4)
    assert (tr.opt_g.ratio, tr.opt_d.ratio) == (1, 2)
    reals = [torch.rand(2, 8, 8, 3) * 2 - 1 for _ in range(2)]
    d_loss, g_loss = tr.step(reals)
    assert torch.isfinite(d_loss) and torch.isfinite(g_loss)
    assert int(tr.opt_d.counter) == 2 and int(tr.opt_g.counter) == 1
    assert tr.opt_d.current_lr() == pytest.approx(5e-4 * (1 - 2 / 8)) and tr.opt_g.current_lr() == pytest.approx(3e-4 * (1 - 1 / 4))
    # the first update of a fresh run with beta1 = 0 moves every weight with a non-zero gradient by rate x g / (|g| + eps): the rate is visible
    tr = _cpu_trainer(lr_decay_schedule='linear', schedule_iters=4, generator_lr=3e-4, discriminator_lr=5e-4)
    before = [p.detach().clone() for p in tr.d_bucket.params]
    tr.d_step(reals[0])
    moved = torch.cat([(p.detach() - b).abs().reshape(-1) for p, b in zip(tr.d_bucket.params, before)])
    assert float(moved.max()) == pytest.approx(5e-4, rel=1e-3)
    before = [p.detach().clone() for p in tr.g_bucket.params]
    tr.g_step()
    moved = torch.cat([(p.detach() - b).abs().reshape(-1) for p, b in zip(tr.g_bucket.params, before)])
    assert float(moved.max()) == pytest.approx(3e-4, rel=1e-3)


def test_trainer_epochs_give_the_totals_and_hip_is_opt_in():
    from wc_gan_amd.optim import ScheduledAdam
    tr = _cpu_trainer(lr_decay_schedule='dropat30', number_of_epochs=50)
    assert (tr.opt_g.total_iters, tr.opt_d.total_iters) == (50000.0, 100000.0)
    assert tr.opt_g.current_lr() == 2e-4
    tr = _cpu_trainer(optimizer='hip')
    assert type(tr.opt_g) is ScheduledAdam and tr.opt_g.schedule is None
    with pytest.raises(ValueError):
        _cpu_trainer(lr_decay_schedule='linear')
    with pytest.raises(ValueError):
        _cpu_trainer(optimizer='sgd')


def test_default_trainer_keeps_torch_adam():
    tr = _cpu_trainer()
    assert type(tr.opt_d) is torch.optim.Adam and type(tr.opt_g) is torch.optim.Adam
    assert tr.opt_d.param_groups[0]['lr'] == 2e-4 and tr.opt_d.param_groups[0]['betas'] == (0.0, 0.9)


def test_recipe_schedules_name_the_recipes():
    from wc_gan_amd import optim, train
    names = set(train.CONFIGS) | set(train.DCGAN_CONFIGS) | set(train.WGAN_CONFIGS)
    assert set(train.RECIPE_SCHEDULES) == names and len(names) == 7
    for name, kw in train.RECIPE_SCHEDULES.items():
        assert set(kw) == {'lr_decay_schedule', 'number_of_epochs'}
        optim.parse_schedule(kw['lr_decay_schedule'])
        assert kw['number_of_epochs'] > 0
    assert train.RECIPE_SCHEDULES['cifar10_cond']['lr_decay_schedule'] == 'dropat30'
