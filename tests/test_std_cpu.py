"""CPU tests of the fused batch-norm site (norm 'b' on the HIP route): the float64 reference itself (tests/std_reference.py), its
committed fixture, the C ABI's argument checks and the wiring through create_norm / make_generator / checkpoint / train.  No kernel
is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import std_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wc_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "std_golden.npz")

STD_SYMBOLS = ["wc_std_stats_workspace_bytes", "wc_std_stats_f32", "wc_std_factor_f64", "wc_std_apply_f32",
               "wc_std_bwd_reduce_workspace_bytes", "wc_std_bwd_reduce_f32", "wc_std_bwd_factor_f64", "wc_std_bwd_apply_f32"]


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _inputs(rng, N=12, H=5, W=7, C=32, K=4):
    scale = 10.0 ** rng.uniform(-2.0, 2.0, C)                # channel scales over four decades
    x = rng.standard_normal((N, H, W, C)) * scale + 3.0 * scale * rng.standard_normal(C)       # offsets of 3 (sigma)
    gamma = 1.0 + 0.5 * rng.standard_normal((K, C))
    beta = 0.3 * rng.standard_normal((K, C))
    slot = rng.integers(0, K, N)
    gy = rng.standard_normal((N, H, W, C))
    return x, gamma, beta, slot, gy


@pytest.mark.parametrize("conditional", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_closed_form_backward_equals_float64_autograd(conditional, relu):
    """The closed form against torch float64 autograd through (x - mean) / sqrt(var + eps) * gamma[slot] + beta[slot] (+ relu), at 1e-9
    relative (float64 against float64: the bound tests/test_k5_algebra.py uses for algebra)."""
    rng = np.random.default_rng(5 + 2 * conditional + relu)
    x, gamma, beta, slot, gy = _inputs(rng)
    if not conditional:
        gamma, beta, slot = gamma[:1], beta[:1], None
    eps = 1e-3
    y, cache = R.forward(x, gamma, beta, slot, eps=eps, relu=relu)
    dx, dgamma, dbeta = R.backward(gy, cache)

    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    gt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    idx = torch.zeros(x.shape[0], dtype=torch.long) if slot is None else torch.tensor(slot, dtype=torch.long)
    mean = xt.mean((0, 1, 2))
    var = ((xt - mean) ** 2).mean((0, 1, 2))
    yt = (xt - mean) / torch.sqrt(var + eps) * gt[idx][:, None, None, :] + bt[idx][:, None, None, :]
    if relu:
        yt = torch.relu(yt)
    yt.backward(torch.tensor(gy, dtype=torch.float64))
    errs = dict(y=R.rel(y, yt.detach().numpy()), dx=R.rel(dx, xt.grad.numpy()), dgamma=R.rel(dgamma, gt.grad.numpy()),
                dbeta=R.rel(dbeta, bt.grad.numpy()))
    print(errs)
    assert all(v < 1e-9 for v in errs.values()), errs


def test_reference_modes_are_consistent():
    """Groups equal separate calls (outputs and the moving statistics after them); evaluation mode with the statistics a training call
    would normalise with reproduces that call; ddof changes the moving variance by M / (M - 1) and nothing else."""
    rng = np.random.default_rng(11)
    x, gamma, beta, slot, _ = _inputs(rng, N=12)
    C = x.shape[-1]
    mm, mv = 0.1 * rng.standard_normal(C), 1.0 + rng.random(C)
    y, c = R.forward(x, gamma, beta, slot, mm, mv, True, relu=True, groups=3)
    m, v = mm, mv
    for g in range(3):
        sl = slice(4 * g, 4 * g + 4)
        yg, cg = R.forward(x[sl], gamma, beta, slot[sl], m, v, True, relu=True)
        m, v = cg['moving_mean'], cg['moving_variance']
        assert np.array_equal(yg, y[sl]) and np.array_equal(cg['mu'][0], c['mu'][g])
    assert np.array_equal(m, c['moving_mean']) and np.array_equal(v, c['moving_variance'])
    y1, c1 = R.forward(x, gamma, beta, slot, mm, mv, True, ddof=0)
    y2, c2 = R.forward(x, gamma, beta, slot, mm, mv, True, ddof=1)
    M = x.size // C
    assert np.array_equal(y1, y2) and np.array_equal(c1['moving_mean'], c2['moving_mean'])
    batch_var = 1.0 / c1['w'][0] ** 2 - 1e-3
    assert np.allclose(c1['moving_variance'], 0.99 * mv + 0.01 * batch_var, rtol=1e-9, atol=0)
    assert np.allclose(c2['moving_variance'], 0.99 * mv + 0.01 * batch_var * M / (M - 1), rtol=1e-9, atol=0)
    ye, _ = R.forward(x, gamma, beta, slot, c1['mu'][0], batch_var, False)
    assert R.rel(ye, y1) < 1e-12


def test_golden_fixture_reproduces():
    """tests/golden/std_golden.npz is what tests/golden/make_golden_std.py writes from the reference today."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_std", os.path.join(ROOT, "tests", "golden", "make_golden_std.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.cases()
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(fresh)
    for k in gold.files:
        a, b = gold[k], np.asarray(fresh[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind == 'f' and a.dtype.itemsize == 8:
            assert R.rel(b, a) < 1e-12, k               # (float64 sums: numpy's pairwise order may differ between builds)
        else:
            assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported(lib):
    from wc_gan_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", src))
    for name in STD_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    core = re.search(r'#define WC_CORE_API((?:\s*"[^"]*"\s*\\?\n?)+)', open(HEADER).read()).group(1)
    assert "wc_std_" not in core                                    # a second norm, not part of the WC boundary
    assert lib.wc_abi_version() == 8


def test_argument_checks_return_codes_without_a_launch(lib):
    one = ctypes.c_void_p(16)       # never dereferenced: every call below is rejected first
    big = 1 << 30
    st = lambda x=one, M=64, C=64, ws=big: lib.wc_std_stats_f32(x, M, C, 1, one, one, one, ws, None)
    assert (st(x=None), st(M=0), st(C=40), st(ws=16)) == (-1, -2, -3, -4)
    assert lib.wc_std_stats_f32(one, 64, 64, 3, one, one, one, big, None) == -2                 # M % groups
    fa = lambda mu=one, M=64, C=64, eps=1e-3, mom=0.99, ddof=0, tr=1: lib.wc_std_factor_f64(
        one, one, M, C, 1, eps, mom, ddof, tr, None, None, None, None, 1, mu, one, one, one, None)
    assert (fa(mu=None), fa(M=0), fa(C=40), fa(eps=0.0), fa(mom=1.5), fa(ddof=2)) == (-1, -2, -3, -5, -5, -5)
    assert fa(M=1, ddof=1) == -2 and fa(tr=0) == -1                                              # evaluation mode needs the moving statistics
    ap = lambda x=one, N=4, C=64, relu=1: lib.wc_std_apply_f32(x, one, one, None, N, 16, C, 1, relu, one, None)
    assert (ap(x=None), ap(N=0), ap(C=40), ap(relu=2)) == (-1, -2, -3, -5)
    assert lib.wc_std_apply_f32(one, one, one, None, 1 << 20, 1 << 20, 64, 1, 0, one, None) == -2       # 2^31 rows and more
    br = lambda x=one, N=4, C=64, ws=big, Kc=1: lib.wc_std_bwd_reduce_f32(x, one, one, one, None, N, 16, C, Kc, 1, one, one, one, ws, None)
    assert (br(x=None), br(N=0), br(C=40), br(ws=16), br(Kc=0)) == (-1, -2, -3, -4, -2)
    assert lib.wc_std_bwd_reduce_f32(one, one, None, None, None, 4, 16, 64, 1, 1, one, one, one, big, None) == -1   # relu needs the tables
    bf = lambda q=one, M=64, C=64: lib.wc_std_bwd_factor_f64(one, one, one, one, None, M, C, 1, 1, None, None, q, one, None)
    assert (bf(q=None), bf(M=0), bf(C=40)) == (-1, -2, -3)
    ba = lambda dx=one, N=4, C=64, relu=0: lib.wc_std_bwd_apply_f32(one, one, one, one, one, one, None, N, 16, C, 1, relu, dx, None)
    assert (ba(dx=None), ba(N=0), ba(C=40), ba(relu=3)) == (-1, -2, -3, -5)


def test_sizers(lib):
    assert lib.wc_std_stats_workspace_bytes(131072, 256, 1) >= 2 * 256 * 8
    assert lib.wc_std_stats_workspace_bytes(0, 256, 1) == 0 and lib.wc_std_stats_workspace_bytes(64, 40, 1) == 0
    assert lib.wc_std_stats_workspace_bytes(64, 64, 3) == 0
    # a group's slabs do not depend on how many groups ride along (the grouped call equals separate calls bit for bit)
    assert lib.wc_std_stats_workspace_bytes(5 * 65536, 256, 5) == 5 * lib.wc_std_stats_workspace_bytes(65536, 256, 1)
    assert lib.wc_std_bwd_reduce_workspace_bytes(128, 1024, 256, 10) >= 128 * 2 * 256 * 8
    assert lib.wc_std_bwd_reduce_workspace_bytes(64, 36, 256, 1) > 0                             # the STL-10 6x6 site
    assert lib.wc_std_bwd_reduce_workspace_bytes(0, 16, 64, 1) == 0 and lib.wc_std_bwd_reduce_workspace_bytes(4, 16, 48, 1) == 0
    assert lib.wc_std_bwd_reduce_workspace_bytes(4, 16, 64, 0) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# wiring
# ---------------------------------------------------------------------------------------------------------------------------------
def _sub_names(stack):
    return sorted(m.layer_name for m in stack.modules() if getattr(m, 'layer_name', None))


def test_create_norm_wiring_for_every_after_norm():
    from wc_gan_amd import layers
    from wc_gan_amd.generator import AFTER_NORMS, NORMS, _UnfusedStack, create_norm
    assert NORMS == ['n', 'b', 'd', 'dr'] and len(AFTER_NORMS) == 10
    for an in AFTER_NORMS:
        fused = create_norm('b', an, number_of_classes=7, fused_batch_norm=True)(axis=-1, name='G.0.bn1', channels=64)
        plain = create_norm('b', an, number_of_classes=7)(axis=-1, name='G.0.bn1', channels=64)
        assert type(fused) is layers.StandardizeColoring, an
        assert type(plain) is _UnfusedStack, an
        assert type(fused.npart) is layers.BatchStandardization and fused.npart.layer_name == 'G.0.bn1_npart'
        assert _sub_names(fused) == _sub_names(plain), an            # the reference's sub-layer names (generator.py:85-86, 36-38, 55-58)
        assert fused.diagonal == (an in ('ucs', 'ccs', 'uccs', 'n')), an
        assert fused.npart.moving_mean.shape == (64,) and float(fused.npart.moving_variance.min()) == 1.0
        assert fused.npart.ddof == 0 and fused.npart.epsilon == 1e-3 and fused.npart.momentum == 0.99
    # the keyword changes nothing for the other norms
    assert type(create_norm('d', 'uconv', fused_batch_norm=True)(-1, 'x', 64)) is layers.WhiteningColoring
    assert type(create_norm('n', 'ucs', fused_batch_norm=True)(-1, 'x', 64)) is _UnfusedStack


def test_coloring_vectors_add_without_a_square_table():
    from wc_gan_amd.generator import create_norm
    st = create_norm('b', 'uccs', number_of_classes=5, fused_batch_norm=True)(axis=-1, name='s', channels=32)
    with torch.no_grad():
        for p in st.parameters():
            p.copy_(torch.randn_like(p))
    cls = torch.tensor([[3], [0], [4]])
    gamma, beta, slot = st.coloring_vectors(torch.zeros(3, 2, 2, 32), cls)
    cond, unc = st.branches
    assert gamma.shape == (5, 32) and beta.shape == (5, 32) and slot.tolist() == [3, 0, 4] and slot.dtype == torch.int32
    assert torch.equal(gamma, cond.gamma + unc.gamma) and torch.equal(beta, cond.beta + unc.beta)
    none = create_norm('b', 'n', fused_batch_norm=True)(axis=-1, name='s', channels=32)
    assert none.coloring_vectors(torch.zeros(3, 2, 2, 32), None) == (None, None, None)


def test_supports_statistic_groups():
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.layers import supports_statistic_groups
    from wc_gan_amd.train import CONFIGS, baseline_config
    kw = baseline_config(CONFIGS['cifar10_uncond'])['generator']
    assert supports_statistic_groups(make_generator(**kw))
    assert not supports_statistic_groups(make_generator(**dict(kw, fused_batch_norm=False)))
    narrow = dict(kw, block_sizes=(48, 48, 48), first_block_shape=(4, 4, 48))       # a width the HIP route does not take
    assert not supports_statistic_groups(make_generator(**narrow))


def test_checkpoint_keys_are_those_of_the_unfused_generator_and_load_both_ways():
    from wc_gan_amd.checkpoint import keras_named_state, load_keras_named
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import CONFIGS, baseline_config
    kw = dict(baseline_config(CONFIGS['cifar10_cond'], after_norm='ccs')['generator'], block_sizes=(32, 32), resamples=("UP", "UP"),
              first_block_shape=(4, 4, 32))
    torch.manual_seed(0)
    fused = make_generator(**kw)
    plain = make_generator(**dict(kw, fused_batch_norm=False))
    z, cls = torch.randn(4, 128), torch.randint(0, 10, (4, 1))
    plain(z, cls)                                  # torch's route builds its BatchNorm2d on the first call (CPU: it has no HIP kernel)
    with torch.no_grad():
        for m in fused.modules():
            if hasattr(m, 'moving_variance'):
                m.moving_mean.normal_(); m.moving_variance.uniform_(0.5, 2.0)
    sf, sp = keras_named_state(fused), keras_named_state(plain)
    assert sorted(sf) == sorted(sp)
    assert 'Generator.0.bn1_npart/moving_variance:0' in sf and sf['Generator.0.bn1_npart/moving_mean:0'].shape == (32,)
    load_keras_named(plain, sf)
    back = keras_named_state(plain)
    assert all(np.array_equal(sf[k], back[k]) for k in sf)
    with torch.no_grad():
        for m in fused.modules():
            if hasattr(m, 'moving_variance'):
                m.moving_mean.zero_(); m.moving_variance.fill_(1.0)
    load_keras_named(fused, back)
    again = keras_named_state(fused)
    assert all(np.array_equal(sf[k], again[k]) for k in sf)


def test_baseline_config_leaves_configs_untouched():
    import copy
    from wc_gan_amd.train import CONFIGS, baseline_config
    before = copy.deepcopy(CONFIGS)
    b = baseline_config(CONFIGS['cifar10_uncond'])
    g = b['generator']
    assert (g['block_norm'], g['last_norm'], g['block_after_norm'], g['last_after_norm'], g['fused_batch_norm']) == ('b', 'b', 'ucs', 'ucs', True)
    c = baseline_config(CONFIGS['cifar10_cond'], after_norm='ccs', fused=False)['generator']
    assert c['block_after_norm'] == c['last_after_norm'] == 'ccs' and c['fused_batch_norm'] is False
    g['block_sizes'] = (1,)
    assert CONFIGS == before and sorted(CONFIGS) == ['cifar10_cond', 'cifar10_uncond', 'stl10_uncond', 'tinyimagenet_cond_sa']
    assert 'fused_batch_norm' not in CONFIGS['cifar10_uncond']['generator']
    assert b['discriminator'] == CONFIGS['cifar10_uncond']['discriminator']


def test_cpu_tensors_and_odd_widths_raise_with_the_layers_name():
    from wc_gan_amd import _lib, ops
    from wc_gan_amd.generator import create_norm
    st = create_norm('b', 'ucs', fused_batch_norm=True)(axis=-1, name='Generator.0.bn1', channels=64)
    with pytest.raises(_lib.WcHipError, match='Generator.0.bn1_npart'):
        st(torch.zeros(2, 4, 4, 64), None, relu=True)
    with pytest.raises(_lib.WcHipError):
        ops.std_stats(torch.zeros(64, 32))
    with pytest.raises(_lib.WcHipError):
        ops.std_apply(torch.zeros(2, 4, 4, 32), torch.zeros(1, 32), torch.zeros(1, 32))
    # without the keyword 'b' keeps running on the CPU
    plain = create_norm('b', 'ucs')(axis=-1, name='p', channels=64)
    assert plain(torch.randn(2, 4, 4, 64), None).shape == (2, 4, 4, 64)
