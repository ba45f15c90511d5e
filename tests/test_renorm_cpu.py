"""CPU tests of the renorm ('dr') route: the closed form K5 runs against the oracle's renorm backward in float64 numpy, the
new entry points' declarations, sizers and argument checks (no launch), and the host surface (train.renorm_config, takes_split)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import wc_oracle as o
import renorm_reference as rr

EPS = 1e-3
NEW = ("wc_renorm_supported", "wc_renorm_f64", "wc_bwd_factor_renorm_f64")
SIZERS = ("wc_renorm_workspace_bytes", "wc_bwd_factor_renorm_workspace_bytes")


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# (shape, Kc): the issue's three; the last has fewer rows (16) than channels (64)
@pytest.mark.parametrize("shape,Kc", [((6, 4, 4, 32), 3), ((16, 2, 2, 96), 1), ((4, 2, 2, 64), 2)])
def test_closed_form_equals_the_oracles_renorm_backward(shape, Kc):
    rng = np.random.default_rng(shape[-1] + Kc)
    N, C = shape[0], shape[-1]
    M = int(np.prod(shape[:-1]))
    x = o.synth_activation(rng, shape, 'ill')
    ref = 0.7 * o.synth_activation(rng, (8 * C, C), 'ill') - 0.1
    mm, mc = o.moments_to_stats(*o.batch_moments(ref))
    gamma = rng.standard_normal((Kc, C, C)) / np.sqrt(C)
    beta = rng.standard_normal((Kc, C))
    slot = rng.integers(0, Kc, N) if Kc > 1 else None
    gy = rng.standard_normal(shape)
    y_ref, cache = o.wc_forward_renorm(x, gamma, beta, slot, moving_mean=mm, moving_cov=mc, eps=EPS)
    dx_ref, dG_ref, dB_ref = o.wc_backward_renorm(gy, cache)

    # the route: K2's (L, W) of the batch, the moving factor from the statistics BEFORE the update, the coloring with W_m
    L, W, f = cache['L'], cache['W'], cache['f']
    _, Wm = o.whitening_matrix(mc, EPS)
    C0 = Wm @ L
    assert np.abs(np.triu(C0, 1)).max() == 0.0
    A = np.einsum('ji,kjo->kio', Wm, gamma)                         # A_k = W_m^T Gamma_k: no C0 in the forward
    rows = cache['row_slot']
    y = np.einsum('mc,mco->mo', f, A[rows]) + beta[rows]
    g = gy.reshape(M, C)
    R = np.stack([f[rows == k].T @ g[rows == k] for k in range(Kc)])
    gsum = np.stack([g[rows == k].sum(0) for k in range(Kc)])
    dgamma, dbeta, S, gmean = rr.factor_backward(R, gsum, W, Wm, C0, gamma, A, M, EPS)
    dx = np.einsum('mo,mco->mc', g, A[rows]) + f @ S - gmean       # K6, unchanged
    errs = dict(y=rel(y.reshape(shape), y_ref), dx=rel(dx.reshape(shape), dx_ref), dG=rel(dgamma, dG_ref), dB=rel(dbeta, dB_ref))
    print(shape, Kc, errs)
    assert all(v <= 1e-12 for v in errs.values()), errs


def test_header_and_binding_table_declare_the_new_symbols():
    from wc_gan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "wc_hip.h")).read()
    for name in NEW + SIZERS:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    core = header[header.index("WC_CORE_API"):]
    core = core[:core.index("\n\n")]
    assert not any(name in core for name in NEW + SIZERS)           # additive entries: the core list stays as it is
    ret, args = _lib.SIGNATURES["wc_renorm_f64"]
    assert ret is ctypes.c_int and len(args) == 9 and args[2] is ctypes.c_int and args[3] is ctypes.c_double
    assert len(_lib.SIGNATURES["wc_bwd_factor_renorm_f64"][1]) == 20


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_new_entry_points_are_exported_and_sized(lib):
    for name in NEW + SIZERS:
        assert hasattr(lib, name), name
    assert [C for C in range(0, 1100, 8) if lib.wc_renorm_supported(C)] == list(range(32, 1025, 32))      # K2's widths
    for C in (32, 96, 256, 288, 1024):
        assert lib.wc_renorm_workspace_bytes(C) >= 2 * C * C * 8
        assert lib.wc_renorm_workspace_bytes(C) >= lib.wc_factor_workspace_bytes(C, 1) + C * C * 8       # L_m and K2's own scratch
    assert lib.wc_renorm_workspace_bytes(40) == 0 and lib.wc_renorm_workspace_bytes(1056) == 0
    assert lib.wc_bwd_factor_renorm_workspace_bytes(128, 3) == lib.wc_bwd_factor_workspace_bytes(128, 3) >= 3 * 128 * 128 * 8
    assert lib.wc_bwd_factor_renorm_workspace_bytes(40, 1) == 0 and lib.wc_bwd_factor_renorm_workspace_bytes(1056, 1) == 0


def test_new_entry_points_reject_bad_arguments_without_a_launch(lib):
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is rejected first
    big = 1 << 30

    def rn(mc=one, L=one, C=64, eps=EPS, Wm=one, C0=one, ws=one, nb=big):
        return lib.wc_renorm_f64(mc, L, C, eps, Wm, C0, ws, nb, None)

    assert rn(Wm=None) == -1 and rn(ws=None) == -1
    assert rn(mc=None, L=None) == -1            # neither phase asked for
    assert rn(C0=None) == -1                    # the product needs its output
    assert rn(C=40) == -3 and rn(C=1056) == -3 and rn(C=0) == -3
    assert rn(eps=0.0) == -5 and rn(eps=1.0) == -5
    assert rn(nb=lib.wc_renorm_workspace_bytes(64) - 1) == -4

    def k5(R=one, gsum=one, W=one, Wm=one, C0=one, gamma=one, A=one, Kc=1, C=64, M=100, eps=EPS, ddof=1, training=1,
           S=one, gmean=one, ws=one, nb=big):
        return lib.wc_bwd_factor_renorm_f64(R, gsum, W, Wm, C0, gamma, A, Kc, C, M, eps, ddof, training, one, one, S, gmean, ws, nb, None)

    assert k5(R=None) == -1 and k5(gsum=None) == -1 and k5(Wm=None) == -1 and k5(ws=None) == -1
    assert k5(W=None) == -1 and k5(C0=None) == -1 and k5(A=None) == -1 and k5(S=None) == -1 and k5(gmean=None) == -1
    assert k5(C=40) == -3 and k5(C=1056) == -3
    assert k5(Kc=0) == -2 and k5(gamma=None, Kc=2) == -2 and k5(M=1) == -2
    assert k5(eps=1.0) == -5 and k5(eps=0.0) == -5 and k5(ddof=2) == -5
    assert k5(nb=lib.wc_bwd_factor_renorm_workspace_bytes(64, 1) - 1) == -4


def test_renorm_config_sets_both_norms_and_leaves_the_shipped_configurations_alone():
    import copy
    from wc_gan_amd.train import CONFIGS, renorm_config
    before = copy.deepcopy(CONFIGS)
    for name, base in CONFIGS.items():
        cfg = renorm_config(base)
        assert cfg['generator']['block_norm'] == 'dr' and cfg['generator']['last_norm'] == 'dr', name
        rest = {k: v for k, v in cfg['generator'].items() if k not in ('block_norm', 'last_norm')}
        assert rest == {k: v for k, v in base['generator'].items() if k not in ('block_norm', 'last_norm')}
        assert cfg['discriminator'] == base['discriminator']
    assert CONFIGS == before
    assert all(c['generator'].get('block_norm') != 'dr' and c['generator'].get('last_norm') != 'dr' for c in CONFIGS.values())


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("answer", [True, False])
def test_a_renorm_layer_takes_planes_where_its_plain_twin_does(monkeypatch, training, answer):
    from wc_gan_amd import layers
    from wc_gan_amd.layers import DecorelationNormalization, supports_statistic_groups
    asked = []

    def fake(shape, train, groups=1):
        asked.append((tuple(shape), bool(train), groups))
        return answer

    monkeypatch.setattr(layers.WF, "split_route_supported", fake)
    monkeypatch.setattr(layers, "USE_TORCH_OPS", False)
    shape = (128, 16, 16, 256)
    twins = [DecorelationNormalization(name=n, renorm=r, channels=256).train(training) for n, r in (('r', True), ('d', False))]
    got = [m.takes_split(shape) for m in twins]
    assert got == [answer, answer]
    assert asked == [(shape, training, 1)] * 2
    assert not twins[0].takes_split((128, 16, 16, 128))            # another width than the layer's: refused before the route is asked
    # ... while the grouped form stays refused for renorm
    assert not supports_statistic_groups(twins[0]) and supports_statistic_groups(twins[1])
