"""The references of small_stage_reference.py pinned before the GPU sees them, and its case tables run against the `_cpu` twin
(oracle/wc_cpu.cpp through oracle/cpu_port.py).  No GPU.

  * K5's autograd reference against oracle.wc_backward (dgamma, dbeta, and S through the dx it produces), against the textbook chain
    restated on (R, W, L, Gamma), and against the collapsed Cholesky step of test_k5_algebra.py -- on 'ill' inputs.
  * per K2 row: how far LAPACK and torch differ on L and W (the GPU test's bounds come from here, small_stage_reference.k2_bounds), the
    reference's own residuals, and the frexp mantissa of sqrt(tmax) inside [0.51, 0.99] for EVERY channel (chan_scale is compared bit
    for bit on the GPU).
  * every row of the K2 / K5 / colouring / bias tables against the twin, with the bounds the GPU test uses.  Rows whose arguments the
    twin's loader cannot express are skipped in the parametrisation, with the reason.

`PYTHONPATH=. python tests/test_small_stage_cpu.py` prints the CPU half of profiles/small_stage_parity.txt."""
import numpy as np
import pytest

import small_stage_reference as ref
from oracle import wc_oracle as o

ALL_K2 = [(C, G, "base") for (C, G, _r) in ref.K2_ROUTE_ROWS] + ref.K2_PARAM_ROWS
_ID = lambda r: "-".join(map(str, r))


# ---- the autograd reference against the oracle --------------------------------------------------------------------------------------
def _oracle_row(C, Kc):
    rng = np.random.default_rng(300 + C + Kc)
    M = 4 * C + 3
    x = o.synth_activation(rng, (M, C), "ill")
    G, B = o.synth_coloring(rng, C, Kc)
    slot = rng.permutation(np.arange(M) % Kc)
    gy = rng.standard_normal((M, C))
    _, cache = o.wc_forward(x, G, B, slot)
    dx, dgamma, dbeta = o.wc_backward(gy, cache)
    R = np.stack([cache["f"][slot == k].T @ gy[slot == k] for k in range(Kc)])
    gsum = np.stack([gy[slot == k].sum(0) for k in range(Kc)])
    T = (1.0 - cache["eps"]) * cache["sigma"] + cache["eps"] * np.eye(C)
    return cache, slot, gy, R, gsum, T, dx, dgamma, dbeta


# float64 on cond(T) <= 1e6: both sides carry ~cond * 2^-53 * (a small multiple of sqrt(C)) ~ 1e-10 .. 1e-9; 1e-8 is a sixth of the float32
# floor 2^-24 the GPU bounds start from, so a reference that passes here cannot be what decides a float32 comparison
PIN = 1e-8


@pytest.mark.parametrize("C", [32, 96, 256])
@pytest.mark.parametrize("Kc", [1, 3])
def test_autograd_reference_agrees_with_the_oracles_closed_form(C, Kc):
    cache, slot, gy, R, gsum, T, dx, dgamma, dbeta = _oracle_row(C, Kc)
    M = cache["M"]
    dg_ag, S_ag = ref.k5_autograd(R, T, cache["G"], M, cache["eps"], cache["ddof"])
    # S through what the oracle makes of it: dx = fbar - mean(fbar), fbar = g A_k^T + f S
    fbar = np.einsum("mo,mio->mi", gy, cache["A"][slot]) + cache["f"] @ S_ag
    errs = dict(dgamma=ref.rel(dg_ag, dgamma), dbeta=ref.rel(gsum, dbeta), dx_from_S=ref.rel(fbar - fbar.mean(0), dx))
    # the restated textbook chain IS the oracle's (same S into the same dx), and the autograd S equals it and the collapsed step
    dg_cf, S_cf = ref.k5_closed_form(R, cache["W"], cache["L"], cache["G"], M, cache["eps"], cache["ddof"])
    fbar_cf = np.einsum("mo,mio->mi", gy, cache["A"][slot]) + cache["f"] @ S_cf
    errs.update(restated_dx=ref.rel(fbar_cf - fbar_cf.mean(0), dx), restated_dgamma=ref.rel(dg_cf, dgamma), S=ref.rel(S_ag, S_cf),
                S_collapsed=ref.rel(ref.k5_closed_form(R, cache["W"], cache["L"], cache["G"], M, cache["eps"], cache["ddof"], collapsed=True)[1], S_ag))
    print("K5 reference", C, Kc, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= PIN for v in errs.values()), errs
    assert errs["restated_dx"] <= 1e-12 and errs["restated_dgamma"] <= 1e-12          # the same arithmetic, restated


def test_autograd_reference_of_the_identity_colouring():
    """Gamma = I, Kc = 1: the case wc_bwd_factor_f64 reads Wbar = R^T for"""
    cache, slot, gy, R, gsum, T, dx, dgamma, dbeta = _oracle_row(96, 1)
    _, c1 = o.wc_forward(cache["f"] + cache["mu"], None, None, None)
    dx1 = o.wc_backward(gy, c1)[0]
    _, S = ref.k5_autograd(R, T, None, c1["M"], c1["eps"], c1["ddof"])
    fbar = gy @ c1["A"][0].T + c1["f"] @ S
    assert ref.rel(fbar - fbar.mean(0), dx1) <= PIN


# ---- the K2 references against each other -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ALL_K2, ids=_ID)
def test_k2_references_agree_and_chan_scale_is_decidable(row):
    case = ref.k2_case(*row)
    ag = ref.k2_agreement(*row)
    b = ref.k2_bounds(*row)
    print("K2 references", _ID(row), {k: f"{v:.2e}" for k, v in ag.items()}, "bounds", {k: f"{v:.2e}" for k, v in b.items()},
          f"mantissa {case['mant'].min():.3f}..{case['mant'].max():.3f}")
    assert case["mant"].min() >= 0.51 and case["mant"].max() <= 0.99          # every channel: a last-bit difference cannot flip the exponent
    assert b["L"] >= 4.0 * ag["L"] and b["W"] >= 4.0 * ag["W"]                 # the bound leaves the references' own disagreement four times over
    assert b["L"] <= 1e-8 and b["W"] <= 1e-7, b                                # ... and a row that needs more than 10 x the suite's bounds is too ill-conditioned to keep
    assert ag["res_L"] < 1e-13 and b["f32"] <= 1e-6
    if case["variant"] == "eval":
        assert (case["moving_cov0"] != case["moving_cov0"].T).any()


@pytest.mark.parametrize("row", ref.K5_ROWS, ids=_ID)
def test_k5_bounds_stay_under_the_twin_comparisons_limits(row):
    e = ref.k5_expected(*row)
    print("K5 spread", _ID(row), {k: f"{v:.2e}" for k, v in e["spread"].items()})
    for k, lim in ref.K5_LIMIT.items():
        assert ref.f32_bound(e["spread"][k]) <= lim, (k, e["spread"][k])


# ---- the tables against the `_cpu` twin ---------------------------------------------------------------------------------------------
def _twin_k2(cp, case):
    mm = None if case["moving_mean0"] is None else case["moving_mean0"].copy()
    mc = None if case["moving_cov0"] is None else case["moving_cov0"].copy()
    tr = bool(case["training"])
    mu, L, W, cs = cp.factor(case["s"] if tr else None, case["xtx"] if tr else None, case["M"], case["C"], case["eps"], case["momentum"],
                             case["ddof"], tr, mm, mc, case["groups"])
    return dict(mu=mu, L=L, W=W, chan_scale=cs, moving_mean=mm, moving_cov=mc)


_NOSCALE = "oracle/cpu_port.factor always passes chan_scale: the twin cannot be called without it"
K2_TWIN = [pytest.param(r, marks=pytest.mark.skip(reason=_NOSCALE)) if r[2] == "noscale" else r for r in ALL_K2]


@pytest.mark.parametrize("row", K2_TWIN, ids=_ID)
def test_k2_table_against_the_cpu_twin(row):
    from oracle import cpu_port as cp
    case = ref.k2_case(*row)
    ref.assert_report("twin K2 " + _ID(row), *ref.check_k2(case, _twin_k2(cp, case)))


def _twin_k5(cp, case):
    Kc = case["Kc"]
    gam = None if case["gamma"] is None else case["gamma"][:Kc]
    dg, db, S, gm = cp.bwd_factor(case["R"][:Kc], case["gsum"][:Kc], case["W"], case["L"], gam, case["A"][:Kc], case["M"], case["eps"],
                                  case["ddof"], bool(case["training"]))
    return dict(dgamma=dg, dbeta=db, S=S, gmean=gm)


_NODG = "oracle/cpu_port.bwd_factor computes dgamma whenever gamma is given: the twin has no head without it"
K5_TWIN = [pytest.param(r, marks=pytest.mark.skip(reason=_NODG)) if r[0] == "nodg" else r for r in ref.K5_ROWS]


@pytest.mark.parametrize("row", K5_TWIN, ids=_ID)
def test_k5_table_against_the_cpu_twin(row):
    from oracle import cpu_port as cp
    case = ref.k5_case(*row)
    ref.assert_report("twin K5 " + _ID(row), *ref.check_k5(case, _twin_k5(cp, case)))


@pytest.mark.parametrize("row", ref.COLOR_ROWS, ids=_ID)
def test_colouring_table_against_the_cpu_twin(row):
    from oracle import cpu_port as cp
    C, Kc, groups, per_group = row
    case = ref.color_case(*row)
    A, At = cp.color(case["W"], case["gamma"], groups, bool(per_group))
    ref.assert_report("twin colour " + _ID(row), *ref.check_color(case, A, At))


def _twin_bias(cp, case, C, G, Kc, per_group, beta):
    import ctypes
    center = np.empty(C, np.float32); bias = np.empty((G * Kc, C), np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = cp.load().wc_group_bias_f32_cpu(p(case["mu"]), p(case["A"]), p(beta), G, Kc, C, per_group, p(center), p(bias), None)
    assert rc == 0
    return center, bias


@pytest.mark.parametrize("with_beta", [True, False], ids=["beta", "nobeta"])
@pytest.mark.parametrize("row", ref.BIAS_ROWS, ids=_ID)
def test_bias_table_against_the_cpu_twin(row, with_beta):
    """(the centred form, wc_group_bias_centered_f32, has no `_cpu` twin: it runs on the GPU only)"""
    from oracle import cpu_port as cp
    case = ref.bias_case(*row)
    center, bias = _twin_bias(cp, case, *row, case["beta"] if with_beta else None)
    fig = dict(center=(ref.rel(center, case["center"]), ref.f32_bound()),
               bias=(ref.rel(bias, case["bias_mean" if with_beta else "nobeta_mean"]), ref.f32_bound()))
    ref.assert_report("twin bias " + _ID(row) + ("" if with_beta else " no beta"), fig, {})


if __name__ == "__main__":
    print("K2: LAPACK (scipy) against torch per row -- rel of L and W, the reference's residuals |L L^T - T|/|T| and |W L - I|, and the "
          "bounds derived from them")
    for row in ALL_K2:
        ag, b, case = ref.k2_agreement(*row), ref.k2_bounds(*row), ref.k2_case(*row)
        print(f"{_ID(row):<20}" + "  ".join(f"{k}={v:.2e}" for k, v in ag.items()) + "   bounds " + "  ".join(f"{k}={v:.2e}" for k, v in b.items()) +
              f"   mantissa {case['mant'].min():.3f}..{case['mant'].max():.3f}")
    print("\nK5: spread of the autograd reference from the textbook closed form per row (the float32 bound is 4 x max(2^-24, spread))")
    for row in ref.K5_ROWS:
        e = ref.k5_expected(*row)
        print(f"{_ID(row):<20}" + "  ".join(f"{k}={v:.2e}" for k, v in e["spread"].items() if k in ("dgamma", "S")))
