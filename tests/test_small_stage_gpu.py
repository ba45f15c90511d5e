"""The C x C float64 stage on the GPU at every route edge of its host dispatch, against the float64 references of
small_stage_reference.py (bounds and their derivation: that module's docstring; the references themselves are pinned in
test_small_stage_cpu.py).  csrc/wc_small.hip behind csrc/wc_abi.hip:

  K2  wc_factor_f64        three launch sequences (wc_factor_route): Cholesky + level-doubling inverse above C = 256 (with and without the
                           trailing partial pair), the fused factor + tri_inverse_cols<1..4> in two launches, both in one launch (one
                           stage / three stages) -- each row asserts the route the library reports, and the error words of the one-launch
                           form where it has them (the workspace is handed over as 0xFF bytes, L and W as NaN: what is not written shows)
  K5  wc_bwd_factor_f64    the three head forms, the wbar_parts route at its edges (Kc = 31 | 32, 33, 47, 64), training = 0, ddof = 0
      wc_color_f32         groups, per_group, gamma = None, C up to 1024
      wc_group_bias_f32 / wc_group_bias_centered_f32      row quarters that are no multiple of 16, the second column pass, per_group

Everything is built on the CPU from a few hundred rows; no tensor is larger than Kc C^2.
`PYTHONPATH=. python tests/test_small_stage_gpu.py` prints every row (the GPU half of profiles/small_stage_parity.txt)."""
import numpy as np
import pytest
import torch

import small_stage_reference as ref

pytestmark = pytest.mark.gpu
_ID = lambda r: "-".join(map(str, r))
ROUTE_NAME = {0: "cholesky+levels", 1: "fused,2 launches", 2: "fused,1 launch"}


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy()


# ---- K2 -----------------------------------------------------------------------------------------------------------------------------
def _hip_k2(case):
    """wc_factor_f64 through the C ABI (ops.factor keeps the workspace to itself) -> (outputs, error words | None)"""
    from wc_gan_amd import _lib
    from wc_gan_amd.ops import _ptr, _stream
    lib = _lib.load()
    C, G, tr = case["C"], case["groups"], case["training"]
    s, xtx = (dev(case["s"], torch.float64), dev(case["xtx"], torch.float64)) if tr else (None, None)
    mm, mc = dev(case["moving_mean0"]), dev(case["moving_cov0"])
    mu = torch.full((G, C), float("nan"), device="cuda")
    cs = torch.full((C,), float("nan"), device="cuda") if case["want_scale"] else None
    L = torch.full((G, C, C), float("nan"), dtype=torch.float64, device="cuda"); W = torch.full_like(L, float("nan"))
    nb = lib.wc_factor_workspace_bytes(C, G)
    assert nb >= G * C * C * 8
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    _lib.check(lib.wc_factor_f64(_ptr(s), _ptr(xtx), case["M"], C, G, case["eps"], case["momentum"], case["ddof"], tr, _ptr(mm), _ptr(mc),
                                 _ptr(mu), _ptr(cs), _ptr(L), _ptr(W), _ptr(ws), ws.numel(), _stream()), "wc_factor_f64")
    torch.cuda.synchronize()
    off = lib.wc_factor_error_offset(C, G)
    words = host(ws[off:off + 64 * G].view(torch.int32)[::16]) if off else None
    return dict(mu=host(mu), L=host(L), W=host(W), chan_scale=host(cs), moving_mean=host(mm), moving_cov=host(mc)), words


def _k2_row(C, G, variant="base"):
    from wc_gan_amd import _lib
    lib = _lib.load()
    case = ref.k2_case(C, G, variant)
    out, words = _hip_k2(case)
    fig, exact = ref.check_k2(case, out)
    route = lib.wc_factor_route(C, G)
    exact["error_words_iff_one_launch"] = (words is not None) == (route == 2)
    if words is not None:
        exact["error_words_zero"] = bool(len(words) == G and (words == 0).all())
    return f"K2 {_ID((C, G, variant))} [{ROUTE_NAME[route]}]", fig, exact


@pytest.mark.parametrize("C,G,route", ref.K2_ROUTE_ROWS, ids=lambda v: str(v))
def test_k2_at_every_route(C, G, route):
    from wc_gan_amd import _lib
    assert _lib.load().wc_factor_route(C, G) == route          # the row is there for THIS route: a gate that moves fails it instead of emptying it
    ref.assert_report(*_k2_row(C, G))


@pytest.mark.parametrize("C,G,variant", ref.K2_PARAM_ROWS, ids=lambda v: str(v))
def test_k2_parameter_edges(C, G, variant):
    """ddof = 0, momentum 0 and 1, no moving statistics, no chan_scale, evaluation mode on a moving covariance that is not symmetric in
    float32, fewer rows than channels -- on one shape per route"""
    ref.assert_report(*_k2_row(C, G, variant))


# ---- K5 -----------------------------------------------------------------------------------------------------------------------------
def _hip_k5(case, Kc, R):
    from wc_gan_amd import ops
    d64 = lambda a: dev(a, torch.float64)
    gam, A = dev(case["gamma"]), dev(case["A"])                       # Kc + surplus slots on the device; the call sees the first Kc
    Rd, gs = d64(R), d64(case["gsum"])
    dg, db, S, gm = ops.bwd_factor(Rd[:Kc], gs[:Kc], d64(case["W"]), d64(case["L"]), None if gam is None else gam[:Kc], A[:Kc], case["M"],
                                   case["eps"], case["ddof"], bool(case["training"]), want_dgamma=case["want_dgamma"])
    torch.cuda.synchronize()
    return dict(dgamma=host(dg), dbeta=host(db), S=host(S), gmean=host(gm))


def _k5_row(form, C, Kc):
    case = ref.k5_case(form, C, Kc)
    out = _hip_k5(case, Kc, case["R"])
    fig, exact = ref.check_k5(case, out)
    if Kc >= 31:
        # the slots BEHIND the Kc the call is told about hold non-zero Gamma, and now non-zero R too: a partial sum that ran past
        # red_total (or a part that should be empty and is not) changes the answer only in this second run
        again = _hip_k5(case, Kc, case["R_extra"])
        fig2, _ = ref.check_k5(case, again)
        fig.update({k + "_surplusR": v for k, v in fig2.items()})
        exact["same_with_surplus_R"] = all(np.array_equal(out[k], again[k]) for k in out if out[k] is not None)
    return f"K5 {_ID((form, C, Kc))}", fig, exact


@pytest.mark.parametrize("form,C,Kc", ref.K5_ROWS, ids=lambda v: str(v))
def test_k5_against_autograd(form, C, Kc):
    ref.assert_report(*_k5_row(form, C, Kc))


def _k5_threshold_row():
    case = ref.k5_case("parts", 32, 31)
    a = _hip_k5(case, 31, case["R"])
    b = _hip_k5(case, 32, case["R"])          # slot 31: Gamma non-zero, R and gsum zero -> the same sums through 16 partials of two terms
    one_ulp = 2.0 ** -23                      # two float32 roundings of float64 values that differ by rounding: at most one ulp of the largest entry apart
    fig = dict(S=(ref.rel(b["S"], a["S"]), one_ulp), gmean=(ref.rel(b["gmean"], a["gmean"]), one_ulp),
               dgamma=(ref.rel(b["dgamma"][:31], a["dgamma"]), one_ulp))
    return "K5 Kc 31 | 32 (one launch | wbar_parts)", fig, dict(empty_slot_dgamma_zero=bool((b["dgamma"][31] == 0).all()),
                                                                 empty_slot_dbeta_zero=bool((b["dbeta"][31] == 0).all()))


def test_k5_single_launch_and_parts_give_the_same_S():
    ref.assert_report(*_k5_threshold_row())


# ---- colouring and grouped bias -----------------------------------------------------------------------------------------------------
def _color_row(C, Kc, groups, per_group):
    from wc_gan_amd import ops
    case = ref.color_case(C, Kc, groups, per_group)
    A, At = ops.color(dev(case["W"], torch.float64), dev(case["gamma"]), groups=groups, per_group=bool(per_group))
    torch.cuda.synchronize()
    return (f"colour {_ID((C, Kc, groups, per_group))}",) + ref.check_color(case, host(A), host(At))


@pytest.mark.parametrize("C,Kc,groups,per_group", ref.COLOR_ROWS, ids=lambda v: str(v))
def test_colouring_against_the_einsum(C, Kc, groups, per_group):
    ref.assert_report(*_color_row(C, Kc, groups, per_group))


def _bias_row(C, G, Kc, per_group, with_beta):
    from wc_gan_amd import ops
    case = ref.bias_case(C, G, Kc, per_group)
    mu, A, beta = dev(case["mu"]), dev(case["A"]), dev(case["beta"]) if with_beta else None
    center, bias = ops.group_bias(mu, A, beta, G, Kc, bool(per_group))
    given = dev(case["given"])
    biasc = ops.group_bias_centered(mu, A, beta, given, G, Kc, bool(per_group))
    torch.cuda.synchronize()
    key = "bias_" if with_beta else "nobeta_"
    fig = dict(center=(ref.rel(host(center), case["center"]), ref.f32_bound()), bias=(ref.rel(host(bias), case[key + "mean"]), ref.f32_bound()),
               bias_centred=(ref.rel(host(biasc), case[key + "given"]), ref.f32_bound()))
    return f"bias {_ID((C, G, Kc, per_group))}{'' if with_beta else ' no beta'}", fig, dict(given_centre_untouched=bool(np.array_equal(host(given), case["given"])))


@pytest.mark.parametrize("with_beta", [True, False], ids=["beta", "nobeta"])
@pytest.mark.parametrize("C,G,Kc,per_group", ref.BIAS_ROWS, ids=lambda v: str(v))
def test_grouped_bias_against_the_einsum(C, G, Kc, per_group, with_beta):
    ref.assert_report(*_bias_row(C, G, Kc, per_group, with_beta))


if __name__ == "__main__":
    def show(tag, fig, exact):
        print(ref.format_report(tag, fig, exact))
    print("measured/bound per tensor against float64 (small_stage_reference.py); exact: the bit-exact properties that held")
    for C, G, _route in ref.K2_ROUTE_ROWS:
        show(*_k2_row(C, G))
    for row in ref.K2_PARAM_ROWS:
        show(*_k2_row(*row))
    for row in ref.K5_ROWS:
        show(*_k5_row(*row))
    show(*_k5_threshold_row())
    for row in ref.COLOR_ROWS:
        show(*_color_row(*row))
    for row in ref.BIAS_ROWS:
        for wb in (True, False):
            show(*_bias_row(*row, wb))
