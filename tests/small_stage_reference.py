"""Float64 references, inputs, case tables and bounds for the C x C stage of the WC path (csrc/wc_small.hip behind csrc/wc_abi.hip): K2
(wc_factor_f64), the colouring product (wc_color_f32), the grouped bias (wc_group_bias_f32 / wc_group_bias_centered_f32) and K5
(wc_bwd_factor_f64).  numpy / scipy / torch on the CPU only; the library under test is never imported here.  test_small_stage_cpu.py runs
the tables against the `_cpu` twin and pins the references to each other, test_small_stage_gpu.py runs them against the HIP library.

K5's reference is a derivative taken by torch.autograd, not a formula: with R (Kc, C, C) and Gamma constant,
    l(T, Gamma) = sum_k <R_k, W(T)^T Gamma_k>,   W(T) = solve_triangular(cholesky(T), I)
is the loss as the site sees it (y_n = f_n W^T Gamma_k, gradient g_n, R_k = sum_n f_n^T g_n), so dgamma = dl/dGamma and, T being
(1 - eps) f^T f / (M - ddof) + eps I, the matrix the apply multiplies f by is S = 2 (1 - eps) / (M - ddof) sym(dl/dT).

Bounds ("rel" = max |a - b| / max |b|, as everywhere in tests/):
  * L, W (float64): the suite's 1e-9 / 1e-8 where LAPACK (scipy) and torch agree on the row to a quarter of that, else 4 x their measured
    disagreement (k2_bounds); the residuals |L L^T - T| / |T| and |W L - I| at 100 x the reference's own.
  * float32 outputs: 4 x max(2^-24, spread), 2^-24 being the rounding of the reference itself to float32 (every entry moves by at most
    2^-24 of itself, hence of the largest entry) and `spread` the rel distance of the autograd reference from the textbook closed form on
    the same row (K5 only; zero elsewhere: one reference) -- and never above the twin comparison's 1e-6 (mu, moving statistics, A, dgamma,
    dbeta) / 1e-5 (S, gmean), which test_small_stage_cpu.py asserts of the derived bounds.
  * bit-exact: chan_scale, At against A, the strict upper triangles of L and W, S against S^T, the moving statistics in evaluation mode.
The moving statistics are float32 STATE: "group after group, as separate calls would" means each group's update is rounded to float32 before
the next one reads it, and the reference does the same."""
import functools

import numpy as np
import scipy.linalg as sla
import torch

from oracle import wc_oracle as o

EPS, MOMENTUM = 1e-3, 0.99
F32 = 2.0 ** -24


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def f32_bound(spread=0.0):
    return 4.0 * max(F32, spread)


# =====================================================================================================================================
# K2
# =====================================================================================================================================
# (C, groups, route): route as wc_factor_route reports it -- 0 Cholesky + level-doubling inverse, 1 fused factor + column inverse in two
# launches, 2 both in one launch.  The comment names what the row is there for.
K2_ROUTE_ROWS = [
    (32, 1, 1),      # two launches, tri_inverse_cols<1>, two block columns
    (32, 3, 1),
    (64, 3, 1),
    (96, 1, 1),      # <2>, a row block of 768 pieces on 1024 slots
    (96, 4, 1),
    (128, 8, 2),     # one launch at the gate's edge: 8 * (1 + 4) = 40 workgroups
    (160, 1, 2),     # one stage
    (192, 1, 2),     # one stage at its largest phase, 66 blocks of CP_MAXB = 75
    (192, 8, 2),
    (224, 1, 2),     # three stages
    (256, 8, 2),
    (128, 9, 1),     # the gate closed: 9 groups -> two launches, <2>
    (160, 9, 1),     # <3>: reachable only here and at (192, 9)
    (192, 9, 1),
    (224, 9, 1),     # <4>
    (512, 1, 0),     # level inverse, complete pairs only
    (1024, 1, 0),
    (288, 1, 0),     # trailing partial pair, mrows = 32 (k = 32: the GEMM's 4-wide tail only)
    (320, 2, 0),     # mrows = 64
    (352, 1, 0),     # mrows = 32 then 96 (k = 96: one 16-wide group, then the tail)
    (384, 3, 0),     # mrows = 128
    (768, 1, 0),     # mrows = 256
]
K2_PARAM_SHAPES = [(64, 2), (192, 2), (320, 1)]          # one per route
K2_VARIANTS = ["ddof0", "mom0", "mom1", "nomoving", "noscale", "eval", "fewrows"]
K2_PARAM_ROWS = [(C, G, v) for (C, G) in K2_PARAM_SHAPES for v in K2_VARIANTS]


def _variant_args(variant, C):
    a = dict(ddof=1, momentum=MOMENTUM, training=1, moving=True, want_scale=True, M=4 * C + 3)
    if variant == "ddof0": a["ddof"] = 0
    elif variant == "mom0": a["momentum"] = 0.0
    elif variant == "mom1": a["momentum"] = 1.0
    elif variant == "nomoving": a["moving"] = False
    elif variant == "noscale": a["want_scale"] = False
    elif variant == "eval": a["training"] = 0
    elif variant == "fewrows": a["M"] = C // 2
    elif variant != "base": raise ValueError(variant)
    return a


def factor_lapack(T):
    L = np.stack([sla.cholesky(t, lower=True) for t in T])
    W = np.stack([sla.solve_triangular(l, np.eye(l.shape[0]), lower=True) for l in L])
    return L, W


def factor_torch(T):
    Tt = torch.tensor(T, dtype=torch.float64)
    L = torch.linalg.cholesky(Tt)
    W = torch.linalg.solve_triangular(L, torch.eye(T.shape[-1], dtype=torch.float64).expand_as(L), upper=False)
    return L.numpy(), W.numpy()


def k2_prepare(s, xtx, G, M, eps, momentum, ddof, training, moving_mean, moving_cov):
    """mu (G, C), T (G, C, C) float64, the moving statistics after all groups (float32 | None), and sqrt(max_g T_g[j][j])"""
    C = s.shape[-1]
    mm = None if moving_mean is None else np.array(moving_mean, np.float32)
    mc = None if moving_cov is None else np.array(moving_cov, np.float32)
    mu = np.empty((G, C)); T = np.empty((G, C, C))
    for g in range(G):
        if training:
            m = s[g] / M
            sig = (0.5 * (xtx[g] + xtx[g].T) - np.outer(s[g], s[g]) / M) / (M - ddof)
            if mm is not None:          # float32 state: rounded after every group
                mm = (momentum * mm.astype(np.float64) + (1.0 - momentum) * m).astype(np.float32)
                mc = (momentum * mc.astype(np.float64) + (1.0 - momentum) * sig).astype(np.float32)
        else:
            m = mm.astype(np.float64)
            sig = 0.5 * (mc.astype(np.float64) + mc.astype(np.float64).T)
        mu[g] = m
        T[g] = (1.0 - eps) * sig + eps * np.eye(C)
    rt = np.sqrt(np.diagonal(T, axis1=1, axis2=2).max(0))
    return mu, T, mm, mc, rt


def chan_scale_of(rt):
    mant, e = np.frexp(rt)
    return np.ldexp(1.0, 3 - e), mant


@functools.lru_cache(maxsize=None)
def k2_case(C, groups, variant="base"):
    """Inputs and float64 expectations of one K2 row.  The rows are synth_activation(rng, (M, C), 'ill') per group (each group its own
    draw and mix).  chan_scale is compared bit for bit, so no channel's sqrt(tmax) may sit where a last-bit difference flips frexp's
    exponent: its mantissa has to lie in [0.51, 0.99].  A channel misses that band with probability log2(0.51 / 0.5) + log2(1 / 0.99)
    = 4.3 %, so no seed passes at C = 1024 (0.957^1024 ~ 1e-20; 1.5 % at C = 96): instead every channel outside [0.53, 0.97] is rescaled
    by 1.09 in all groups (a diagonal scaling of the input, at most twice per channel) until none is left.  test_small_stage_cpu.py asserts
    the band on the result, all channels."""
    a = _variant_args(variant, C)
    M, training = a["M"], a["training"]
    seed = 1000 + 7 * C + groups + 131 * K2_VARIANTS.index(variant) if variant != "base" else 1000 + 7 * C + groups
    rng = np.random.default_rng(seed)
    x = np.stack([o.synth_activation(rng, (M, C), "ill") for _ in range(groups)])
    xm = o.synth_activation(rng, (4 * C + 3, C), "ill")                    # the batch the initial moving statistics come from
    asym = 1e-6 * np.triu(rng.standard_normal((C, C)), 1)
    for _ in range(8):
        s = x.sum(1); xtx = np.einsum("gmi,gmj->gij", x, x)
        mm0 = (0.5 * xm.mean(0)).astype(np.float32)
        mc0 = (np.cov(xm, rowvar=False) + asym).astype(np.float32)         # NOT symmetric in float32: evaluation mode symmetrises it
        moving = a["moving"] or not training
        args = (s, xtx, groups, M, EPS, a["momentum"], a["ddof"], training, mm0 if moving else None, mc0 if moving else None)
        mu, T, mm, mc, rt = k2_prepare(*args)
        cs, mant = chan_scale_of(rt)
        bad = (mant < 0.53) | (mant > 0.97)
        if not bad.any():
            break
        x[:, :, bad] *= 1.09; xm[:, bad] *= 1.09
    assert (mc0 != mc0.T).any()
    L, W = factor_lapack(T)
    return dict(C=C, groups=groups, variant=variant, M=M, eps=EPS, momentum=a["momentum"], ddof=a["ddof"], training=training,
                want_scale=a["want_scale"], s=s, xtx=xtx, moving_mean0=mm0 if moving else None, moving_cov0=mc0 if moving else None,
                mu=mu, T=T, L=L, W=W, moving_mean=mm, moving_cov=mc, chan_scale=cs.astype(np.float32), mant=mant)


@functools.lru_cache(maxsize=None)
def k2_agreement(C, groups, variant="base"):
    """How far two float64 references -- LAPACK through scipy, and torch -- differ on the row's T: rel per tensor (the worst group), and
    the reference's own residuals."""
    case = k2_case(C, groups, variant)
    Lt, Wt = factor_torch(case["T"])
    out = dict(L=max(rel(Lt[g], case["L"][g]) for g in range(groups)), W=max(rel(Wt[g], case["W"][g]) for g in range(groups)))
    out["res_L"], out["res_W"] = k2_residuals(case["T"], case["L"], case["W"])
    return out


def k2_residuals(T, L, W):
    """max over groups of |L L^T - T|_F / |T|_F and |W L - I|_F"""
    eye = np.eye(T.shape[-1])
    return (max(float(np.linalg.norm(l @ l.T - t) / np.linalg.norm(t)) for t, l in zip(T, L)),
            max(float(np.linalg.norm(w @ l - eye)) for l, w in zip(L, W)))


def k2_bounds(C, groups, variant="base"):
    ag = k2_agreement(C, groups, variant)
    return dict(L=1e-9 if ag["L"] <= 0.25e-9 else 4.0 * ag["L"], W=1e-8 if ag["W"] <= 0.25e-8 else 4.0 * ag["W"],
                res_L=100.0 * ag["res_L"], res_W=100.0 * ag["res_W"], f32=f32_bound())


def check_k2(case, out):
    """out: mu (G, C) f32, L, W (G, C, C) f64, chan_scale (C,) f32 | None, moving_mean / moving_cov f32 | None, as the backend left them.
    -> (figures {name: (measured, bound)}, exact {name: bool}); assert_report() asserts them."""
    C, G, v = case["C"], case["groups"], case["variant"]
    b = k2_bounds(C, G, v)
    L = out["L"].reshape(G, C, C); W = out["W"].reshape(G, C, C)
    fig = dict(L=(max(rel(L[g], case["L"][g]) for g in range(G)), b["L"]), W=(max(rel(W[g], case["W"][g]) for g in range(G)), b["W"]),
               mu=(max(rel(out["mu"].reshape(G, C)[g], case["mu"][g]) for g in range(G)), b["f32"]))
    rl, rw = k2_residuals(case["T"], L, W)
    fig["res_L"] = (rl, b["res_L"]); fig["res_W"] = (rw, b["res_W"])
    exact = dict(upper_L=bool((np.triu(L, 1) == 0.0).all()), upper_W=bool((np.triu(W, 1) == 0.0).all()))
    if case["want_scale"]:
        exact["chan_scale"] = bool(np.array_equal(out["chan_scale"], case["chan_scale"]))
    if case["moving_mean0"] is not None:
        if case["training"]:
            fig["moving_mean"] = (rel(out["moving_mean"], case["moving_mean"]), b["f32"])
            fig["moving_cov"] = (rel(out["moving_cov"], case["moving_cov"]), b["f32"])
        else:
            exact["moving_untouched"] = bool(np.array_equal(out["moving_mean"], case["moving_mean0"]) and
                                             np.array_equal(out["moving_cov"], case["moving_cov0"]))
            exact["mu_is_moving_mean"] = bool(all(np.array_equal(out["mu"].reshape(G, C)[g], case["moving_mean0"]) for g in range(G)))
    return fig, exact


def assert_report(tag, fig, exact):
    """print every figure, then assert all of them"""
    print(format_report(tag, fig, exact))
    bad = [k for k, (m, bnd) in fig.items() if not m <= bnd] + [k for k, ok in exact.items() if not ok]
    assert not bad, (tag, bad, {k: fig[k] for k in bad if k in fig})


def format_report(tag, fig, exact):
    return f"{tag:<34}" + "  ".join(f"{k}={m:.2e}/{bnd:.2e}" for k, (m, bnd) in fig.items()) + \
        ("  exact: " + ",".join(k if ok else "NOT-" + k for k, ok in exact.items()) if exact else "")


# =====================================================================================================================================
# K5
# =====================================================================================================================================
# (form, C, Kc).  pair: gamma given, dgamma wanted, training (gemm_f64_pair_kernel); nodg: dgamma not wanted; ident: gamma = None
# (Wbar = R^T through swapped strides); parts: Kc >= 32 -> 16 partial sums of ceil(Kc / 16) terms, red_total cutting the last ones short
# (33: five parts empty, 47: the last part cut mid-way; 31: the last single-launch value); eval: training = 0; ddof0.
K5_ROWS = [("pair", 32, 1), ("pair", 96, 3), ("pair", 160, 10), ("pair", 256, 2), ("pair", 352, 2), ("pair", 512, 1),
           ("nodg", 96, 3), ("nodg", 256, 2),
           ("ident", 64, 1), ("ident", 192, 1), ("ident", 320, 1),
           ("parts", 32, 31), ("parts", 32, 32), ("parts", 32, 33), ("parts", 64, 47), ("parts", 32, 64),
           ("eval", 96, 3), ("eval", 32, 33),
           ("ddof0", 128, 2)]
K5_ROWS_M = 327          # rows behind R and gsum ("a few hundred"); slot of row n = a table drawn once per row
K5_SURPLUS = 16          # table slots allocated BEHIND the Kc the call is told about (parts rows: what a part that ran past red_total reads)


@functools.lru_cache(maxsize=None)
def k5_case(form, C, Kc):
    """W, L, T from the float64 reference of an 'ill' batch; R, gsum from f^T g on K5_ROWS_M rows with a slot table; Gamma, A float32.
    The buffers hold Kc + K5_SURPLUS slots: the surplus slots carry non-zero Gamma and (R_extra) non-zero R."""
    rng = np.random.default_rng(5000 + 11 * C + Kc + 97 * ["pair", "nodg", "ident", "parts", "eval", "ddof0"].index(form))
    M = K5_ROWS_M
    ddof = 0 if form == "ddof0" else 1
    x = o.synth_activation(rng, (M, C), "ill")
    mu = x.mean(0); f = x - mu
    sig = f.T @ f / (M - ddof)
    T = (1.0 - EPS) * 0.5 * (sig + sig.T) + EPS * np.eye(C)
    L, W = factor_lapack(T[None]); L, W = L[0], W[0]
    g = rng.standard_normal((M, C))
    slot = rng.permutation(np.arange(M) % Kc)                 # every slot has rows (M >= Kc)
    Kb = Kc + K5_SURPLUS
    R = np.zeros((Kb, C, C)); gsum = np.zeros((Kb, C))
    for k in range(Kc):
        R[k] = f[slot == k].T @ g[slot == k]; gsum[k] = g[slot == k].sum(0)
    R_extra = R.copy(); R_extra[Kc:] = rng.standard_normal((K5_SURPLUS, C, C)) * np.abs(R[:Kc]).max()
    if form == "ident":
        gamma = None
        A = W.T[None].astype(np.float32)
    else:
        gamma = o.synth_coloring(rng, C, Kb)[0].astype(np.float32)
        A = np.einsum("ji,kjo->kio", W, gamma.astype(np.float64)).astype(np.float32)
    return dict(form=form, C=C, Kc=Kc, M=M, eps=EPS, ddof=ddof, training=0 if form == "eval" else 1, want_dgamma=form not in ("nodg", "ident"),
                T=T, L=L, W=W, R=R, R_extra=R_extra, gsum=gsum, gamma=gamma, A=A)


def k5_autograd(R, T, gamma, M, eps, ddof):
    """-> dgamma (Kc, C, C), S (C, C): derivatives of l(T, Gamma) taken by torch.autograd in float64"""
    C = T.shape[0]
    Tt = torch.tensor(T, dtype=torch.float64, requires_grad=True)
    Gt = torch.tensor(np.eye(C)[None] if gamma is None else np.asarray(gamma, np.float64), dtype=torch.float64, requires_grad=True)
    # W(T) reads the lower triangle of T only, as a Cholesky does: dl/dT is then triangular (off-diagonal entries carry both mirror
    # images' share) and sym() below is what unfolds it -- whichever convention the Cholesky's registered gradient follows.  Fed a full
    # symmetric leaf, torch's backward symmetrises on its own and the formula's sym could be dropped without any test noticing.
    Tlow = torch.tril(Tt) + torch.tril(Tt, -1).T
    Wt = torch.linalg.solve_triangular(torch.linalg.cholesky(Tlow), torch.eye(C, dtype=torch.float64), upper=False)
    loss = (torch.tensor(R, dtype=torch.float64) * (Wt.T @ Gt)).sum()
    loss.backward()
    dT = Tt.grad.numpy()
    return Gt.grad.numpy(), (2.0 * (1.0 - eps) / (M - ddof)) * 0.5 * (dT + dT.T)


def k5_closed_form(R, W, L, gamma, M, eps, ddof, collapsed=False):
    """The textbook chain of oracle.wc_backward on (R, W, L, Gamma) (test_small_stage_cpu.py pins this restatement to the oracle itself);
    collapsed: the one-product Cholesky step of wc_bwd_factor_f64, P = -Phi(Wbar W^T) (test_k5_algebra.py)."""
    C = W.shape[0]
    G = np.eye(C)[None] if gamma is None else np.asarray(gamma, np.float64)
    dgamma = np.einsum("ij,kjo->kio", W, R)
    Wbar = np.einsum("kij,klj->il", G, R)
    if collapsed:
        P = -np.tril(Wbar @ W.T)
    else:
        P = np.tril(L.T @ -np.tril(W.T @ Wbar @ W.T))
    P[np.diag_indices(C)] *= 0.5
    Sbar = W.T @ P @ W
    return dgamma, (2.0 * (1.0 - eps) / (M - ddof)) * 0.5 * (Sbar + Sbar.T)


@functools.lru_cache(maxsize=None)
def k5_expected(form, C, Kc):
    """The autograd expectations of the row and, per tensor, their spread from the closed form"""
    c = k5_case(form, C, Kc)
    R, gsum = c["R"][:Kc], c["gsum"][:Kc]
    gam = None if c["gamma"] is None else c["gamma"][:Kc]
    dgamma, S = k5_autograd(R, c["T"], gam, c["M"], c["eps"], c["ddof"])
    dg_cf, S_cf = k5_closed_form(R, c["W"], c["L"], gam, c["M"], c["eps"], c["ddof"])
    gmean = np.einsum("kj,kcj->c", gsum, c["A"][:Kc].astype(np.float64)) / c["M"]
    return dict(dgamma=dgamma, S=S, dbeta=gsum, gmean=gmean, spread=dict(dgamma=rel(dg_cf, dgamma), S=rel(S_cf, S), dbeta=0.0, gmean=0.0))


K5_LIMIT = dict(dgamma=1e-6, dbeta=1e-6, S=1e-5, gmean=1e-5)


def check_k5(case, out):
    """out: dgamma | None, dbeta, S | None, gmean | None (float32 numpy)"""
    e = k5_expected(case["form"], case["C"], case["Kc"])
    fig, exact = {}, {}
    want = ["dbeta"] + (["dgamma"] if case["want_dgamma"] else []) + (["S", "gmean"] if case["training"] else [])
    for k in want:
        fig[k] = (rel(out[k], e[k]), f32_bound(e["spread"][k]))
    for k in ("dgamma", "S", "gmean"):
        if k not in want:
            exact["no_" + k] = out.get(k) is None
    if case["training"]:
        exact["S_symmetric"] = bool(np.array_equal(out["S"], out["S"].T))
    return fig, exact


# =====================================================================================================================================
# colouring and grouped bias
# =====================================================================================================================================
COLOR_ROWS = [(96, 2, 1, 0), (160, 3, 4, 0), (64, 2, 3, 1), (512, 1, 2, 0), (1024, 1, 1, 0), (96, 0, 3, 0)]      # (C, Kc, groups, per_group); Kc = 0: gamma None
BIAS_ROWS = [(32, 1, 1, 0), (96, 3, 2, 0), (160, 5, 1, 0), (256, 2, 3, 1), (512, 2, 1, 0), (1024, 1, 2, 0)]      # (C, G, Kc, per_group)


@functools.lru_cache(maxsize=None)
def color_case(C, Kc, groups, per_group):
    """W (groups, C, C) from the float64 reference of 'ill' batches; A[g Kc + k] = W_g^T Gamma_k (Gamma_{g Kc + k} if per_group)"""
    rng = np.random.default_rng(7000 + 3 * C + 17 * Kc + groups)
    M = 2 * C + 3
    T = np.empty((groups, C, C))
    for g in range(groups):
        sig = np.cov(o.synth_activation(rng, (M, C), "ill"), rowvar=False)
        T[g] = (1.0 - EPS) * sig + EPS * np.eye(C)
    W = factor_lapack(T)[1]
    if Kc == 0:
        return dict(W=W, gamma=None, A=np.transpose(W, (0, 2, 1)).copy())
    gamma = o.synth_coloring(rng, C, Kc * (groups if per_group else 1))[0].astype(np.float32)
    G64 = gamma.astype(np.float64).reshape((groups, Kc, C, C) if per_group else (1, Kc, C, C))
    A = np.einsum("gji,gkjo->gkio", W, np.broadcast_to(G64, (groups, Kc, C, C))).reshape(groups * Kc, C, C)
    return dict(W=W, gamma=gamma, A=A)


def check_color(case, A, At):
    return dict(A=(rel(A, case["A"]), f32_bound())), dict(At_is_A_transposed=bool(np.array_equal(At, np.transpose(A, (0, 2, 1)))))


@functools.lru_cache(maxsize=None)
def bias_case(C, G, Kc, per_group):
    """center = mean_g mu_g (or the given one, deliberately NOT that mean); bias[g Kc + k] = beta - (mu_g - center) A[g Kc + k]"""
    rng = np.random.default_rng(9000 + 5 * C + 13 * G + Kc)
    mu = (0.2 + 0.5 * rng.standard_normal((G, C))).astype(np.float32)
    A = (rng.standard_normal((G * Kc, C, C)) / np.sqrt(C)).astype(np.float32)
    beta = (0.1 * rng.standard_normal((G * Kc if per_group else Kc, C))).astype(np.float32)
    given = (0.2 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    out = dict(mu=mu, A=A, beta=beta, given=given, center=mu.astype(np.float64).mean(0))
    for name, cen in (("mean", out["center"]), ("given", given.astype(np.float64))):
        dm = mu.astype(np.float64) - cen
        corr = np.einsum("gc,gkcn->gkn", dm, A.astype(np.float64).reshape(G, Kc, C, C))
        b64 = beta.astype(np.float64).reshape((G, Kc, C) if per_group else (1, Kc, C))
        out["bias_" + name] = (b64 - corr).reshape(G * Kc, C)
        out["nobeta_" + name] = (-corr).reshape(G * Kc, C)
    return out
