"""GPU tests of the renorm ('dr') route: the C x C stage (wc_renorm_f64) and its K5 (wc_bwd_factor_renorm_f64)
at the C ABI on poisoned, guard-banded device memory (tests/_poison.py), the site through create_norm('dr', ...) against the float64
oracle (oracle.wc_oracle.wc_forward_renorm / wc_backward_renorm, 1e-4 relative max-norm), the planes route behind
functional.residual_add(planes=True), and a captured graph against the eager site."""
import functools

import numpy as np
import pytest
import torch

from oracle import wc_oracle as o
import renorm_reference as rr
from _poison import run_patterns

pytestmark = pytest.mark.gpu
EPS = 1e-3
TOL = 1e-4          # the project's contract against float64, fp32 path


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


# ---- the C x C stage ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stage_case(C):
    """(moving_cov float32, L float64): the moments of one ill-conditioned draw, and the batch factor of another."""
    import scipy.linalg as sl
    rng = np.random.default_rng(4000 + C)
    _, mc = o.moments_to_stats(*o.batch_moments(o.synth_activation(rng, (2 * C, C), 'ill')))
    _, sb = o.moments_to_stats(*o.batch_moments(1.5 * o.synth_activation(rng, (3 * C, C), 'ill') - 0.3))
    L = np.ascontiguousarray(sl.cholesky((1 - EPS) * sb + EPS * np.eye(C), lower=True))
    return mc.astype(np.float32), L


# one tile, a tile count that is not a power of two, the last width of K2's phased kernel, the first beyond it, the maximum
@pytest.mark.parametrize("C", [32, 96, 256, 288, 1024])
def test_renorm_stage(C):
    from wc_gan_amd import ops
    mc, L = _stage_case(C)

    def call(P):
        mcd, Ld = P.guarded(mc), P.guarded(L)
        Wm, C0 = ops.renorm(mcd, Ld, EPS)
        Wm1, none = ops.renorm(mcd, None, EPS)                  # ... and in two halves, as a site calls it around K2
        Wm2, C02 = ops.renorm(None, Ld, EPS, Wm1)
        assert none is None and Wm2 is Wm1
        _, Lm, Wk2 = ops.factor(None, None, 1, C, EPS, 0.0, 1, False, torch.zeros(C, device="cuda"), mcd, mcd.device)
        return dict(Wm=Wm, C0=C0, Wm_halves=Wm1, C0_halves=C02, Lm=Lm, W_k2=Wk2)

    out = run_patterns(call)[0x7B]
    Wm, C0, Lm, Wk2 = (out[k].numpy() for k in ('Wm', 'C0', 'Lm', 'W_k2'))
    assert np.isfinite(Wm).all() and np.isfinite(C0).all()
    # the moving factor runs K2's evaluation-mode kernels themselves: the same bits, hence the same residual
    assert torch.equal(out['Wm'], out['W_k2'])
    assert torch.equal(out['Wm_halves'], out['Wm']) and torch.equal(out['C0_halves'], out['C0'])
    res, res_k2 = np.abs(Wm @ Lm - np.eye(C)).max(), np.abs(Wk2 @ Lm - np.eye(C)).max()
    print(C, "max|Wm Lm - I|", res, "K2's", res_k2)
    assert res <= 2.0 * res_k2
    # the product: the rounding bound of a float64 dot product of length C, in any order
    u = 2.0 ** -53
    gam = C * u / (1 - C * u)
    exact, bound = Wm @ L, gam * (np.abs(Wm) @ np.abs(L))
    over = np.abs(C0 - exact) - bound
    print(C, "max |C0 - Wm L| / bound", float((np.abs(C0 - exact) / np.maximum(bound, 1e-300)).max()))
    assert (over <= 0).all(), float(over.max())
    assert (np.triu(C0, 1) == 0).all() and (np.triu(Wm, 1) == 0).all()


def _k5_inputs(C, Kc, seed):
    import scipy.linalg as sl
    rng = np.random.default_rng(seed)
    mc, L = _stage_case(C)
    W = sl.solve_triangular(L, np.eye(C), lower=True)
    Wm = o.whitening_matrix(mc.astype(np.float64), EPS)[1]
    C0 = np.tril(Wm @ L)
    R = rng.standard_normal((Kc, C, C))
    gsum = rng.standard_normal((Kc, C))
    gamma = (rng.standard_normal((Kc, C, C)) / np.sqrt(C)).astype(np.float32)
    A = np.einsum('ji,kjo->kio', Wm, gamma.astype(np.float64)).astype(np.float32)
    return W, Wm, C0, R, gsum, gamma, A


@pytest.mark.parametrize("C,Kc", [(32, 1), (96, 3), (256, 1), (288, 2)])
def test_renorm_backward_factor(C, Kc):
    from wc_gan_amd import ops
    M, ddof = 4096, 1
    W, Wm, C0, R, gsum, gamma, A = _k5_inputs(C, Kc, 90 + C + Kc)

    def call(P):
        args = [P.guarded(a) for a in (R, gsum, W, Wm, C0, gamma, A)]
        dg, db, S, gm = ops.bwd_factor_renorm(*args, M, EPS, ddof, True)
        dg0, db0, S0, gm0 = ops.bwd_factor_renorm(*args, M, EPS, ddof, False)
        assert S0 is None and gm0 is None
        # C0 = I and Wm = W: the plain Cholesky site
        eye = P.guarded(np.eye(C))
        Ap = P.guarded(np.einsum('ji,kjo->kio', W, gamma.astype(np.float64)).astype(np.float32))
        plain = ops.bwd_factor_renorm(args[0], args[1], args[2], args[2], eye, args[5], Ap, M, EPS, ddof, True)
        k5 = ops.bwd_factor(args[0], args[1], args[2], args[2], args[5], Ap, M, EPS, ddof, True)
        return dict(dgamma=dg, dbeta=db, S=S, gmean=gm, dgamma_eval=dg0, dbeta_eval=db0,
                    **{f"plain{i}": t for i, t in enumerate(plain)}, **{f"k5{i}": t for i, t in enumerate(k5)})

    out = run_patterns(call)[0x7B]
    ref = rr.factor_backward(R, gsum, W, Wm, C0, gamma.astype(np.float64), A.astype(np.float64), M, EPS, ddof)
    errs = {}
    for name, r in zip(('dgamma', 'dbeta', 'S', 'gmean'), ref):
        got = out[name].numpy().astype(np.float64)
        assert np.isfinite(got).all(), name
        errs[name] = rel(got, r)
    for i, name in enumerate(('dgamma', 'dbeta', 'S', 'gmean')):
        errs['plain_' + name] = rel(out[f"plain{i}"].numpy(), out[f"k5{i}"].numpy())
    print(C, Kc, errs)
    assert all(v <= 1e-6 for v in errs.values()), errs
    # evaluation mode: the parameter gradients are the training call's
    assert torch.equal(out['dgamma_eval'], out['dgamma']) and torch.equal(out['dbeta_eval'], out['dbeta'])


def test_renorm_backward_factor_eval_mode_leaves_S_and_gmean_alone():
    """training == 0 at the C ABI, with S and gmean given: both keep the pattern they were filled with."""
    from wc_gan_amd import _lib
    C, Kc = 96, 3
    lib = _lib.load()
    W, Wm, C0, R, gsum, gamma, A = _k5_inputs(C, Kc, 7)
    # row-major on the device: scipy's triangular solve returns column-major arrays, and torch.tensor keeps their strides
    d = [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in (R, gsum, W, Wm, C0, gamma, A)]
    assert all(t.is_contiguous() for t in d)
    dg = torch.empty(Kc, C, C, device="cuda"); db = torch.empty(Kc, C, device="cuda")
    S = torch.full((C, C), 123.25, device="cuda"); gm = torch.full((C,), -7.5, device="cuda")
    nb = lib.wc_bwd_factor_renorm_workspace_bytes(C, Kc)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.wc_bwd_factor_renorm_f64(*[t.data_ptr() for t in d], Kc, C, 4096, EPS, 1, 0, dg.data_ptr(), db.data_ptr(),
                                      S.data_ptr(), gm.data_ptr(), ws.data_ptr(), nb, stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((S == 123.25).all()) and bool((gm == -7.5).all())
    assert rel(_np(dg), np.einsum('ij,kjo->kio', Wm, R)) <= 1e-6 and rel(_np(db), gsum) <= 1e-6


# ---- the site through the layers ----------------------------------------------------------------------------------------------------
def _stack(after_norm, C, K=5, seed=2):
    from wc_gan_amd.generator import create_norm
    torch.manual_seed(seed)
    stack = create_norm('dr', after_norm, number_of_classes=K)(axis=-1, name='s', channels=C).cuda()
    for p in stack.parameters():
        torch.nn.init.normal_(p, std=0.3)
    return stack


@functools.lru_cache(maxsize=None)
def _site_case(after_norm, shape, scale, seed=8):
    """Host inputs of a site: moving statistics that differ from the batch's (the batch is `scale` times wider and shifted)."""
    rng = np.random.default_rng(seed)
    N, C = shape[0], shape[-1]
    mm, mc = o.moments_to_stats(*o.batch_moments(o.synth_activation(rng, (40 * C, C), "well")))
    x = (scale * o.synth_activation(rng, shape, "well") + 0.1).astype(np.float32)
    cls = rng.integers(0, 5, (N, 1)).astype(np.int32)
    gy = rng.standard_normal(shape).astype(np.float32)
    return mm.astype(np.float32), mc.astype(np.float32), x, cls, gy


def _site_errors(stack, after_norm, xin, leaves, x_ref, mm, mc, cls, gy, relu, planes=False):
    """Forward + backward of the stack on xin (a tensor or a pre-split handle; `leaves`: the tensors whose gradient is dx) against the
    oracle's renorm on x_ref.  A ReLU'd site is judged on the mask its own output has, as everywhere in this suite."""
    C = x_ref.shape[-1]
    stack.npart.moving_mean.copy_(dev(mm).view(C, 1)); stack.npart.moving_cov.copy_(dev(mc))
    clsd = dev(cls, torch.int32)
    gamma, beta, slot, _ = stack.coloring_table(xin, clsd)
    Gn, Bn = _np(gamma), (None if beta is None else _np(beta))
    sn = None if slot is None else _np(slot)
    y = stack(xin, clsd, relu=relu, planes=planes)
    pl = getattr(y, '_wc_planes', None)
    y.backward(dev(gy))
    torch.cuda.synchronize()
    yn = _np(y) if pl is None else _np((pl[0].double() + pl[1].double()) / float(pl[2][0]))
    y_ref, cache = o.wc_forward_renorm(x_ref, Gn, Bn, sn, moving_mean=mm.astype(np.float64), moving_cov=mc.astype(np.float64))
    gm = gy.astype(np.float64) * (yn > 0) if relu else gy
    dx_ref, dG_ref, dB_ref = o.wc_backward_renorm(gm, cache)
    errs = dict(y=rel(yn, np.maximum(y_ref, 0.0) if relu else y_ref), mc=rel(_np(stack.npart.moving_cov), cache['moving_cov']))
    for name, (leaf, fold) in leaves.items():
        errs[name] = rel(_np(leaf.grad), fold(dx_ref))
    if after_norm == 'uconv':
        br = stack.branches[0]
        errs['dG'] = rel(_np(br.kernel.grad).reshape(C, C), dG_ref[0])
        errs['dB'] = rel(_np(br.bias.grad), dB_ref[0])
    if after_norm == 'ucconv':
        cb, ub = stack.branches
        errs['dG_c'] = rel(_np(cb.kernel.grad), dG_ref)
        errs['dG_u'] = rel(_np(ub.kernel.grad).reshape(C, C), dG_ref.sum(0))
    return errs, pl is not None


# fewer rows than channels; a class table; the first width behind K2's phased kernel; a padded width (C = 48 -> 64)
SITES = [('uconv', (4, 2, 2, 64)), ('ucconv', (12, 6, 6, 32)), ('uconv', (8, 4, 4, 288)), ('uconv', (6, 4, 4, 48))]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("after_norm,shape", SITES, ids=[f"{a}-{'x'.join(map(str, s))}" for a, s in SITES])
def test_renorm_site_matches_the_oracle(after_norm, shape, relu):
    mm, mc, x, cls, gy = _site_case(after_norm, shape, 1.3)
    stack = _stack(after_norm, shape[-1])
    xt = dev(x).requires_grad_(True)
    errs, _ = _site_errors(stack, after_norm, xt, dict(dx=(xt, lambda d: d)), x, mm, mc, cls, gy, relu)
    print(after_norm, shape, relu, errs)
    assert all(v < TOL for v in errs.values()), errs


def test_renorm_site_hands_planes_over_when_the_batch_is_eight_times_the_moving_scale():
    """The planes-out hand-off predicts the output's scale from the coloring alone (a whitened input has unit variance); W_m (x - mu) of
    a batch 8 x as wide as the moving statistics has not: the gated redo of the hand-off is what keeps the planes inside fp16."""
    from wc_gan_amd.functional import conv_handoff_supported
    after_norm, shape = 'uconv', (16, 8, 8, 256)
    assert conv_handoff_supported(shape, True)
    mm, mc, x, cls, gy = _site_case(after_norm, shape, 8.0)
    stack = _stack(after_norm, shape[-1])
    xt = dev(x).requires_grad_(True)
    errs, handed = _site_errors(stack, after_norm, xt, dict(dx=(xt, lambda d: d)), x, mm, mc, cls, gy, True, planes=True)
    print(shape, errs)
    assert handed, "the site did not take the hand-off route"
    assert all(v < TOL for v in errs.values()), errs


# ---- planes in: a 'dr' site behind the residual add ------------------------------------------------------------------------------
K1_FAMILY = ("xtx", "xty_f16", "stats_", "colsum")          # the moments pass and its tails, whatever form it takes


def _profile_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key: e.count for e in prof.key_averages()}


# (128, 16, 16, C): the smallest shapes of tests/test_producer_gpu.py that functional.split_route_supported takes in training mode
@pytest.mark.parametrize("C,Kc,presummed", [(128, 1, True), (128, 3, False), (256, 1, False), (256, 3, True)])
def test_renorm_site_on_the_planes_route(C, Kc, presummed):
    from wc_gan_amd.functional import residual_add, split_of, split_route_supported
    shape = (128, 16, 16, C)
    N, H, W_ = shape[:3]
    after_norm = 'uconv' if Kc == 1 else 'ucconv'
    assert split_route_supported(shape, True)
    mm, mc, x, cls, gy = _site_case(after_norm, shape, 1.3)
    cls = (cls % Kc).astype(np.int32)
    rng = np.random.default_rng(C + Kc)
    s = (0.5 * rng.standard_normal((N, H // 2, W_ // 2, C))).astype(np.float32)
    up = np.repeat(np.repeat(s, 2, axis=1), 2, axis=2)
    h = (x - up).astype(np.float32)
    xsum = (h + up).astype(np.float32)                # the fp32 sum the producer forms
    stack = _stack(after_norm, C, K=Kc)
    assert stack.takes_split(shape) and stack.npart.renorm and stack.npart.training
    ht, st_ = dev(h).requires_grad_(True), dev(s).requires_grad_(True)
    xh = residual_add(ht, st_, True, planes=True, x32=not stack.backward_takes_split(shape), stat_groups=1 if presummed else 0)
    st = split_of(xh)
    assert st is not None and (st.moments is not None) == presummed
    leaves = dict(dh=(ht, lambda d: d.reshape(shape)),
                  ds=(st_, lambda d: d.reshape(N, H // 2, 2, W_ // 2, 2, C).sum((2, 4))))
    errs, _ = _site_errors(stack, after_norm, xh, leaves, xsum, mm, mc, cls, gy, True)
    print(shape, Kc, presummed, errs)
    assert all(v < TOL for v in errs.values()), errs


@pytest.mark.parametrize("C", [128, 256])
def test_renorm_site_on_planes_launches_no_second_moments_pass(C):
    """A profiled forward + backward of the site behind the producer: the planes kernels run, and the K1 family (moments pass, its
    tails) is launched no more often than by the same site without renorm."""
    from wc_gan_amd.functional import residual_add
    shape = (128, 16, 16, C)
    mm, mc, x, cls, gy = _site_case('uconv', shape, 1.3)
    counts = {}
    for renorm in (True, False):
        stack = _stack('uconv', C)
        stack.npart.renorm = renorm
        stack.npart.moving_mean.copy_(dev(mm).view(C, 1)); stack.npart.moving_cov.copy_(dev(mc))
        assert stack.takes_split(shape)
        h, gyd = dev(x).requires_grad_(True), dev(gy)
        zero = torch.zeros(shape, device="cuda")

        def step():
            xh = residual_add(h, zero, False, planes=True, x32=not stack.backward_takes_split(shape))
            stack(xh, None, relu=True).backward(gyd)

        counts[renorm] = _profile_kernels(step)
    names = " ".join(counts[True])
    assert "apply_split_kernel" in names, names[:2000]
    assert "tri_gemm_kernel" in names and "tri_gemm_kernel" not in " ".join(counts[False])
    fam = lambda c: {k: n for k, n in c.items() if any(t in k for t in K1_FAMILY)}
    a, b = fam(counts[True]), fam(counts[False])
    print(a, b)
    assert b and sum(a.values()) <= sum(b.values()), (a, b)
    assert all(n <= b.get(k, 0) for k, n in a.items()), (a, b)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_renorm_site_replays_from_a_graph_bit_for_bit():
    after_norm, shape = 'uconv', (16, 8, 8, 64)
    C = shape[-1]
    mm, mc, x, cls, gy = _site_case(after_norm, shape, 1.3)
    rng = np.random.default_rng(3)
    inputs = [dev(x), dev((0.7 * o.synth_activation(rng, shape, "well") - 0.2).astype(np.float32))]
    stack = _stack(after_norm, C)
    gyd = dev(gy)

    def reset():
        stack.npart.moving_mean.copy_(dev(mm).view(C, 1)); stack.npart.moving_cov.copy_(dev(mc))

    def step(xt):
        y = stack(xt, None, relu=True)
        (dx,) = torch.autograd.grad(y, [xt], gyd)
        return y, dx

    eager = []
    reset()
    for xi in inputs:               # the moving statistics evolve from call to call: the replays below repeat this sequence
        y, dx = step(xi.clone().requires_grad_(True))
        eager.append((y.detach().clone(), dx.clone(), stack.npart.moving_cov.clone()))
    buf = inputs[0].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, dx_g = step(buf)
    reset()
    for xi, (y_e, dx_e, mc_e) in zip(inputs, eager):
        with torch.no_grad():
            buf.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_g.detach(), y_e) and torch.equal(dx_g, dx_e) and torch.equal(stack.npart.moving_cov, mc_e)
