"""The fused spectral-norm op (csrc/wc_sn.hip) at every edge of its workgroup plan, its column and row slices, its
meeting state and its batched launches, against the float64 oracle (oracle.wc_oracle.spectral_normalize and
spectral_normalize_backward).

Shapes, matrix families, the warm start and the float32 precondition live in tests/spectral_reference.py; the bounds are
the suite's own (2e-5: relative for w_sn, sigma and dW, absolute for u and v).  The workgroup count a launch really used
is read from what it leaves behind: one non-zero maximum per workgroup behind wc_spectral_norm_amax_offset.

    PYTHONPATH=. python tests/test_spectral_edges_gpu.py        # the table of profiles/spectral_parity.txt

No test here makes the bounded wait of a meeting expire."""
import numpy as np
import pytest
import torch

import spectral_reference as S
from _poison import run_patterns

pytestmark = pytest.mark.gpu


def _ops():
    from wc_gan_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.detach().double().cpu().numpy()


def _ids(cases):
    return [f"{s[0]}x{s[1]}-{f}" for s, f in cases]


# ---- what a launch leaves in its workspace ------------------------------------------------------------------------------------
def _words(ws, R, K):
    """[error word, forward arrivals, forward done, backward arrivals, backward done]"""
    from wc_gan_amd import _lib
    off = _lib.load().wc_spectral_norm_error_offset(R, K)
    assert off + 32 == ws.numel()
    return ws[off:off + 4].view(torch.int32).tolist() + ws[-16:].view(torch.int32).tolist()


def _amax(ws, R, K):
    from wc_gan_amd import _lib
    off = _lib.load().wc_spectral_norm_amax_offset(R, K)
    return ws[off:ws.numel() - 16].view(torch.float32).cpu().numpy()


def _left_behind(ws, R, K, w_sn):
    """The per-workgroup maxima say how many workgroups ran (each owns at least one row, and no row of the families is
    zero): exactly plan(R, K) non-zero floats, zeros behind them up to the meeting words; their maximum is max |w_sn|
    bit for bit; the meeting words and the error word are zero.  Returns the observed workgroup count."""
    a = _amax(ws, R, K)
    n = int(np.count_nonzero(a))
    assert n == S.plan(R, K) and np.all(a[:n] > 0) and not a[n:].any(), (n, S.plan(R, K))
    assert a.max() == np.float32(w_sn.abs().max().item())
    assert _words(ws, R, K) == [0, 0, 0, 0, 0]
    return n


def _check_forward(got, ref, what=""):
    e = S.forward_errors(got, ref)
    assert all(x < S.BOUND for x in e.values()), (what, e)
    return e


# ---- a. every shape, family and iteration count ---------------------------------------------------------------------------------
def _measure(c, iterations, ws=None):
    """Forward twice and both backwards twice on one workspace; bit-identical repeats; the errors against the oracle."""
    ops = _ops()
    R, K = c.R, c.K
    W, g = _dev(c.W), _dev(c.g)
    ws = ops.spectral_norm_workspace(R, K, 'cuda') if ws is None else ws
    runs = []
    for rep in range(2):
        u, v = _dev(c.u0), _dev(c.v0)
        w_sn, sigma, uu, vv = ops.spectral_norm(W, u, v, iterations, ws, eps=c.eps, keep_uv=True)
        nwg = _left_behind(ws, R, K, w_sn)
        runs.append((w_sn, sigma, u, v, uu, vv))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the second launch on the same workspace differs"
    assert torch.equal(u, uu) and torch.equal(v, vv)                    # what sigma was taken with is what the buffers hold
    if iterations == 0:
        assert torch.equal(u, _dev(c.u0)) and torch.equal(v, _dev(c.v0))            # inference leaves u, v alone
    assert torch.equal(W, _dev(c.W)) and w_sn.stride() == W.stride()
    w_o, s_o, u_o, v_o, d_o = c.oracle(iterations)
    e = S.forward_errors((_host(w_sn), float(sigma), _host(u), _host(v)), (w_o, s_o, u_o, v_o))
    for fd in (True, False):
        d1 = ops.spectral_norm_bwd(g, w_sn, uu, vv, sigma, fd, ws)
        d2 = ops.spectral_norm_bwd(g, w_sn, uu, vv, sigma, fd, ws)
        assert torch.equal(d1, d2) and _words(ws, R, K) == [0, 0, 0, 0, 0]
        e["dW_full" if fd else "dW_const"] = c.dw_error(_host(d1), iterations, fd)
    return e, nwg


@pytest.mark.parametrize("shape,family", S.CASES, ids=_ids(S.CASES))
def test_forward_and_backward_at_every_edge(shape, family):
    c = S.case(*shape, family)
    for it in S.ITERATIONS:
        c.precondition(it)                      # a correct float32 kernel cannot fail what follows
        e, nwg = _measure(c, it)
        assert all(x < S.BOUND for x in e.values()), (shape, family, it, e)
        assert nwg == dict((s, n) for s, n, _ in S.TABLE)[shape]


# ---- b. the plan through the layers' view of the maxima ------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k", [(8, 16, 3), (32, 64, 3), (128, 128, 3), (64, 128, 1)])
def test_layers_see_one_maximum_per_workgroup(cin, cout, k):
    """SNConv2d.normalized_weight() hands the convolution `_wc_amax`: the same floats, for a channels-last 4-D weight."""
    from wc_gan_amd.spectral import SNConv2d
    torch.manual_seed(cin + cout)
    m = SNConv2d(cin, cout, k, padding=k // 2).cuda()
    R, K = cout, cin * k * k
    for train in (True, False, True):
        m.train(train)
        w = m.normalized_weight()
        a = w._wc_amax.cpu().numpy()
        n = S.plan(R, K)
        assert int(np.count_nonzero(a)) == n and np.all(a[:n] > 0) and not a[n:].any()
        assert a.max() == np.float32(w.detach().abs().max().item())
        assert _words(m._sn_workspace(), R, K) == [0, 0, 0, 0, 0]


# ---- c. state across launches on one workspace -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(33, 127), (1024, 513)])
def test_forward_and_backward_alternate_on_one_workspace(shape):
    """Forward and fully differentiable backward meet on different words of the same workspace, and the forward meets
    once, twice or 3k - 1 times: every step of the sequence finds the words zero and leaves them zero."""
    ops = _ops()
    R, K = shape
    c = S.case(R, K, "gauss")
    W, g = _dev(c.W), _dev(c.g)
    ws = ops.spectral_norm_workspace(R, K, 'cuda')
    u, v = _dev(c.u0), _dev(c.v0)
    for step, (it, fd) in enumerate([(3, True), (0, True), (1, False)]):
        # the oracle follows the same state: u, v move on with the launches (from the device's float32 values)
        u64, v64 = _host(u), _host(v)
        w_o, s_o, u_o, v_o = S.O.spectral_normalize(c.W, u64, v64, it)
        m = S.model_f32(c.W, u64, v64, it)
        assert all(x <= S.PRECONDITION for x in S.forward_errors(m, (w_o, s_o, u_o, v_o)).values())
        w_sn, sigma, uu, vv = ops.spectral_norm(W, u, v, it, ws, keep_uv=True)
        _left_behind(ws, R, K, w_sn)
        _check_forward((_host(w_sn), float(sigma), _host(u), _host(v)), (w_o, s_o, u_o, v_o), (step, it))
        dW = ops.spectral_norm_bwd(g, w_sn, uu, vv, sigma, fd, ws)
        assert _words(ws, R, K) == [0, 0, 0, 0, 0], (step, it, fd)
        d_o = S.O.spectral_normalize_backward(c.g, w_o, u_o, v_o, s_o, fd)
        assert S.rel(_host(dW), d_o) < S.BOUND, (step, it, fd)


# ---- d. eps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.EPS_SHAPES, ids=[f"{r}x{k}" for r, k in S.EPS_SHAPES])
def test_products_below_eps_are_divided_by_eps(shape):
    """eps = 1e-2 and a matrix scaled so that |W^T u| and |W v| stay below it: v = t / eps, u = s / eps and
    sigma = |s|^2 / eps (the kernel's n2 * inv_u; |s| itself would be > 100 times off, see the CPU file)."""
    c = S.eps_case(*shape)
    for it in (1, 2):
        c.precondition(it)
        e, _ = _measure(c, it)
        assert all(x < S.BOUND for x in e.values()), (shape, it, e)
        # u and v are not unit vectors here (1e-4 and smaller): the absolute bound says nothing, so relative as well
        u, v = _dev(c.u0), _dev(c.v0)
        w_sn, sigma = _ops().spectral_norm(_dev(c.W), u, v, it, _ops().spectral_norm_workspace(*shape, 'cuda'), eps=c.eps)
        _, _, u_o, v_o, _ = c.oracle(it)
        assert S.rel(_host(u), u_o) < S.BOUND and S.rel(_host(v), v_o) < S.BOUND
        assert bool(torch.isfinite(w_sn).all())


# ---- e. layouts ---------------------------------------------------------------------------------------------------------------------------
def _strided(a, strides):
    t = torch.empty_strided(a.shape, strides, dtype=a.dtype, device='cuda')
    t.copy_(a)
    return t


LAYOUTS = [((16, 8, 3, 3), (72, 1, 24, 8), (72, 9, 3, 1)),        # channels-last weight; the gradient arrives contiguous
           ((64, 32, 1, 1), (32, 1, 32, 32), (32, 1, 1, 1)),      # 1 x 1: two stride tuples, one memory order
           ((64, 32, 1, 1), (32, 1, 1, 1), (32, 1, 32, 32)),
           ((40, 72), (72, 1), (1, 40))]                          # 2-D weight; a column-major gradient


@pytest.mark.parametrize("shape,w_strides,g_strides", LAYOUTS)
def test_backward_takes_a_gradient_in_the_other_memory_format(shape, w_strides, g_strides):
    """The matrix is the weight in MEMORY order; dW comes back in w_sn's strides whatever the gradient's were, with
    the values of a gradient that was converted beforehand."""
    ops = _ops()
    rng = np.random.default_rng(shape[0] + len(shape))
    R = shape[0]; K = int(np.prod(shape[1:]))
    w = _strided(torch.from_numpy((rng.standard_normal(shape) / np.sqrt(K)).astype(np.float32)), w_strides)
    g_log = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    mat = (lambda t: t.permute(0, 2, 3, 1).reshape(R, K)) if len(shape) == 4 else (lambda t: t)
    Wm = mat(w).cpu().numpy()
    u0, v0 = S.warm_start(Wm, 5)
    ws = ops.spectral_norm_workspace(R, K, 'cuda')
    u, v = _dev(u0), _dev(v0)
    w_sn, sigma, uu, vv = ops.spectral_norm(w, u, v, 1, ws, keep_uv=True)
    assert w_sn.stride() == w.stride() == tuple(w_strides)
    w_o, s_o, u_o, v_o = S.O.spectral_normalize(Wm, u0, v0, 1)
    _check_forward((_host(mat(w_sn)), float(sigma), _host(u), _host(v)), (w_o, s_o, u_o, v_o))
    g_same, g_other = _strided(g_log, w_strides), _strided(g_log, g_strides)
    assert g_other.stride() == tuple(g_strides) != w_sn.stride() and torch.equal(g_same, g_other)
    for fd in (True, False):
        d_same = ops.spectral_norm_bwd(g_same, w_sn, uu, vv, sigma, fd, ws)
        d_other = ops.spectral_norm_bwd(g_other, w_sn, uu, vv, sigma, fd, ws)
        assert d_same.stride() == d_other.stride() == w_sn.stride()
        assert torch.equal(d_same, d_other)
        d_o = S.O.spectral_normalize_backward(mat(g_log).numpy(), w_o, u_o, v_o, s_o, fd)
        assert S.rel(_host(mat(d_other)), d_o) < S.BOUND
        # and the batched entry re-lays the gradient out the same way
        d_b, = ops.spectral_norm_bwd_batched([g_other], [w_sn], [uu], [vv], [sigma], [ws], fd)
        assert d_b.stride() == w_sn.stride() and torch.equal(d_b, d_same)


# ---- f. batched launches ------------------------------------------------------------------------------------------------------------------
ONE_WG = [(1, 7), (2, 50), (7, 585), (64, 64), (1, 257), (1, 1), (16, 256)]
MIXED = [(64, 64), (33, 127), (20000, 3), (130, 16000), (256, 512), (1024, 513), (1040, 2001), (1, 7), (7, 586), (100, 4133)]
_BATCH_CASES = {}


def _bcase(shape):
    if shape not in _BATCH_CASES:
        _BATCH_CASES[shape] = S.Case(*shape, "gauss")
    return _BATCH_CASES[shape]


def _batched_against_single_and_oracle(shapes, it):
    ops = _ops()
    cs = [_bcase(s) for s in shapes]
    for c in {id(c): c for c in cs}.values():
        c.precondition(it)
    W = [_dev(c.W) for c in cs]; g = [_dev(c.g) for c in cs]
    us = [_dev(c.u0) for c in cs]; vs = [_dev(c.v0) for c in cs]
    wss = [ops.spectral_norm_workspace(c.R, c.K, 'cuda') for c in cs]
    outs = ops.spectral_norm_batched(W, us, vs, wss, it)
    single = []
    for i, c in enumerate(cs):
        u1, v1, ws1 = _dev(c.u0), _dev(c.v0), ops.spectral_norm_workspace(c.R, c.K, 'cuda')
        one = ops.spectral_norm(W[i], u1, v1, it, ws1, keep_uv=True)
        single.append((one, ws1))
        assert all(torch.equal(a, b) for a, b in zip(outs[i], one)), (i, shapes[i])
        assert torch.equal(us[i], u1) and torch.equal(vs[i], v1), (i, shapes[i])
        _left_behind(wss[i], c.R, c.K, outs[i][0])
        w_o, s_o, u_o, v_o, _ = c.oracle(it)
        _check_forward((_host(outs[i][0]), float(outs[i][1]), _host(us[i]), _host(vs[i])), (w_o, s_o, u_o, v_o), (i, shapes[i]))
    for fd in (True, False):
        dWs = ops.spectral_norm_bwd_batched(g, [o[0] for o in outs], [o[2] for o in outs], [o[3] for o in outs],
                                            [o[1] for o in outs], wss, fd)
        for i, c in enumerate(cs):
            (w_sn, sigma, uu, vv), ws1 = single[i]
            assert torch.equal(dWs[i], ops.spectral_norm_bwd(g[i], w_sn, uu, vv, sigma, fd, ws1)), (i, shapes[i], fd)
            assert c.dw_error(_host(dWs[i]), it, fd) < S.BOUND, (i, shapes[i], fd)
            assert _words(wss[i], c.R, c.K) == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("it", [0, 2])
@pytest.mark.parametrize("count", [1, 16, 17, 32, 33])
def test_batched_launches_are_cut_at_sixteen_items(count, it):
    """One-workgroup items: residency never cuts, so launches hold 16, 16, ... and the rest; block b of a launch is
    item b of it (the first[] lookup's densest form)."""
    assert all(S.plan(*s) == 1 for s in ONE_WG)
    _batched_against_single_and_oracle([ONE_WG[i % len(ONE_WG)] for i in range(count)], it)


@pytest.mark.parametrize("it", [0, 2])
def test_batched_launch_of_mixed_plans(it):
    """Plans 1, 2, 15, 127, 32, 33, 128, 1, 2, 32 in one call.  The two items behind the LDS opt-in (81 KB for the
    20000 rows of u, 65.5 KB for the 16000 columns of v) are neither first nor last: the items around them run with
    their allocation, and at one 81 KB workgroup per CU the 373 workgroups are cut by residency, not by the item count."""
    assert [S.plan(*s) for s in MIXED] == [1, 2, 15, 127, 32, 33, 128, 1, 2, 32]
    lds = [S.lds_bytes(*s) for s in MIXED]
    assert lds[2] == 81052 and lds[3] == 65560 and max(lds[:2] + lds[4:]) < 48 * 1024
    _batched_against_single_and_oracle(MIXED, it)


@pytest.mark.parametrize("fully_diff", [False, True])
def test_batched_backward_skips_a_layer_whose_weight_was_not_used(fully_diff):
    """prepare_spectral normalises every layer; a layer the forward then leaves out gets no gradient (None, as when the
    layers run one by one: an optimizer skips it) and the others get their per-layer gradients."""
    import copy
    import torch.nn as nn
    from wc_gan_amd.spectral import SNConv2d, SNLinear, prepare_spectral
    torch.manual_seed(13)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            kw = dict(fully_diff_spectral=fully_diff)
            self.a = SNConv2d(8, 16, 3, padding=1, **kw); self.b = SNConv2d(16, 16, 1, **kw); self.c = SNLinear(16, 1, **kw)

        def forward(self, x, batched):
            if batched:
                prepare_spectral(self)
            return self.c(torch.relu(self.a(x)).mean(dim=(2, 3)))          # b is normalised but not used

    n1 = Net().cuda(); n2 = copy.deepcopy(n1)
    x = torch.randn(4, 8, 10, 10, device='cuda').contiguous(memory_format=torch.channels_last)
    for step in range(2):
        y1 = n1(x, True); y2 = n2(x, False)
        assert torch.equal(y1, y2)
        y1.sum().backward(); y2.sum().backward()
        assert n2.b.weight.grad is None and n1.b.weight.grad is None
        for name in ("a", "c"):
            g1, g2 = getattr(n1, name).weight.grad, getattr(n2, name).weight.grad
            assert g1 is not None and float((g1 - g2).abs().max()) <= 1e-5 * float(g2.abs().max())      # (MIOpen's weight gradient)
        assert torch.equal(n1.a.sn_u, n2.a.sn_u) and torch.equal(n1.c.sn_v, n2.c.sn_v)
        for m in (n1.a, n1.b, n1.c):
            assert _words(m._sn_workspace(), m.sn_u.numel(), m.sn_v.numel()) == [0, 0, 0, 0, 0]
        n1.zero_grad(); n2.zero_grad()


# ---- g. poisoned outputs and guard bands -----------------------------------------------------------------------------------------------
POISON_SHAPES = [(1, 1), (4097, 1), (20000, 3), (3, 2000), (1, 257)]


@pytest.mark.parametrize("it", [0, 2])
def test_edge_shapes_on_poisoned_and_guarded_memory(it):
    """Empty and ragged slices, the c0 loop's last pass and the 1 x 1 weight with every output allocated on 0x00, 0xFF
    and 0x7B inside guard bands: every output is written in full (the bits do not depend on the pattern) and nothing is
    written outside; the workspace is the documented torch.zeros contract."""
    ops = _ops()
    cs = [_bcase(s) for s in POISON_SHAPES]

    def run(P):
        W = [P.guarded(c.W) for c in cs]; g = [P.guarded(c.g) for c in cs]
        u = [P.guarded(c.u0) for c in cs]; v = [P.guarded(c.v0) for c in cs]
        u2 = [P.guarded(c.u0) for c in cs]; v2 = [P.guarded(c.v0) for c in cs]
        wss = [ops.spectral_norm_workspace(c.R, c.K, 'cuda') for c in cs]
        wss2 = [ops.spectral_norm_workspace(c.R, c.K, 'cuda') for c in cs]
        out = []
        for i in range(len(cs)):
            w_sn, sig, uu, vv = ops.spectral_norm(W[i], u[i], v[i], it, wss[i], keep_uv=True)
            out += [w_sn, sig, uu, vv, u[i], v[i]]
            out += [ops.spectral_norm_bwd(g[i], w_sn, uu, vv, sig, fd, wss[i]) for fd in (True, False)]
        batched = ops.spectral_norm_batched(W, u2, v2, wss2, it)
        for i, q in enumerate(batched):
            out += list(q) + [u2[i], v2[i]]
        for fd in (True, False):
            out += ops.spectral_norm_bwd_batched(g, [q[0] for q in batched], [q[2] for q in batched], [q[3] for q in batched],
                                                 [q[1] for q in batched], wss2, fd)
        out += [w[-48:].clone() for w in wss + wss2]
        return out

    r = run_patterns(run)[0xFF]
    n = len(cs)
    for i, c in enumerate(cs):
        c.precondition(it)
        w_o, s_o, u_o, v_o, d_o = c.oracle(it)
        single, bat = r[8 * i:8 * i + 8], r[8 * n + 6 * i:8 * n + 6 * i + 6]
        assert all(torch.equal(a, b) for a, b in zip(single[:6], bat))
        _check_forward((_host(single[0]), float(single[1]), _host(single[4]), _host(single[5])), (w_o, s_o, u_o, v_o), c.R)
        assert torch.equal(single[2], single[4]) and torch.equal(single[3], single[5])
        for k, fd in enumerate((True, False)):
            assert c.dw_error(_host(single[6 + k]), it, fd) < S.BOUND
            assert torch.equal(r[14 * n + k * n + i], single[6 + k])
    for tail in r[16 * n:]:
        assert not tail[-32:].any()                                      # the error word and the meeting words


if __name__ == '__main__':
    keys = ("w_sn", "sigma", "u", "v", "dW_full", "dW_const")
    print("the HIP op and the op's formulas in NumPy float32 (model) against the float64 oracle; bound 2e-5, precondition 5e-6")
    print(f"{'shape':<14}{'family':<10}{'it':>3}{'nwg':>5}{'plan':>5}  " + ''.join(f"{k:>10}" for k in keys) + "   |"
          + ''.join(f"{'m.' + k:>11}" for k in keys), flush=True)
    worst, worst_m = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    rows = [(s, f, S.ITERATIONS, S.case) for s, f in S.CASES] + [(s, "gauss*1e-4", (1, 2), lambda R, K, f: S.eps_case(R, K)) for s in S.EPS_SHAPES]
    for shape, family, its, make in rows:
        c = make(*shape, family)
        for it in its:
            m = c.model_errors(it)
            e, nwg = _measure(c, it)
            print(f"{str(shape):<14}{family:<10}{it:>3}{nwg:>5}{S.plan(*shape):>5}  " + ''.join(f"{e[k]:>10.1e}" for k in keys) + "   |"
                  + ''.join(f"{m[k]:>11.1e}" for k in keys), flush=True)
            for k in keys:
                worst[k] = max(worst[k], e[k]); worst_m[k] = max(worst_m[k], m[k])
    print(f"{'worst':<37}  " + ''.join(f"{worst[k]:>10.1e}" for k in keys) + "   |" + ''.join(f"{worst_m[k]:>11.1e}" for k in keys))
