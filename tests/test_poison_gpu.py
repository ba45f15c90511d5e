"""The HIP path on poisoned and guard-banded device memory (tests/_poison.py).

Every torch.empty / empty_like / empty_strided / new_empty the wrappers make comes back filled with 0x00, 0xFF (NaN, -1) or 0x7B (large
but finite, a large positive counter), inside guard bands of the same pattern.  For each case: (a) the outputs are bit-identical across
the three patterns -- the kernels are deterministic, so a difference is a word read before the call wrote it; (b) every guard byte is
intact -- no tail tile read-modify-wrote past the end of a tensor; (c) under 0xFF the result matches the float64 oracle at the
tolerance of the existing test of that op."""
import numpy as np
import pytest
import torch

from oracle import wc_oracle as o

from _poison import PATTERNS, Poison, run_patterns, same_bits

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.99


def rel(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    if a.shape != b.shape and a.size == b.size:           # (C,) against (C, 1)
        a, b = a.reshape(-1), b.reshape(-1)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _ops():
    from wc_gan_amd import ops
    return ops


# ---- the harness itself ----------------------------------------------------------------------------------------------------
def _raw(a):
    n = a.numel() * a.element_size()
    return torch.empty(0, dtype=torch.uint8, device=a.device).set_(a.untyped_storage(), a.storage_offset() * a.element_size(), (n,))


def test_harness_poisons_guards_and_reports_the_site():
    from wc_gan_amd import ops
    x = torch.randn(4, 8, device="cuda")
    for p in PATTERNS:
        with Poison(p) as P:
            t = torch.empty(3, 5, device="cuda")
            u = torch.empty_like(x)
            v = x.new_empty((7,))
            w = torch.empty_like(torch.empty(2, 128, 4, 4, device="cuda"), memory_format=torch.channels_last)
            z = torch.zeros(9, device="cuda")
            m = torch.empty(5, device="meta")
            torch.cuda.synchronize()
            for a in (t, u, v, w):
                assert bool((_raw(a) == p).all())
            assert bool((z == 0).all()) and m.is_meta
            assert t.data_ptr() % 512 == 0 and not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last)
            ws = ops._workspace(100, x.device)              # an allocation inside the package: its site is named
            P.check_guards()
            # a write one byte past the end is caught and names the allocating line (the view's storage is the guarded buffer)
            raw = torch.empty(0, dtype=torch.uint8, device="cuda").set_(ws.untyped_storage(), ws.storage_offset() + ws.numel(), (1,))
            raw.fill_(p ^ 1)
            with pytest.raises(AssertionError, match="ops.py"):
                P.check_guards()


def test_harness_refills_pool_buffers_on_every_graph_replay():
    x = torch.randn(1024, device="cuda")
    with Poison(0x7B) as P:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t = torch.empty(1024, device="cuda")
            head = t[:512].clone()
            t[512:].copy_(x[512:])
        t[:512].fill_(1.0)                      # what a previous replay might have left
        g.replay()
        torch.cuda.synchronize()
        assert bool((head.view(torch.uint8) == 0x7B).all())
        P.check_guards()


# ---- stage tests -----------------------------------------------------------------------------------------------------------
def _ref_apply(x, mu, A, b, slot):
    N, C = x.shape[0], x.shape[-1]
    f = x.astype(np.float64).reshape(N, -1, C) - (0.0 if mu is None else mu.astype(np.float64))
    y = np.einsum('npc,nco->npo', f, A.astype(np.float64)[slot])
    return y if b is None else y + b.astype(np.float64)[slot][:, None, :]


# the edge shapes: row counts off the 128 / 256-row tiles, tiles that straddle samples of different slots, every channel width
SITE_CASES = [((3, 5, 7, 64), 1), ((5, 12, 12, 128), 3), ((8, 6, 6, 256), 1), ((128, 12, 12, 256), 7), ((16, 8, 8, 32), 2),
              ((9, 7, 5, 160), 1), ((6, 10, 6, 224), 2), ((17, 32, 32, 256), 1), ((33, 24, 24, 128), 1), ((64, 16, 16, 64), 4)]


def _site_inputs(shape, Kc, seed, cond="well"):
    rng = np.random.default_rng(seed)
    N, C = shape[0], shape[-1]
    x = o.synth_activation(rng, shape, cond).astype(np.float32)
    G, B = o.synth_coloring(rng, C, Kc)
    slot = rng.integers(0, Kc, N).astype(np.int32)
    gy = (rng.standard_normal(shape) * 1e-2).astype(np.float32)
    return x, G.astype(np.float32), B.astype(np.float32), slot, gy


@pytest.mark.parametrize("shape,Kc", SITE_CASES)
def test_forward_and_backward_stages(shape, Kc):
    """K1 / K2 (stats + factor, whiten, the flat form), color with the apply plan, K3 (fp32, ReLU, ReLU + bit mask), K4 in every form
    (plain, relu_y, mask, bits, flat), K5, K6 (fast, scaled, bits)."""
    ops = _ops()
    x, G, B, slot, gy = _site_inputs(shape, Kc, 3)
    N, C = shape[0], shape[-1]
    M = x.size // C
    bits_ok = ops.bwd_bits_supported(shape, Kc > 1) and M % 32 == 0
    mask_ok = M % 32 == 0

    def run(P):
        xd, Gd, Bd, gyd = P.guarded(x), P.guarded(G), P.guarded(B), P.guarded(gy)
        sd = P.guarded(slot) if Kc > 1 else None
        mm, mc = P.guarded(np.zeros(C, np.float32)), P.guarded(np.eye(C, dtype=np.float32))
        x2 = xd.view(M, C)
        s, xtx = ops.stats(x2)
        s2, xtx2, flat = ops.stats(x2, flat=True)
        mu, L, W, cs = ops.factor(s, xtx, M, C, EPS, MOM, 1, True, mm, mc, xd.device, want_scale=True)
        mu2, L2, W2, cs2 = ops.whiten(x2, EPS, MOM, 1, None, None)
        A, At, plan = ops.color(W, Gd, cs)
        A0, At0 = ops.color(W, Gd)
        y = ops.apply(xd, mu, A, Bd, sd, plan=plan)
        y_exact = ops.apply(xd, mu, A, Bd, sd, fast=False)
        yr = ops.apply(xd, mu, A, Bd, sd, plan=plan, relu=True)
        out = dict(s=s, xtx=xtx, flat=flat, mu=mu, L=torch.tril(L), W=W, cs=cs, mm=mm, mc=mc, mu2=mu2, W2=W2, cs2=cs2, A=A, At=At, A0=A0,
                   At0=At0, y=y, y_exact=y_exact, yr=yr)
        R, gsum = ops.bwd_reduce(xd, mu, gyd, sd, Kc)
        Rf, gf, buf, sc = ops.bwd_reduce(xd, mu, gyd, sd, Kc, flat=True, want_scales=True)
        Rr, gr, gmr, scr = ops.bwd_reduce(xd, mu, gyd, sd, Kc, want_scales=True, relu_y=yr)
        dG, dB, S, gmean = ops.bwd_factor(R, gsum, W, L, Gd, A, M, EPS, 1, True)
        dx = ops.bwd_apply(gyd, xd, mu, At, S, gmean, sd)
        dx_sc = ops.bwd_apply(gyd, xd, mu, At, S, gmean, sd, scales=sc)
        dx_exact = ops.bwd_apply(gyd, xd, mu, At, S, gmean, sd, fast=False)
        out.update(R=R, gsum=gsum, buf=buf, sc=sc, Rr=Rr, gr=gr, gmr=gmr, scr=scr, dG=dG, dB=dB, S=S, gmean=gmean, dx=dx, dx_sc=dx_sc,
                   dx_exact=dx_exact)
        if mask_ok:
            ym, mask = ops.apply(xd, mu, A, Bd, sd, plan=plan, relu=True, want_mask=True)
            Rm, gm_, gmm, scm = ops.bwd_reduce(xd, mu, gyd, sd, Kc, want_scales=True, relu_mask=mask)
            out.update(ym=ym, mask=mask, Rm=Rm, gm_=gm_, gmm=gmm, scm=scm, rmb=ops.relu_mask_bits(gyd, mask))
            if bits_ok:
                Rb, gb, scb = ops.bwd_reduce(xd, mu, gyd, sd, Kc, want_scales=True, relu_mask=mask, write_masked=False)
                out.update(Rb=Rb, gb=gb, scb=scb, dxb=ops.bwd_apply(gyd, xd, mu, At, S, gmean, sd, scales=scb, relu_mask=mask))
        return out

    t = run_patterns(run)[0xFF]
    # (c) the float64 oracle, at the existing tests' tolerances
    X = x.reshape(-1, C).astype(np.float64)
    s_ref, xtx_ref, _ = o.batch_moments(X)
    _, cov_ref = o.moments_to_stats(s_ref, xtx_ref, M)
    _, cov = o.moments_to_stats(t['s'].numpy(), t['xtx'].numpy(), M)
    assert rel(t['s'], s_ref) < 1e-5 and rel(cov, cov_ref) < 1e-7                     # test_fast_gpu.test_fast_stats_matches_float64
    assert same_bits(t['mu'], t['mu2']) and same_bits(t['W'], t['W2']) and same_bits(t['cs'], t['cs2'])
    assert torch.equal(t['flat'][:C], t['s']) and torch.equal(t['flat'][C:].view(C, C), t['xtx'])
    y_ref, cache = o.wc_forward(x, G, B, slot, moving_mean=np.zeros(C), moving_cov=np.eye(C))
    assert rel(t['y'], y_ref.reshape(shape)) < 1e-4 and rel(t['yr'], np.maximum(y_ref, 0).reshape(shape)) < 1e-4     # TOL of test_layers_gpu
    A_np, mu_np = t['A'].numpy(), t['mu'].numpy()
    ref = _ref_apply(x, mu_np, A_np, B, slot)
    assert rel(t['y'].numpy().reshape(ref.shape), ref) < 3e-6 and rel(t['y_exact'].numpy().reshape(ref.shape), ref) < 3e-6   # test_fast_apply
    assert rel(t['mm'], cache['moving_mean']) < 1e-4 and rel(t['mc'], cache['moving_cov']) < 1e-4
    f = x.astype(np.float64).reshape(N, -1, C) - mu_np.astype(np.float64)
    g = gy.astype(np.float64).reshape(N, -1, C)
    for k in range(Kc):
        sel = slot == k
        if not sel.any():
            continue
        R_ref = np.einsum('npi,npj->ij', f[sel], g[sel])
        nat = np.sqrt(np.outer((f[sel] ** 2).sum((0, 1)), (g[sel] ** 2).sum((0, 1)))) + 1e-300
        assert np.abs((t['R'][k].numpy() - R_ref) / nat).max() < 1e-7                     # test_fast_bwd_reduce_matches_float64
        assert rel(t['gsum'][k], g[sel].sum((0, 1))) < 1e-5
    dx_ref = np.einsum('npc,nco->npo', g, t['At'].numpy().astype(np.float64)[slot]) + f @ t['S'].numpy().astype(np.float64) \
        - t['gmean'].numpy().astype(np.float64)
    for k in ('dx', 'dx_exact'):
        assert rel(t[k].numpy().reshape(dx_ref.shape), dx_ref) < 3e-6                      # test_fast_bwd_apply_matches_float64
    dx_o, dG_o, dB_o = o.wc_backward(gy, cache)
    assert rel(t['dx'], dx_o.reshape(shape)) < 1e-4 and rel(t['dG'], dG_o) < 1e-4 and rel(t['dB'], dB_o) < 1e-4
    if mask_ok:
        g_ref = np.where(~(t['ym'].numpy() <= 0), gy, np.float32(0))
        assert np.array_equal(t['gmm'].numpy(), g_ref) and np.array_equal(t['rmb'].numpy(), g_ref)


@pytest.mark.parametrize("shape,groups,Kc", [((12, 6, 6, 96), 3, 1), ((40, 8, 8, 64), 5, 2), ((16, 8, 8, 256), 2, 3),
                                             ((320, 8, 8, 256), 5, 1), ((10, 7, 5, 128), 5, 3)])
def test_grouped_stages(shape, groups, Kc):
    """Statistic groups: stats / factor / whiten with groups, color for the groups' tables, group_bias, group_bias_centered, and the
    grouped forward (whiten_color_grouped) on the fp32 route."""
    ops = _ops()
    from wc_gan_amd.functional import whiten_color_grouped
    x, G, B, slot, _ = _site_inputs(shape, Kc, 7)
    N, C = shape[0], shape[-1]
    M = x.size // C

    def run(P):
        xd, Gd, Bd = P.guarded(x), P.guarded(G), P.guarded(B)
        sd = P.guarded(slot) if Kc > 1 else None
        mm, mc = P.guarded(np.zeros(C, np.float32)), P.guarded(np.eye(C, dtype=np.float32))
        s, xtx = ops.stats(xd.view(M, C), groups)
        mu, L, W, cs = ops.factor(s, xtx, M // groups, C, EPS, MOM, 1, True, mm, mc, xd.device, want_scale=True, groups=groups)
        mu2, L2, W2, cs2 = ops.whiten(xd.view(M, C), EPS, MOM, 1, None, None, groups)
        A, At, plan = ops.color(W, Gd, cs, groups=groups)
        center, bias = ops.group_bias(mu, A, Bd, groups, Kc)
        bias_c = ops.group_bias_centered(mu, A, Bd, center, groups, Kc)
        y = whiten_color_grouped(xd, groups, Gd, Bd, sd, None, None)
        yr = whiten_color_grouped(xd, groups, Gd, Bd, sd, None, None, relu=True)
        return [s, xtx, mu, torch.tril(L), W, cs, mm, mc, mu2, W2, cs2, A, At, center, bias, bias_c, y, yr]

    r = run_patterns(run)[0xFF]
    s, xtx, mu, W, W2, y, yr = r[0], r[1], r[2], r[4], r[9], r[16], r[17]
    assert same_bits(W, W2)
    xg = x.reshape(groups, -1, C)
    sg = shape[0] // groups
    for gi in range(groups):
        X = xg[gi].astype(np.float64)
        assert rel(s[gi], X.sum(0)) < 1e-5
        _, cov_ref = o.moments_to_stats(X.sum(0), X.T @ X, X.shape[0])
        _, cov = o.moments_to_stats(s[gi].numpy(), xtx[gi].numpy(), X.shape[0])
        assert rel(cov, cov_ref) < 1e-7
        xs = x[gi * sg:(gi + 1) * sg]
        y_ref, _ = o.wc_forward(xs, G, B, slot[gi * sg:(gi + 1) * sg])
        assert rel(y[gi * sg:(gi + 1) * sg], y_ref.reshape(xs.shape)) < 1e-4                 # test_layers_gpu TOL
        assert rel(yr[gi * sg:(gi + 1) * sg], np.maximum(y_ref, 0).reshape(xs.shape)) < 1e-4


@pytest.mark.parametrize("shape,Kc", [((128, 32, 32, 256), 1), ((128, 16, 16, 256), 10), ((64, 16, 16, 128), 3), ((128, 12, 12, 256), 7),
                                      ((16, 8, 8, 256), 1), ((32, 16, 16, 128), 1)])
def test_planes_stages(shape, Kc):
    """The pre-split route: split_scales / split / unsplit, stats_split, whiten_split, color_split, split_bias, out_scale, apply_split with
    every epilogue, apply_planes, bwd_reduce_xsplit / bwd_apply_xsplit, resadd, resadd_split, resadd_stats_split with whiten_presummed /
    stats_presummed, patch_sum, fold / unfold_channel_scale."""
    ops = _ops()
    x, G, B, slot, gy = _site_inputs(shape, Kc, 11, cond="well")
    N, H, Wd, C = shape
    M = x.size // C
    rng = np.random.default_rng(12)
    s_half = (0.5 * rng.standard_normal((N, H // 2, Wd // 2, C))).astype(np.float32)
    h = (x - np.repeat(np.repeat(s_half, 2, axis=1), 2, axis=2)).astype(np.float32)
    w1 = (rng.standard_normal((128, C)) / np.sqrt(C)).astype(np.float32)
    b1 = rng.standard_normal(128).astype(np.float32)
    assert ops.apply_split_supported(shape)
    stats_ok = ops.resadd_stats_supported(shape, True)
    xsplit_ok = ops.bwd_xsplit_supported(shape, Kc > 1)
    planes_ok = ops.apply_planes_supported(shape)

    ss_ok = ops.stats_split_supported(M, C)

    def run(P):
        xd, Gd, Bd, gyd, hd, sd_ = P.guarded(x), P.guarded(G), P.guarded(B), P.guarded(gy), P.guarded(h), P.guarded(s_half)
        sl = P.guarded(slot) if Kc > 1 else None
        out = {}
        out['c'], out['sc'], fl = ops.split_scales(xd)
        out['fl'] = fl[:1]
        xs = ops.split(xd)
        out['planes'], out['back'] = xs.planes, ops.unsplit(xs)
        if ss_ok:
            out['s'], out['xtx'] = ops.stats_split(xs)
            mu, L, W = ops.whiten_split(xs, EPS, MOM, 1, None, None)
        else:                       # (K1 on these planes has no kernel: the statistics from the fp32 tensor)
            mu, L, W, _ = ops.whiten(xd.view(M, C), EPS, MOM, 1, None, None)
        out.update(mu=mu, L=torch.tril(L), W=W)
        A, At, plan, be = ops.color_split(W, Gd, xs, mu, Bd)
        A2, At2, plan2 = ops.color(W, Gd, xs.scale)
        out.update(A=A, At=At, be=be, A2=A2, be2=ops.split_bias(A2, Bd, xs, mu))
        out['y'] = ops.apply_split(xs, None, A, be, sl, plan=plan, folded=True)
        out['y2'] = ops.apply_split(xs, mu, A2, Bd, sl, plan=plan2)
        out['y3'] = ops.apply_split(xs, mu, A2, Bd, sl)                     # tables built inside the call
        out['yr'], mask = ops.apply_split(xs, None, A, be, sl, plan=plan, relu=True, folded=True, want_mask=True)
        rec = ops.out_scale(Gd, Bd, C, xd.device)
        out['pl'], rec, out['pmask'] = ops.apply_split(xs, None, A, be, sl, plan=plan, relu=True, folded=True, want_mask=True, oscale=rec)
        out.update(mask=mask, rec=rec[:1])
        if planes_ok:
            mu32, L32, W32, cs32 = ops.whiten(xd.view(M, C), EPS, MOM, 1, None, None)
            A32, At32, plan32 = ops.color(W32, Gd, cs32)
            rec2 = ops.out_scale(Gd, Bd, C, xd.device)
            out['pl2'], rec2, out['m2'] = ops.apply_planes(xd, mu32, A32, Bd, sl, plan32, rec2, relu=True, want_mask=True)
            out['rec2'] = rec2[:1]
        if xsplit_ok:
            R, gsum, scs = ops.bwd_reduce_xsplit(xs, mu, gyd, sl, Kc, relu_mask=mask if C == 256 else None)
            _, _, S, gmean = ops.bwd_factor(R, gsum, W, L, Gd, A, M, EPS, 1, True)
            # (scales [0, C) are not written: x's scales are the planes' -- include/wc_hip.h, wc_bwd_reduce_xsplit_f32)
            out.update(R=R, gsum=gsum, scs=scs[C:], S=S, gmean=gmean,
                       dxs=ops.bwd_apply_xsplit(gyd, xs, mu, At, S, gmean, sl, scs, relu_mask=mask if C == 256 else None))
        out['ra'] = ops.resadd(hd, sd_, up=True)
        r2 = ops.resadd_split(hd, sd_, up=True, want_x32=True)
        out.update(r2p=r2.planes, r2c=r2.center, r2s=r2.scale, r2f=r2.flag[:1], r2x=r2.x32, ps=ops.patch_sum(gyd))
        if stats_ok:
            r3 = ops.resadd_stats_split(hd, sd_, up=True, want_x32=True)
            mu3, L3, W3 = ops.whiten_presummed(r3, EPS, MOM, 1, None, None)
            s3, x3 = ops.stats_presummed(r3)
            out.update(r3p=r3.planes, r3s=r3.scale, r3f=r3.flag[:1], r3x=r3.x32, mu3=mu3, L3=torch.tril(L3), W3=W3, s3=s3, x3=x3)
        w1d, b1d = P.guarded(w1), P.guarded(b1)
        wf, bf = ops.fold_channel_scale(w1d, b1d, xs.scale, xs.center)
        out.update(wf=wf, bf=bf, uf=ops.unfold_channel_scale(wf, bf, xs.scale, xs.center))
        return out

    r = run_patterns(run)[0xFF]
    assert float((r['back'].double() - torch.from_numpy(x).double()).abs().max()) <= float(np.abs(x).max()) * 2.0 ** -20
    y_ref, _ = o.wc_forward(x, G, B, slot)
    assert rel(r['y'], y_ref.reshape(shape)) < 1e-4 and rel(r['y2'], y_ref.reshape(shape)) < 1e-4      # test_producer_gpu's 1e-4
    xsum = h.astype(np.float64) + np.repeat(np.repeat(s_half.astype(np.float64), 2, axis=1), 2, axis=2)
    assert np.array_equal(r['ra'].numpy(), (h + np.repeat(np.repeat(s_half, 2, axis=1), 2, axis=2)).astype(np.float32))   # bit for bit
    assert rel(r['r2x'], xsum) < 1e-6
    assert rel(r['ps'], gy.astype(np.float64).reshape(N, H // 2, 2, Wd // 2, 2, C).sum((2, 4))) < 1e-6


@pytest.mark.parametrize("E,C,K,Kc", [(3, 64, 6, 6), (4, 128, 10, 5), (2, 256, 3, 7), (5, 32, 7, 3), (3, 160, 4, 4), (15, 224, 200, 9)])
def test_factor_mix_and_its_gradient(E, C, K, Kc):
    ops = _ops()
    if not ops.factor_mix_supported(E, C):
        pytest.fail(f"factor_mix does not take E={E}, C={C}")
    rng = np.random.default_rng(E * C + K)
    D = rng.standard_normal((E, C, C)).astype(np.float32)
    al = rng.standard_normal((K, E)).astype(np.float32)
    idx = rng.integers(0, K, Kc).astype(np.int32)
    base = rng.standard_normal((C, C)).astype(np.float32)
    dout = rng.standard_normal((Kc, C, C)).astype(np.float32)

    def run(P):
        Dd, ad, idd, bd, dd = P.guarded(D), P.guarded(al), P.guarded(idx), P.guarded(base), P.guarded(dout)
        out = ops.factor_mix(Dd, ad, idd, bd)
        out0 = ops.factor_mix(Dd, ad)
        ddict, dal, db = ops.factor_mix_bwd(Dd, ad, idd, dd, want_base=True)
        return [out, out0, ddict, dal, db]

    out, out0, ddict, dal, db = run_patterns(run)[0xFF]
    ref = base.astype(np.float64) + np.einsum('te,ecd->tcd', al.astype(np.float64)[idx], D.astype(np.float64))
    assert rel(out, ref) <= 2e-6 and rel(out0, np.einsum('ke,ecd->kcd', al.astype(np.float64), D.astype(np.float64))) <= 2e-6   # test_mix_gpu
    dal_ref = np.zeros((K, E))
    np.add.at(dal_ref, idx, np.einsum('tcd,ecd->te', dout.astype(np.float64), D.astype(np.float64)))
    dd_ref = np.einsum('te,tcd->ecd', al.astype(np.float64)[idx], dout.astype(np.float64))
    assert rel(dal, dal_ref) <= 5e-6 and rel(ddict, dd_ref) <= 5e-6 and rel(db, dout.astype(np.float64).sum(0)) <= 5e-6


@pytest.mark.parametrize("shapes", [[(128, 128, 3, 3)], [(256, 128, 3, 3), (128, 3, 3, 3), (10, 256), (256, 256, 1, 1)]])
def test_spectral_norm_single_and_batched(shapes):
    """The spectral-norm ops on poisoned outputs; their workspace is the documented torch.zeros contract (not poisoned)."""
    ops = _ops()
    rng = np.random.default_rng(len(shapes))
    ws_np = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    us = [rng.standard_normal(s[0]).astype(np.float32) for s in shapes]
    vs = [rng.standard_normal(int(np.prod(s[1:]))).astype(np.float32) for s in shapes]
    gs = [rng.standard_normal(s).astype(np.float32) for s in shapes]

    def run(P):
        w = [P.guarded(a) for a in ws_np]
        u = [P.guarded(a) for a in us]; u2 = [P.guarded(a) for a in us]
        v = [P.guarded(a) for a in vs]; v2 = [P.guarded(a) for a in vs]
        g = [P.guarded(a) for a in gs]
        wss = [ops.spectral_norm_workspace(a.shape[0], a.numel() // a.shape[0], a.device) for a in w]
        wss2 = [ops.spectral_norm_workspace(a.shape[0], a.numel() // a.shape[0], a.device) for a in w]
        out = []
        single = [ops.spectral_norm(w[i], u[i], v[i], 1, wss[i], keep_uv=True) for i in range(len(w))]
        for i, (w_sn, sig, uu, vv) in enumerate(single):
            out += [w_sn, sig, uu, vv, u[i], v[i], ops.spectral_norm_bwd(g[i], w_sn, uu, vv, sig, True, wss[i])]
        batched = ops.spectral_norm_batched(w, u2, v2, wss2, 1)
        for q in batched:
            out += list(q)
        out += ops.spectral_norm_bwd_batched(g, [q[0] for q in batched], [q[2] for q in batched], [q[3] for q in batched],
                                             [q[1] for q in batched], wss2, True)
        return out

    r = run_patterns(run)[0xFF]
    n = len(shapes)
    for i in range(n):
        R = shapes[i][0]
        ref_w, ref_s, ref_u, ref_v = o.spectral_normalize(ws_np[i].reshape(R, -1), us[i], vs[i], 1)
        g64 = gs[i].reshape(R, -1).astype(np.float64)
        for w_sn, sig, dW in ((r[7 * i], r[7 * i + 1], r[7 * i + 6]), (r[7 * n + 4 * i], r[7 * n + 4 * i + 1], r[11 * n + i])):
            assert rel(w_sn.reshape(R, -1), ref_w) < 2e-5 and rel(sig, np.atleast_1d(ref_s)) < 2e-5                 # test_spectral's 2e-5
            assert rel(dW.reshape(R, -1), o.spectral_normalize_backward(g64, ref_w, ref_u, ref_v, ref_s, True)) < 2e-5


CONV_CASES = [('same', 2, 8, 8, 128, 128, 3), ('same', 8, 12, 12, 128, 256, 3), ('same', 4, 8, 8, 256, 128, 1),
              ('down', 32, 12, 12, 128, 256, 0), ('down', 2, 16, 16, 128, 128, 0), ('up', 2, 8, 8, 128, 128, 0), ('up', 32, 4, 4, 256, 256, 0),
              ('down3', 32, 12, 12, 128, 256, 3), ('up3', 8, 8, 8, 128, 128, 3), ('up3', 32, 4, 4, 256, 256, 3)]


@pytest.mark.parametrize("kind,N,H,W,ci,co,k", CONV_CASES)
def test_fast_conv_forward_and_gradients(kind, N, H, W, ci, co, k):
    from wc_gan_amd import conv as Cv
    import test_conv_gpu as tc
    g = torch.Generator().manual_seed(N + H + ci)
    x = (torch.randn(N, H, W, ci, generator=g) * 1.7 + 0.3)
    shape = (ci, co, 4, 4) if kind == 'up' else (co, ci, 4, 4) if kind == 'down' else (co, ci, k, k)
    w = torch.randn(*shape, generator=g) / (ci * shape[2] * shape[3]) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    Ho, Wo = (H // 2, W // 2) if kind.startswith('down') else (2 * H, 2 * W) if kind.startswith('up') else (H, W)
    gy = torch.randn(N, Ho, Wo, co, generator=g)

    class Site(torch.nn.Module):
        pass

    def run(P, site=None):
        xd = P.guarded(x).requires_grad_(True)
        wd = P.guarded(w).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bd = P.guarded(b).requires_grad_(True)
        assert Cv.supported(xd, wd, kind)
        p = Cv._plan(kind, xd, wd)
        y = Cv._FastConv.apply(xd, wd, bd, kind, p, False, None, site)
        dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), P.guarded(gy))
        return [y, dx, dw, db]

    y, dx, dw, db = run_patterns(run)[0xFF]
    # split_planes with a history record (a fresh site per pattern): the first call measures, the second takes the scale from the record
    hist = run_patterns(lambda P: (lambda site: run(P, site) + run(P, site))(Site().cuda().train()))[0xFF]
    xr, wr, br = x.double().cuda().requires_grad_(True), w.double().cuda().requires_grad_(True), b.double().cuda().requires_grad_(True)
    if kind in ('down3', 'up3'):
        xn = xr.permute(0, 3, 1, 2)
        if kind == 'down3':
            y64 = torch.nn.functional.avg_pool2d(torch.nn.functional.conv2d(xn, wr, br, padding=1), 2)
        else:
            y64 = torch.nn.functional.conv2d(torch.nn.functional.interpolate(xn, scale_factor=2, mode='nearest'), wr, br, padding=1)
        y64 = y64.permute(0, 2, 3, 1)
    else:
        y64 = tc._ref(xr, wr, br, kind)
    dx64, dw64, db64 = torch.autograd.grad(y64, (xr, wr, br), gy.double().cuda())
    for y_, dx_, dw_, db_ in ((y, dx, dw, db), hist[4:8]):
        assert tc._rel(y_.cuda(), y64) < tc.TOL and tc._rel(dx_.cuda(), dx64) < tc.TOL
        assert tc._rel(dw_.cuda(), dw64) < 2e-5 and tc._rel(db_.cuda(), db64) < tc.TOL


@pytest.mark.parametrize("shape,Cout", [((8, 8, 8, 128), 128), ((16, 16, 16, 256), 128), ((8, 12, 12, 256), 256)])
def test_split_conv_on_the_producers_planes(shape, Cout):
    from wc_gan_amd import conv as Cv
    from wc_gan_amd import functional as F
    ops = _ops()
    rng = np.random.default_rng(Cout + shape[0])
    N, H, W, C = shape
    h = rng.standard_normal(shape).astype(np.float32)
    s = (0.5 * rng.standard_normal((N, H // 2, W // 2, C))).astype(np.float32)
    w = (rng.standard_normal((Cout, C, 1, 1)) / np.sqrt(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    gy = rng.standard_normal((N, H, W, Cout)).astype(np.float32)
    assert ops.resadd_split_supported(shape) and Cv.takes_planes(shape, w.shape, 'same')

    def run(P):
        hd, sd = P.guarded(h).requires_grad_(True), P.guarded(s).requires_grad_(True)
        wd, bd = P.guarded(w).requires_grad_(True), P.guarded(b).requires_grad_(True)
        xh = F.residual_add(hd, sd, True, planes=True, x32=False)
        st = F.split_of(xh)
        assert st is not None
        y = Cv.split_conv(xh, st, wd, bd)
        grads = torch.autograd.grad(y, (hd, sd, wd, bd), P.guarded(gy))
        return [y] + list(grads)

    y, dh, ds, dw, db = run_patterns(run)[0xFF]
    xs = torch.from_numpy(h).double() + torch.from_numpy(np.repeat(np.repeat(s, 2, axis=1), 2, axis=2)).double()
    y64 = torch.einsum('nhwc,oc->nhwo', xs, torch.from_numpy(w[:, :, 0, 0]).double()) + torch.from_numpy(b).double()
    assert rel(y, y64) < 1e-5                                                                      # test_conv_gpu TOL
    dx64 = torch.einsum('nhwo,oc->nhwc', torch.from_numpy(gy).double(), torch.from_numpy(w[:, :, 0, 0]).double())
    assert rel(dh, dx64) < 1e-5 and rel(ds, dx64.reshape(N, H // 2, 2, W // 2, 2, C).sum((2, 4))) < 1e-5
    assert rel(dw[:, :, 0, 0], torch.einsum('nhwo,nhwc->oc', torch.from_numpy(gy).double(), xs)) < 2e-5
    assert rel(db, gy.astype(np.float64).sum((0, 1, 2))) < 1e-5


@pytest.mark.parametrize("N,H,W,C,O,k", [(8, 32, 32, 3, 128, 3), (5, 12, 12, 3, 128, 1), (4, 9, 7, 3, 256, 3), (3, 5, 11, 3, 128, 3)])
def test_narrow_convolution_forward_and_weight_gradients(N, H, W, C, O, k):
    from wc_gan_amd import conv as Cv
    g = torch.Generator().manual_seed(N * H + O)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(O, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(O, generator=g) * 0.1
    gy = torch.randn(N, H, W, O, generator=g)

    def run(P):
        xd, wd, bd, gd = P.guarded(x), P.guarded(w), P.guarded(b), P.guarded(gy)
        assert Cv.narrow_wrw_supported(xd, wd)
        y = Cv.narrow_forward(xd, wd, bd)
        wq = wd.clone().requires_grad_(True)
        bq = bd.clone().requires_grad_(True)
        yq = Cv.narrow_in_conv(xd, wq, bq)
        dw, db = torch.autograd.grad(yq, (wq, bq), gd)
        wo = P.guarded(torch.randn(C, O, k, k, generator=torch.Generator().manual_seed(1)))
        assert Cv.narrow_out_wrw_supported(gd, wo)
        dwo = Cv.narrow_out_weight_gradient(gd, xd, wo)
        return [y, yq, dw, db, dwo]

    y, yq, dw, db, dwo = run_patterns(run)[0xFF]
    assert same_bits(y, yq)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = torch.nn.functional.conv2d(xr.permute(0, 3, 1, 2), wr, br, padding=k // 2).permute(0, 2, 3, 1)
    dw64, db64 = torch.autograd.grad(y64, (wr, br), gy.double())
    assert rel(y, y64) < 1e-5 and rel(dw, dw64) < 2e-5 and rel(db, db64) < 1e-5
    # the narrow-output gradient: conv of gy (O -> C) whose output gradient is x
    gr = gy.double().requires_grad_(False)
    wo64 = torch.zeros(C, O, k, k, dtype=torch.float64, requires_grad=True)
    yo = torch.nn.functional.conv2d(gr.permute(0, 3, 1, 2), wo64, None, padding=k // 2).permute(0, 2, 3, 1)
    dwo64, = torch.autograd.grad(yo, (wo64,), x.double())
    assert rel(dwo, dwo64) < 2e-5


# ---- the existing constructions that force the gated exact redo, under each pattern --------------------------------------
REDO_TESTS = [
    ("test_fast_gpu", "test_fast_apply_out_of_range_tiles_take_the_exact_path", dict()),
    ("test_fast_gpu", "test_fast_bwd_apply_out_of_range_in_the_accumulating_pass", dict(shape=(16, 32, 32, 256))),
    ("test_fast_gpu", "test_fast_bwd_apply_out_of_range_in_the_accumulating_pass", dict(shape=(96, 32, 32, 64))),
    ("test_fast_gpu", "test_fast_reductions_out_of_range_take_the_exact_redo", dict(shape=(32, 32, 32, 256))),
    ("test_fast_gpu", "test_fast_reductions_out_of_range_take_the_exact_redo", dict(shape=(16, 64, 64, 64))),
    ("test_fast_gpu", "test_relu_backward_bits_route_redoes_out_of_range_tiles_exactly", dict()),
    ("test_producer_gpu", "test_apply_split_planes_gate_redoes_an_overflowing_pass", dict()),
    ("test_producer_gpu", "test_fused_producer_redoes_planes_and_moments_when_a_scale_was_too_tight", dict()),
    ("test_conv_gpu", "test_history_scaled_split_outside_its_window_is_split_again_with_the_measured_scale", dict()),
]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("module,name,kw", REDO_TESTS, ids=[f"{n}-{i}" for i, (_, n, _) in enumerate(REDO_TESTS)])
def test_redo_constructions_under_poison(module, name, kw, pattern):
    """The gated redo reads the gate words and what the fast kernel wrote: the existing test's own oracle assertions, on poisoned memory."""
    import importlib
    mod = importlib.import_module(module)
    fn = getattr(mod, name)
    if "ops" in fn.__code__.co_varnames[:fn.__code__.co_argcount]:
        kw = dict(kw, ops=_ops())
    with Poison(pattern) as P:
        fn(**kw)
        P.check_guards()


def _outlier_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) + 0.3).astype(np.float32)
    x[1, 2, 3, 5] = 4.0e7
    x[0, 0, 0, 9] = -6.0e7
    gy = (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    gy[2, 1, 0, 7] = 3.0e6
    gy[0, 0, 0, 11] = 2.0e5
    return x, gy


@pytest.mark.parametrize("shape", [(32, 32, 32, 256), (64, 32, 32, 128), (16, 64, 64, 64), (17, 32, 32, 256)])
def test_fast_reductions_redo_is_bit_identical_across_patterns(shape):
    """The gated exact redo of the fast K1 / K4 (and K6's accumulating pass) on poisoned memory: the same bits under every pattern."""
    ops = _ops()
    x, gy = _outlier_inputs(shape, 23)
    C = shape[-1]
    mu = x.reshape(-1, C).mean(0).astype(np.float32)
    rng = np.random.default_rng(1)
    At = (rng.standard_normal((1, C, C)) / np.sqrt(C)).astype(np.float32)
    S = (rng.standard_normal((C, C)) * 1e-4).astype(np.float32); S = (S + S.T) / 2
    gm = (rng.standard_normal(C) * 1e-4).astype(np.float32)

    def run(P):
        xd, gd, md = P.guarded(x), P.guarded(gy), P.guarded(mu)
        s, xtx = ops.stats(xd.view(-1, C))
        mu2, L, W, cs = ops.whiten(xd.view(-1, C), EPS, MOM, 1, None, None)
        R, gsum, sc = ops.bwd_reduce(xd, md, gd, None, 1, want_scales=True)
        dx = ops.bwd_apply(gd, xd, md, P.guarded(At), P.guarded(S), P.guarded(gm), None, scales=sc)
        return [s, xtx, mu2, W, R, gsum, sc, dx]

    s, xtx = run_patterns(run)[0xFF][:2]
    X = x.reshape(-1, C).astype(np.float64)
    nat = np.sqrt(np.outer((X ** 2).sum(0), (X ** 2).sum(0)))
    assert np.abs((xtx.numpy() - X.T @ X) / nat).max() < 1e-6                         # test_fast_reductions_out_of_range_take_the_exact_redo


# ---- the WC site, forward and backward ---------------------------------------------------------------------------------------
def _wc_site(P, inputs, route, Kc):
    """One WC site forward + backward; P = None: the plain run (no harness)."""
    from wc_gan_amd import functional as F
    x, G, B, slot, gy, h, s = inputs
    put = (lambda a: P.guarded(a)) if P is not None else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    C = x.shape[-1]
    Gt, Bt = put(G).requires_grad_(True), put(B).requires_grad_(True)
    sl = put(slot) if Kc > 1 else None
    if route == 'eval':
        mm = put(x.reshape(-1, C).mean(0).astype(np.float32))
        mc = put((np.cov(x.reshape(-1, C).T.astype(np.float64)) + 0.1 * np.eye(C)).astype(np.float32))
    else:
        mm, mc = put(np.zeros(C, np.float32)), put(np.eye(C, dtype=np.float32))
    if route == 'planes':
        ht, st_ = put(h).requires_grad_(True), put(s).requires_grad_(True)
        xin = F.residual_add(ht, st_, True, planes=True, x32=(C != 256), stat_groups=1)
        assert F.split_of(xin) is not None and F.split_of(xin).moments is not None, "the fused producer did not run"
        leaves = (ht, st_, Gt, Bt)
    else:
        xin = put(x).requires_grad_(True)
        leaves = (xin, Gt, Bt)
    y = F.whiten_color(xin, Gt, Bt, sl, mm, mc, route != 'eval', relu=True)
    grads = torch.autograd.grad(y, leaves, put(gy))
    return [y] + list(grads) + [mm, mc]


@pytest.mark.parametrize("route,shape,Kc", [('fp32', (16, 8, 8, 64), 3), ('fp32', (128, 12, 12, 256), 7), ('fp32', (5, 12, 12, 128), 3),
                                            ('planes', (128, 32, 32, 256), 1), ('planes', (128, 16, 16, 256), 10), ('planes', (128, 32, 32, 128), 10),
                                            ('eval', (16, 8, 8, 64), 3), ('eval', (128, 16, 16, 256), 1)])
def test_wc_site_matches_the_unpoisoned_run_bit_for_bit(route, shape, Kc):
    from wc_gan_amd import functional as F
    x, G, B, slot, gy = _site_inputs(shape, Kc, 31, cond="ill")
    N, H, W, C = shape
    rng = np.random.default_rng(32)
    s = (0.5 * rng.standard_normal((N, H // 2, W // 2, C))).astype(np.float32)
    h = (x - np.repeat(np.repeat(s, 2, axis=1), 2, axis=2)).astype(np.float32)
    if route == 'planes':
        assert F.split_route_supported(shape, True) and _ops().resadd_stats_supported(shape, True)
    inputs = (x, G, B, slot, gy, h, s)
    plain = [t.detach().cpu() for t in _wc_site(None, inputs, route, Kc)]
    outs = run_patterns(lambda P: _wc_site(P, inputs, route, Kc))
    diff = [i for i, (a, b) in enumerate(zip(plain, outs[0x7B])) if not same_bits(a, b)]
    assert not diff, f"outputs {diff} differ from the unpoisoned run"


# ---- one G+D step --------------------------------------------------------------------------------------------------------------
def _trainer(conditional, seed=9):
    import test_layers_gpu as tl
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import CIFAR10_COND, GanTrainer
    torch.manual_seed(21)
    if not conditional:
        return tl.reproducible_trainer(batch_size=8, training_ratio=2, seed=seed, flat_buckets=True)
    cfg = CIFAR10_COND
    G = make_generator(**cfg['generator']).cuda()
    D = make_discriminator(**cfg['discriminator']).cuda()
    for m in (G, D):
        for _, p in m.named_parameters():
            if p.dim() == 4 and 3 in (p.shape[0], p.shape[1]):
                p.requires_grad_(False)          # the MIOpen-gradient layers, frozen as reproducible_trainer does
    return GanTrainer(G, D, batch_size=8, training_ratio=2, number_of_classes=10, conditional=True, seed=seed, flat_buckets=True)


def _state_of(tr):
    torch.cuda.synchronize()
    ps = [p.detach().reshape(-1) for p in list(tr.G.parameters()) + list(tr.D.parameters())]
    bs = [b.detach().reshape(-1) for b in list(tr.G.buffers()) + list(tr.D.buffers()) if b.is_floating_point()]
    return torch.cat(ps + bs).cpu()


def _step_run(pattern, conditional, graphs):
    """Models built outside the harness; the step (or the segment-graph capture and replay) inside it."""
    reals = [torch.rand(8, 32, 32, 3, generator=torch.Generator().manual_seed(i)).cuda() * 2 - 1 for i in range(2)]
    labels = [torch.randint(0, 10, (8, 1), generator=torch.Generator().manual_seed(5 + i)).to(torch.int32).cuda() for i in range(2)] \
        if conditional else None
    g = torch.Generator(device='cuda'); g.manual_seed(5)
    noise = {n: (torch.randn(n, 128, device='cuda', generator=g), torch.randint(0, 10, (n, 1), device='cuda', dtype=torch.int32, generator=g))
             for n in (16, 8)}
    tr = _trainer(conditional)
    tr._noise = lambda n: noise[n]
    P = Poison(pattern) if pattern is not None else None
    if P is not None:
        P.__enter__()
    try:
        if graphs:
            replay = tr.capture_segments(reals, labels, warmup=1)
            losses = replay()
        else:
            losses = tr.step(reals, labels)
        st = _state_of(tr)
        if P is not None:
            P.check_guards()
    finally:
        if P is not None:
            P.__exit__(None, None, None)
    return [float(losses[0]), float(losses[1])], st


@pytest.mark.parametrize("conditional,graphs", [(False, False), (False, True), (True, False)])
def test_one_gan_step_is_bit_identical_on_poisoned_memory(conditional, graphs):
    import test_layers_gpu as tl
    with tl.deterministic_convs():
        ref_l, ref_s = _step_run(None, conditional, graphs)
        for p in (0xFF, 0x7B):
            l, s = _step_run(p, conditional, graphs)
            assert l == ref_l, (hex(p), l, ref_l)
            assert same_bits(s, ref_s), f"pattern 0x{p:02X}: {int((s != ref_s).sum())} parameters / statistics differ"


@pytest.mark.parametrize("pattern", [0xFF, 0x7B])
def test_segment_graphs_equal_eager_steps_on_poisoned_memory(pattern):
    """the segment-graph-vs-eager equality of test_layers_gpu, with every allocation of both runs poisoned."""
    import test_layers_gpu as tl
    with Poison(pattern) as P:
        tl.test_segment_graphs_cut_at_the_gradient_all_reduces()
        P.check_guards()
