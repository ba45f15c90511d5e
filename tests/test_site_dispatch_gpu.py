"""Every branch of the WC site's reduction dispatch -- K1, the covariance (wc_stats_f32 / wc_whiten_f32, wc_stats_split_f16x2 /
wc_whiten_split_f16x2, the producer's wc_resadd_stats_split_f32 + wc_*_presummed_f16x2) and K4, R = (x - mu)^T gy (wc_bwd_reduce*_f32,
wc_bwd_reduce_xsplit_f32) -- at the smallest shape that reaches it, against float64.  A call picks one of three kernels and a slab plan
(csrc/wc_fast_xty.hip wc_fast_xty_plan, csrc/wc_split_xty.hip wc_split_xtx_plan, csrc/wc_rows.hip wc_xty_plan / wc_launch_xty, plan_xty
in csrc/wc_abi.hip); the workloads' power-of-two batches reach the full, unpadded plans only.  The rows here are the other classes: a
grid padded to a multiple of 8 slabs (surplus workgroups leave at z >= nslab), a short last slab down to ONE stage (the double-buffered
pipeline with no steady state), several slabs per sample or statistic group, the thresholds between the kernels, and xty_kernel under
its own plan (ragged last slab).

The three plans are restated below in a few lines each, ONLY to label the rows (kernel, nslab, stages per slab, stages of the last slab,
padded grid); the restatement is pinned to the library by recovering nslab from the workspace sizes the ABI reports, and every row states
the class it is there for as literals -- a later change to a plan fails a row instead of emptying it of its purpose.  One row per
kernel also reads the kernel's name from a profiled call.  References and bounds are the suite's own: test_fast_gpu.py (1e-7 on the
split-fp16 kernels, K4's per-entry 1e-7), test_parity_gpu.py (2e-6 on xty_kernel / xty_f64_kernel), test_split_gpu.py (planes),
test_configs_gpu.py (the site, 1e-4).

`PYTHONPATH=. python tests/test_site_dispatch_gpu.py` prints every row's plan and measured errors (profiles/site_dispatch_parity.txt)."""
import functools

import numpy as np
import pytest
import torch

from oracle import wc_oracle as o
from test_conv_dispatch_gpu import _kernel_names
from test_fast_gpu import _mask_ref, _ref_apply
from test_split_gpu import _planes64

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the site's contract (test_configs_gpu.py)
FAST, EXACT = 1e-7, 2e-6      # covariance: the two split-fp16 kernels | xty_kernel and xty_f64_kernel


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- the three plans, restated to label rows with ---------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _whole_stage_slabs(nseg, seg, R, ntypes):
    """wc_fast_xty_plan / wc_split_xtx_plan: slabs of whole R-row stages, the grid (slab groups of 8 x ntypes) within 256 CUs"""
    stages = seg // R
    per_seg = max(1, min(256 // (8 * ntypes) * 8 // nseg, stages))
    sps = _ceil(stages, per_seg)
    nsplit = _ceil(stages, sps)
    return dict(nslab=nseg * nsplit, nsplit=nsplit, stages=sps, last=stages - (nsplit - 1) * sps, padded=(nseg * nsplit) % 8 != 0, ntypes=ntypes)


def _plan_fast(nseg, seg, C, two):
    """xty_f16x3_kernel<C, TWO>: K1 on fp32 (two = False) from 20480 rows, K4 (two = True) from 16384; None = the plan declines"""
    R = 64 if two and C == 256 else 512 // (C // 4) * (4 if two else 8) if C in (32, 64, 128, 256) else 0
    if not R or nseg * seg < (16384 if two else 20480) or seg % R:
        return None
    nb = C // 32
    ntypes = 4 if two and C == 256 else _ceil(nb * nb if two else nb * (nb + 1) // 2, 24)
    return dict(kernel='xty_f16x3_kernel', **_whole_stage_slabs(nseg, seg, R, ntypes))


def _plan_split(nseg, seg, C):
    """xtx_split_kernel<C>: K1 on planes, 64-row flush periods"""
    if C not in (128, 256) or nseg * seg < 20480 or seg % 64:
        return None
    return dict(kernel='xtx_split_kernel', **_whole_stage_slabs(nseg, seg, 64, 3 if C == 256 else 1))


def _plan_exact(nseg, seg, C, sym):
    """wc_xty_plan: ~512 workgroups, rows_per_slab rounded up to BK = 32 (the `stage` of these labels), the last slab ragged;
    wc_launch_xty: xty_f64_kernel up to 20479 rows, xty_kernel above"""
    nb = _ceil(C, 128)
    ntiles = nb * (nb + 1) // 2 if sym else nb * nb
    want = max(1, min(_ceil(512, nseg * ntiles), _ceil(seg, 128 if seg <= 4096 else 256)))
    rps = _ceil(_ceil(seg, want), 32) * 32
    nsplit = _ceil(seg, rps)
    return dict(kernel='xty_f64_kernel' if nseg * seg <= 20479 else 'xty_kernel', nslab=nseg * nsplit, nsplit=nsplit, stages=rps // 32,
                last=_ceil(seg - (nsplit - 1) * rps, 32), padded=False, ntypes=1)


def _plan_xty(nseg, seg, C, sym):
    """plan_xty (csrc/wc_abi.hip): the fast plan, else xty_kernel's own"""
    return _plan_fast(nseg, seg, C, not sym) or _plan_exact(nseg, seg, C, sym)


def _label(p):
    return (p['kernel'], p['nslab'], p['stages'], p['last'], p['padded'])


def _rows(shape):
    return int(np.prod(shape[:-1]))


def _plan_k1(shape, groups):
    return _plan_xty(groups, _rows(shape) // groups, shape[-1], True)


def _plan_planes(shape, groups):
    return _plan_split(groups, _rows(shape) // groups, shape[-1])


def _plan_k4(shape, has_slot):
    N, HW = shape[0], _rows(shape) // shape[0]
    return _plan_xty(N, HW, shape[-1], False) if has_slot else _plan_xty(1, N * HW, shape[-1], False)


# ---- ... and pinned to the library: nslab recovered from the workspace sizes (the carves of csrc/wc_abi.hip) ----------------------
def _al(n):
    return _ceil(n, 256) * 256


def _solve(nbytes, size_of):
    """the nslab whose workspace is nbytes (size_of grows strictly with it)"""
    hit = [n for n in range(1, 4097) if size_of(n) == nbytes]
    assert len(hit) == 1, (nbytes, hit)
    return hit[0]


def _lib():
    from wc_gan_amd import _lib as L
    return L.load()


def _lib_nslab_k1(shape, groups):
    M, C = _rows(shape), shape[-1]
    return _solve(_lib().wc_stats_workspace_bytes(M, C, groups),
                  lambda n: 256 + 2 * _al(4 * C) + _al(16 * groups * C) + _al(4 * n * C) + _al(8 * n * C) + _al(8 * n * C * C))


def _lib_nslab_planes(shape, groups):
    M, C = _rows(shape), shape[-1]
    return _solve(_lib().wc_stats_split_workspace_bytes(M, C, groups),
                  lambda n: 256 + _al(16 * groups * C) + _al(4 * n * C) + _al(8 * n * C) + _al(8 * n * C * C))


def _lib_nslab_k4(shape, has_slot):
    N, C = shape[0], shape[-1]
    return _solve(_lib().wc_bwd_reduce_workspace_bytes(N, _rows(shape) // N, C, 3 if has_slot else 1, int(has_slot)),
                  lambda n: 256 + 2 * _al(4 * C) + _al(4 * n * C) + _al(8 * n * C * C))


def _lib_nslab_producer(shape, groups, ntypes):
    """the producer's workspace: wc_whiten_split_f16x2's layout under the fp32-input kernel's plan + a flag and a maximum per workgroup"""
    N, H, W, C = shape
    grid = lambda n: _ceil(n, 8) * 8 * ntypes
    return _solve(_lib().wc_resadd_stats_workspace_bytes(N, H, W, C, groups),
                  lambda n: 256 + _al(16 * groups * C) + _al(4 * n * C) + _al(8 * n * C) + _al(8 * n * C * C) + _al(8 * groups * C) +
                  _al(4 * grid(n)) + _al(4 * grid(n) * C) + _al(8 * groups * C * C))


def _check_plan(plan, want, lib_nslab):
    """the row's class as literals == the restatement, whose nslab == the library's"""
    assert _label(plan) == want, (_label(plan), want)
    assert lib_nslab == plan['nslab'], (lib_nslab, plan)


REDUCTIONS = ('xty_f16x3_kernel', 'xtx_split_kernel', 'xty_f64_kernel', 'xty_kernel', 'resadd_xtx_kernel')


def _check_kernels(fn, want):
    """the reduction kernels of one profiled call (a fast kernel is followed by its gated exact redo, a no-op here)"""
    names = _kernel_names(fn)
    if not names:
        pytest.skip("this profiler build reports no device kernel names: the kernel was not checked (the plan and parity assertions ran)")
    seen = {k for k in REDUCTIONS for n in names if '::' + k + '<' in n or '::' + k + '(' in n or n.startswith((k + '<', k + '('))}
    assert seen == set(want), (seen, names)


@functools.lru_cache(maxsize=4)
def _activation(shape, cond):
    """one draw per (shape, cond), shared by the rows that differ in statistic groups only; never written to"""
    x = o.synth_activation(np.random.default_rng(21), shape, cond).astype(np.float32)
    x.setflags(write=False)
    return x


def _moment_errs(s, xtx, V, groups):
    """sums / covariance / asymmetry of K1's outputs against float64 moments of V (M, C), the worst over the statistic groups"""
    C = V.shape[-1]
    V = V.reshape(groups, -1, C)
    sn, xn = s.cpu().numpy().reshape(groups, C), xtx.cpu().numpy().reshape(groups, C, C)
    errs = dict(sum=0.0, cov=0.0, asym=0.0)
    for g in range(groups):
        s_ref, xtx_ref, Mg = o.batch_moments(V[g])
        _, cov_ref = o.moments_to_stats(s_ref, xtx_ref, Mg)
        _, cov = o.moments_to_stats(sn[g], xn[g], Mg)
        errs = dict(sum=max(errs['sum'], rel(sn[g], s_ref)), cov=max(errs['cov'], rel(cov, cov_ref)),
                    asym=max(errs['asym'], float(np.abs(xn[g] - xn[g].T).max())))
    return errs


def _same_factor(ops, one_call, s, xtx, M, C, groups, dev_, want_scale):
    """K1 + K2 as one call == K1's moments through wc_factor_f64, bit for bit, moving statistics included (test_fast_gpu.py's
    test_whiten_is_stats_then_factor_bit_for_bit, test_producer_gpu.py's test_whiten_split_is_stats_split_plus_factor)"""
    mm1 = torch.linspace(-0.1, 0.1, C, device="cuda"); mc1 = torch.eye(C, device="cuda") * 1.5
    mm2, mc2 = mm1.clone(), mc1.clone()
    a = ops.factor(s, xtx, M // groups, C, 1e-3, 0.99, 1, True, mm1, mc1, dev_, want_scale=want_scale, groups=groups)
    b = one_call(mm2, mc2)
    torch.cuda.synchronize()
    same = torch.equal(a[0], b[0]) and torch.equal(torch.tril(a[1]), torch.tril(b[1])) and torch.equal(a[2], b[2])
    if want_scale:
        same = same and torch.equal(a[3], b[3])
    return same and torch.equal(mm1, mm2) and torch.equal(mc1, mc2) and bool(torch.isfinite(b[2]).all())


# ---- K1 on fp32: ops.stats / ops.whiten --------------------------------------------------------------------------------------------
# shape, statistic groups, (kernel, nslab, stages per slab, stages of the last slab, padded grid), the kernels to see in a profile | None
K1_ROWS = [
    ((20, 32, 32, 32), 1, ('xty_f16x3_kernel', 40, 1, 1, False), None),         # M = 20480, the threshold exactly; 40 slabs of ONE 512-row stage
    ((81, 16, 16, 64), 1, ('xty_f16x3_kernel', 81, 1, 1, True), None),          # C = 64: one-stage slabs, 7 surplus slab places in the grid
    ((81, 16, 16, 128), 1, ('xty_f16x3_kernel', 162, 1, 1, True), None),        # C = 128: 162 slabs, 6 surplus
    ((85, 16, 16, 256), 1, ('xty_f16x3_kernel', 114, 3, 1, True), ('xty_f16x3_kernel', 'xty_kernel')),   # the last slab ONE stage; padded; ntypes 2
    ((46, 24, 24, 256), 1, ('xty_f16x3_kernel', 104, 4, 2, False), None),       # a short last slab (2 of 4) in a grid that is not padded
    ((82, 16, 16, 64), 2, ('xty_f16x3_kernel', 82, 1, 1, True), None),          # two statistic groups of 41 slabs
    ((46, 24, 24, 256), 2, ('xty_f16x3_kernel', 104, 4, 3, False), None),       # a short last slab (3 of 4) in EACH group
    ((105, 16, 16, 256), 5, ('xty_f16x3_kernel', 105, 4, 4, True), None),       # five groups of 21 slabs: 105, padded
    ((16, 32, 32, 256), 1, ('xty_f64_kernel', 64, 8, 8, False), None),          # 16384 rows (the row test_fast_stats_matches_float64 used to name "fast")
    ((79, 16, 16, 256), 1, ('xty_f64_kernel', 79, 8, 8, False), ('xty_f64_kernel',)),       # 20224 rows: the largest batch of 16x16 below the threshold
    ((81, 16, 16, 32), 1, ('xty_kernel', 81, 8, 8, False), ('xty_kernel',)),    # 20736 % 512 = 256: no whole stages, xty_kernel under its own plan
    ((81, 16, 16, 96), 1, ('xty_kernel', 81, 8, 8, False), None),               # C outside the fast kernel's widths
    ((81, 16, 16, 160), 1, ('xty_kernel', 81, 8, 8, False), None),              # ... two tile columns, the second 32 wide
    ((23, 30, 30, 256), 1, ('xty_kernel', 81, 8, 7, False), None),              # 20700 rows: ragged against every tile (the last chunk holds 28 rows)
]
_ID1 = lambda r: 'x'.join(str(v) for v in r[0]) + f'-g{r[1]}'


def _k1_row(ops, shape, groups, cond):
    """-> errors of ops.stats against float64 per group, and whether ops.whiten equals stats -> factor bit for bit"""
    C, M = shape[-1], _rows(shape)
    x = _activation(shape, cond)
    xd = dev(x).view(M, C)
    s, xtx = ops.stats(xd, groups)
    errs = _moment_errs(s, xtx, x.reshape(M, C).astype(np.float64), groups)
    errs['whiten_same'] = _same_factor(ops, lambda mm, mc: ops.whiten(xd, 1e-3, 0.99, 1, mm, mc, groups), s, xtx, M, C, groups, xd.device, True)
    return errs, xd


@pytest.mark.parametrize("cond", ["ill", "well"])
@pytest.mark.parametrize("row", K1_ROWS, ids=_ID1)
def test_k1_on_fp32_at_each_plan_and_route_edge(row, cond):
    from wc_gan_amd import ops
    shape, groups, want, kernels = row
    plan = _plan_k1(shape, groups)
    _check_plan(plan, want, _lib_nslab_k1(shape, groups))
    errs, xd = _k1_row(ops, shape, groups, cond)
    print("site dispatch K1", _ID1(row), cond, _label(plan), errs)
    assert errs['sum'] < 1e-5 and errs['asym'] == 0.0, errs
    assert errs['cov'] < (FAST if plan['kernel'] == 'xty_f16x3_kernel' else EXACT), errs
    assert errs['whiten_same'], errs
    if kernels is not None and cond == "ill":
        _check_kernels(lambda: ops.stats(xd, groups), kernels)


# ---- K1 on planes: ops.split, then ops.stats_split / ops.whiten_split; the producer where it takes the shape ---------------------
# shape, groups, (kernel, ...), ops.resadd_stats_supported(shape, up=True, groups), the kernels to see in a profile | None
PLANES_ROWS = [
    ((20, 32, 32, 128), 1, ('xtx_split_kernel', 160, 2, 2, False), True, None),       # M = 20480, the threshold exactly
    ((37, 24, 24, 128), 1, ('xtx_split_kernel', 167, 2, 1, True), False, ('xtx_split_kernel',)),     # C = 128: the last slab ONE period of 2; padded
    ((39, 24, 24, 128), 1, ('xtx_split_kernel', 176, 2, 1, False), False, None),      # ... a short last slab in a grid that is not padded
    ((89, 16, 16, 256), 1, ('xtx_split_kernel', 72, 5, 1, False), True, None),        # C = 256: 72 slabs of 5, the last of ONE
    ((81, 16, 16, 256), 1, ('xtx_split_kernel', 65, 5, 4, True), True, None),         # 65 slabs, the last of 4; padded
    ((36, 24, 24, 256), 2, ('xtx_split_kernel', 66, 5, 2, True), True, None),         # two groups of 33 slabs, the last of each 2 periods
    ((85, 16, 16, 128), 5, ('xtx_split_kernel', 170, 2, 2, True), True, None),        # five groups of 34 slabs
]


def _planes_row(ops, shape, groups, cond, producer):
    C, M = shape[-1], _rows(shape)
    x = _activation(shape, cond)
    xs = ops.split(dev(x))
    s, xtx = ops.stats_split(xs, groups)
    errs = _moment_errs(s, xtx, _planes64(xs), groups)
    errs['flag'] = int(xs.flag[0])
    errs['whiten_same'] = _same_factor(ops, lambda mm, mc: ops.whiten_split(xs, 1e-3, 0.99, 1, mm, mc, groups), s, xtx, M, C, groups,
                                       xs.planes.device, False)
    perrs = None
    if producer:        # h + upsample2x(s) = x up to fp32 rounding: the reference is whatever the planes then hold
        N, H, W, _ = shape
        sd = dev((0.5 * np.random.default_rng(7).standard_normal((N, H // 2, W // 2, C))).astype(np.float32))
        hd = dev(x) - sd.view(N, H // 2, 1, W // 2, 1, C).expand(N, H // 2, 2, W // 2, 2, C).reshape(shape)
        st = ops.resadd_stats_split(hd, sd, True, groups)
        sm, xm = ops.stats_presummed(st, groups)
        perrs = _moment_errs(sm, xm, _planes64(st), groups)
        perrs['flag'] = int(st.flag[0])
        perrs['whiten_same'] = _same_factor(ops, lambda mm, mc: ops.whiten_presummed(st, 1e-3, 0.99, 1, mm, mc, groups), sm, xm, M, C, groups,
                                            st.planes.device, False)
    return errs, perrs, xs


@pytest.mark.parametrize("cond", ["ill", "well"])
@pytest.mark.parametrize("row", PLANES_ROWS, ids=_ID1)
def test_k1_on_planes_at_each_plan_edge(row, cond):
    from wc_gan_amd import ops
    shape, groups, want, producer, kernels = row
    plan = _plan_planes(shape, groups)
    _check_plan(plan, want, _lib_nslab_planes(shape, groups))
    assert ops.stats_split_supported(_rows(shape), shape[-1], groups)
    assert ops.resadd_stats_supported(shape, True, groups) == producer
    if producer:        # the producer accumulates under the fp32-input kernel's plan
        pplan = _plan_fast(groups, _rows(shape) // groups, shape[-1], False)
        assert _lib_nslab_producer(shape, groups, pplan['ntypes']) == pplan['nslab'] == _lib_nslab_k1(shape, groups)
    errs, perrs, xs = _planes_row(ops, shape, groups, cond, producer)
    print("site dispatch K1 planes", _ID1(row), cond, _label(plan), errs, "producer", perrs)
    for e in (errs, perrs) if producer else (errs,):
        assert e['flag'] == 0, e
        assert e['sum'] < 1e-5 and e['asym'] == 0.0 and e['cov'] < FAST, e
        assert e['whiten_same'], e
    if kernels is not None and cond == "ill":
        _check_kernels(lambda: ops.stats_split(xs, groups), kernels)


# ---- K4: ops.bwd_reduce, no slot (Kc = 1) and with a slot table ------------------------------------------------------------------
# shape, Kc, (kernel, ...), ops.bwd_xsplit_supported(shape, Kc > 1), the kernels to see in a profile | None
K4_ROWS = [
    ((64, 16, 16, 32), 1, ('xty_f16x3_kernel', 64, 1, 1, False), False, ('xty_f16x3_kernel', 'xty_f64_kernel')),   # 16384 rows, K4's threshold exactly
    ((64, 16, 16, 32), 3, ('xty_f16x3_kernel', 64, 1, 1, False), False, None),           # one one-stage slab per sample
    ((65, 16, 16, 64), 1, ('xty_f16x3_kernel', 130, 1, 1, True), False, None),           # C = 64: 130 slabs, padded
    ((65, 16, 16, 64), 3, ('xty_f16x3_kernel', 130, 1, 1, True), False, None),           # 2 slabs per sample
    ((29, 24, 24, 128), 1, ('xty_f16x3_kernel', 131, 2, 1, True), False, None),          # the last slab ONE stage of 2; padded
    ((29, 24, 24, 128), 3, ('xty_f16x3_kernel', 145, 2, 1, True), False, None),          # 5 slabs per sample as 2, 2, 2, 2, 1 stages
    ((69, 16, 16, 256), 1, ('xty_f16x3_kernel', 56, 5, 1, False), True, None),           # quadrant form: 56 slabs of 5, the last of ONE
    ((69, 16, 16, 256), 3, ('xty_f16x3_kernel', 69, 4, 4, True), True, None),            # 69 one-slab samples, padded
    ((32, 24, 24, 256), 1, ('xty_f16x3_kernel', 58, 5, 3, True), True, None),            # 58 slabs, the last of 3; padded
    ((32, 24, 24, 256), 3, ('xty_f16x3_kernel', 64, 5, 4, False), True, None),           # 5 + 4 stages per sample
    ((20, 32, 32, 256), 3, ('xty_f16x3_kernel', 60, 6, 4, True), True, None),            # 6, 6, 4 stages per sample; 60 slabs, padded
    ((63, 16, 16, 256), 1, ('xty_f64_kernel', 63, 8, 8, False), False, ('xty_f64_kernel',)),     # 16128 rows: below K4's threshold
    ((63, 16, 16, 256), 3, ('xty_f64_kernel', 126, 4, 4, False), False, None),
    ((160, 12, 12, 256), 7, ('xty_kernel', 160, 5, 5, False), False, ('xty_kernel',)),   # HW = 144: no whole stages per sample, xty_kernel per sample (the last chunk holds 16 rows)
]
_ID4 = lambda r: 'x'.join(str(v) for v in r[0]) + f'-Kc{r[1]}'


def _k4_errs(R, gsum, f, g, slot, Kc):
    """test_fast_bwd_reduce_matches_float64's measure: per entry |dR| / sqrt(sum f^2 sum g^2), and gsum, the worst over the slots"""
    N, C = f.shape[0], f.shape[-1]
    eR = eg = 0.0
    for k in range(Kc):
        sel = slot == k if Kc > 1 else np.ones(N, bool)
        fk, gk = f[sel].reshape(-1, C), g[sel].reshape(-1, C)
        scale = np.sqrt(np.outer((fk ** 2).sum(0), (gk ** 2).sum(0))) + 1e-300
        eR = max(eR, float(np.abs((R[k].cpu().numpy() - fk.T @ gk) / scale).max()))
        eg = max(eg, rel(gsum[k].cpu().numpy(), gk.sum(0)))
    return eR, eg


def _k4_row(ops, shape, Kc, xsplit):
    """-> errors of every form of K4 this row takes: plain; at C = 256 behind a ReLU (relu_y, the bit mask, the bits without a masked
    copy where that route exists); on the planes of the same x where K4 reads planes"""
    rng = np.random.default_rng(22)
    N, C = shape[0], shape[-1]
    x = (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, C)) + 0.3).astype(np.float32)
    gy = (rng.standard_normal(shape) * 1e-3 * np.exp(rng.uniform(-3, 3, C))).astype(np.float32)
    mu = x.reshape(-1, C).mean(0).astype(np.float32)
    slot = rng.integers(0, Kc, N).astype(np.int32)
    st = dev(slot, torch.int32) if Kc > 1 else None
    xd, mud, gyd = dev(x), dev(mu), dev(gy)
    f = x.astype(np.float64).reshape(N, -1, C) - mu.astype(np.float64)
    g = gy.astype(np.float64).reshape(N, -1, C)
    R, gsum = ops.bwd_reduce(xd, mud, gyd, st, Kc)
    errs = {}
    errs['R'], errs['gsum'] = _k4_errs(R, gsum, f, g, slot, Kc)
    if C == 256:
        y = rng.standard_normal(shape).astype(np.float32)
        y[0, 0, 0, :8] = 0.0; y[0, 0, 1, :8] = -0.0; y[1, 2, 3, 4] = np.nan          # the edges of `y > 0`
        g_ref = np.where(~(y <= 0), gy, np.float32(0))
        mask = dev(_mask_ref(y.reshape(-1, C)).view(np.int32), torch.int32)
        R1, g1, gm1, sc1 = ops.bwd_reduce(xd, mud, gyd, st, Kc, want_scales=True, relu_y=dev(y))
        errs['R_relu'], errs['gsum_relu'] = _k4_errs(R1, g1, f, g_ref.astype(np.float64).reshape(N, -1, C), slot, Kc)
        errs['masked_gy_exact'] = bool(np.array_equal(gm1.cpu().numpy(), g_ref))
        R2, g2, gm2, sc2 = ops.bwd_reduce(xd, mud, gyd, st, Kc, want_scales=True, relu_mask=mask)
        errs['bits_same'] = torch.equal(R1, R2) and torch.equal(g1, g2) and torch.equal(gm1, gm2) and torch.equal(sc1, sc2)
        errs['bits_only'] = ops.bwd_bits_supported(shape, Kc > 1)
        if errs['bits_only']:
            R3, g3, sc3 = ops.bwd_reduce(xd, mud, gyd, st, Kc, want_scales=True, relu_mask=mask, write_masked=False)
            errs['bits_only_same'] = torch.equal(R1, R3) and torch.equal(g1, g3) and torch.equal(sc1, sc3)
    if xsplit:
        xs = ops.split(xd)
        Rx, gx, _ = ops.bwd_reduce_xsplit(xs, mud, gyd, st, Kc)
        errs['flag'] = int(xs.flag[0])
        errs['R_xsplit'], errs['gsum_xsplit'] = _k4_errs(Rx, gx, _planes64(xs).reshape(N, -1, C) - mu.astype(np.float64), g, slot, Kc)
    return errs, (xd, mud, gyd, st)


@pytest.mark.parametrize("row", K4_ROWS, ids=_ID4)
def test_k4_at_each_plan_and_route_edge(row):
    from wc_gan_amd import ops
    shape, Kc, want, xsplit, kernels = row
    plan = _plan_k4(shape, Kc > 1)
    _check_plan(plan, want, _lib_nslab_k4(shape, Kc > 1))
    assert ops.bwd_xsplit_supported(shape, Kc > 1) == xsplit
    errs, (xd, mud, gyd, st) = _k4_row(ops, shape, Kc, xsplit)
    print("site dispatch K4", _ID4(row), _label(plan), errs)
    for k in ('', '_relu', '_xsplit'):
        if 'R' + k in errs:
            assert errs['R' + k] < 1e-7 and errs['gsum' + k] < 1e-5, errs
    if shape[-1] == 256:
        assert errs['masked_gy_exact'] and errs['bits_same'] and errs.get('bits_only_same', True), errs
    assert errs.get('flag', 0) == 0, errs
    if kernels is not None:
        _check_kernels(lambda: ops.bwd_reduce(xd, mud, gyd, st, Kc), kernels)


# ---- the site: functional.whiten_color forward, backward and moving statistics against the oracle ---------------------------------
# shape, Kc, planes route (the input arrives from functional.residual_add(planes=True, stat_groups=1)), does the fused producer take it,
# K1's (kernel, nslab, stages per slab, stages of the last slab, padded grid), K4's
SITE_ROWS = [
    # K1: the last slab ONE stage, padded; K4: the last slab 4 of 6, padded
    ((85, 16, 16, 256), 1, False, None, ('xty_f16x3_kernel', 114, 3, 1, True), ('xty_f16x3_kernel', 57, 6, 4, True)),
    # K1: a short last slab; K4: the last slab ONE stage of 7, padded
    ((46, 24, 24, 256), 1, False, None, ('xty_f16x3_kernel', 104, 4, 2, False), ('xty_f16x3_kernel', 60, 7, 1, True)),
    # K4 with slots: 2, 2, 2, 2, 1 stages per sample; K1 below its threshold (16704 rows, ragged last slab)
    ((29, 24, 24, 128), 3, False, None, ('xty_f64_kernel', 66, 8, 2, False), ('xty_f16x3_kernel', 145, 2, 1, True)),
    # K4 with slots: 6, 6, 4 stages per sample; K1 at its threshold, short last slab, padded
    ((20, 32, 32, 256), 3, False, None, ('xty_f16x3_kernel', 107, 3, 2, True), ('xty_f16x3_kernel', 60, 6, 4, True)),
    # K1 on xty_kernel (no whole 512-row stages), K4 on the fast kernel (256-row stages), padded
    ((81, 16, 16, 32), 1, False, None, ('xty_kernel', 81, 8, 8, False), ('xty_f16x3_kernel', 81, 1, 1, True)),
    # K4 on xty_kernel per sample (HW = 144), K1 on the fast kernel
    ((160, 12, 12, 256), 7, False, None, ('xty_f16x3_kernel', 120, 3, 3, False), ('xty_kernel', 160, 5, 5, False)),
    # planes: the producer accumulates K1 under the fp32-input plan (short last slab, padded); K4 and K6 read the planes
    ((89, 16, 16, 256), 1, True, True, ('xty_f16x3_kernel', 119, 3, 2, True), ('xty_f16x3_kernel', 60, 6, 2, True)),
    # planes: no whole 128-row stages for the producer -> xtx_split_kernel, the last slab ONE period, padded; K4 and K6 read the fp32 copy
    ((37, 24, 24, 128), 1, True, False, ('xtx_split_kernel', 167, 2, 1, True), ('xty_f16x3_kernel', 167, 2, 1, True)),
]
_IDS = lambda r: 'x'.join(str(v) for v in r[0]) + f'-Kc{r[1]}' + ('-planes' if r[2] else '')


def _site_row(shape, Kc, planes, fused, cond):
    """test_configs_gpu.py's body (fp32 input) / test_producer_gpu.py's _fused_site (planes): -> errors of y, dx, dGamma, dbeta, moving statistics"""
    from wc_gan_amd.functional import backward_reads_planes, residual_add, split_of, whiten_color
    rng = np.random.default_rng(11)
    N, H, W, C = shape
    x = o.synth_activation(rng, shape, cond).astype(np.float32)
    G, B = o.synth_coloring(rng, C, Kc)
    G = G.astype(np.float32); B = B.astype(np.float32)
    slot = rng.integers(0, Kc, N).astype(np.int32)
    gy = rng.standard_normal(shape).astype(np.float32)
    Gt = dev(G).requires_grad_(True); Bt = dev(B).requires_grad_(True)
    mm = torch.zeros(C, 1, device="cuda"); mc = torch.eye(C, device="cuda")
    st = dev(slot, torch.int32) if Kc > 1 else None
    if planes:
        s = (0.5 * rng.standard_normal((N, H // 2, W // 2, C))).astype(np.float32)
        up = np.repeat(np.repeat(s, 2, axis=1), 2, axis=2)
        h = (x - up).astype(np.float32)
        x = (h + up).astype(np.float32)                   # the fp32 sum the kernel forms (IEEE: the same bits)
        xt, st_ = dev(h).requires_grad_(True), dev(s).requires_grad_(True)
        xin = residual_add(xt, st_, True, planes=True, x32=not backward_reads_planes(shape, Kc > 1), stat_groups=1)
        assert split_of(xin) is not None, "the residual add did not hand over planes"
        assert (split_of(xin).moments is not None) == fused
    else:
        xin = xt = dev(x).requires_grad_(True)
    y_ref, cache = o.wc_forward(x, G, B, slot, moving_mean=np.zeros(C), moving_cov=np.eye(C))
    dx_ref, dG_ref, dB_ref = o.wc_backward(gy, cache)
    y = whiten_color(xin, Gt, Bt, st, mm, mc, True)
    y.backward(dev(gy))
    errs = dict(y=rel(y.detach().cpu().numpy(), y_ref.reshape(shape)), dx=rel(xt.grad.cpu().numpy(), dx_ref.reshape(shape)),
                dG=rel(Gt.grad.cpu().numpy(), dG_ref), dB=rel(Bt.grad.cpu().numpy(), dB_ref),
                mm=rel(mm.cpu().numpy().reshape(-1), cache['moving_mean']), mc=rel(mc.cpu().numpy(), cache['moving_cov']))
    if planes:
        errs['ds'] = rel(st_.grad.cpu().numpy(), dx_ref.reshape(N, H // 2, 2, W // 2, 2, C).sum((2, 4)))
    return errs


@pytest.mark.parametrize("row", SITE_ROWS, ids=_IDS)
def test_site_forward_backward_at_the_plan_edges(row):
    """Well-conditioned input: these rows are about indexing, not about cond(Sigma).  (The same rows at cond ~ 1e6 are measured, not
    asserted, by this file's __main__: profiles/site_dispatch_parity.txt.)"""
    shape, Kc, planes, fused, k1, k4 = row
    groups1 = (shape, 1)
    if fused:
        pplan = _plan_fast(1, _rows(shape), shape[-1], False)
        _check_plan(pplan, k1, _lib_nslab_producer(shape, 1, pplan['ntypes']))
    elif planes:
        _check_plan(_plan_planes(*groups1), k1, _lib_nslab_planes(*groups1))
    else:
        _check_plan(_plan_k1(*groups1), k1, _lib_nslab_k1(*groups1))
    _check_plan(_plan_k4(shape, Kc > 1), k4, _lib_nslab_k4(shape, Kc > 1))
    errs = _site_row(shape, Kc, planes, fused, "well")
    print("site dispatch site", _IDS(row), errs)
    assert all(v < TOL for v in errs.values()), errs


# ---- K3's and K6's own route edges, each with Kc = 3 slots ------------------------------------------------------------------------
K3_ROWS = [
    (16, 8, 8, 256),        # 1024 rows: the fewest the fast kernel takes
    (15, 8, 8, 256),        # 960 rows: rows_gemm_kernel
    (17, 8, 8, 64),         # 1088 rows, no whole 256-row tiles: rows_gemm_kernel
]


def _k3_row(ops, shape, Kc=3):
    """test_fast_apply_matches_float64's body"""
    rng = np.random.default_rng(11)
    N, C = shape[0], shape[-1]
    chan_scale = np.exp(rng.uniform(-6, 6, C))
    x = (rng.standard_normal(shape) * chan_scale + 3 * chan_scale).astype(np.float32)
    mu = (3 * chan_scale).astype(np.float32)
    A = (rng.standard_normal((Kc, C, C)) / np.sqrt(C) / chan_scale[None, :, None]).astype(np.float32)
    b = rng.standard_normal((Kc, C)).astype(np.float32)
    slot = rng.integers(0, Kc, N).astype(np.int32)
    st = dev(slot, torch.int32)
    ref = _ref_apply(x, mu, A, b, slot)
    return {('fast' if fast else 'exact'): rel(ops.apply(dev(x), dev(mu), dev(A), dev(b), st, fast=fast).cpu().numpy().reshape(ref.shape), ref)
            for fast in (True, False)}


@pytest.mark.parametrize("shape", K3_ROWS, ids=lambda s: 'x'.join(map(str, s)))
def test_k3_at_its_route_edges(shape):
    from wc_gan_amd import ops
    errs = _k3_row(ops, shape)
    print("site dispatch K3", shape, errs)
    assert errs['fast'] < 3e-6 and errs['exact'] < 3e-6, errs


K6_ROWS = [
    (64, 8, 8, 256),        # 4096 rows: the fewest the one-pass kernel takes (with K4's scales at hand)
    (63, 8, 8, 256),        # 4032 rows: two passes
]


def _k6_row(ops, shape, Kc=3):
    """test_fast_bwd_apply_matches_float64's body, training mode: the two-pass fast route, the exact route, and the route with K4's scales"""
    rng = np.random.default_rng(13)
    N, C = shape[0], shape[-1]
    x = rng.standard_normal(shape).astype(np.float32) + 0.5
    gy = (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    mu = np.full(C, 0.5, np.float32)
    A = (rng.standard_normal((Kc, C, C)) / np.sqrt(C)).astype(np.float32)
    At = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    S = rng.standard_normal((C, C)).astype(np.float32) * 1e-4; S = (S + S.T) / 2
    gm = (rng.standard_normal(C) * 1e-4).astype(np.float32)
    slot = rng.integers(0, Kc, N).astype(np.int32)
    st = dev(slot, torch.int32)
    args = (dev(gy), dev(x), dev(mu), dev(At), dev(S), dev(gm), st)
    ref = np.einsum('npc,nco->npo', gy.astype(np.float64).reshape(N, -1, C), At.astype(np.float64)[slot]) \
        + (x.astype(np.float64).reshape(N, -1, C) - mu) @ S.astype(np.float64) - gm.astype(np.float64)
    scales = ops.bwd_reduce(dev(x), dev(mu), dev(gy), st, Kc, want_scales=True)[-1]
    got = dict(fast=ops.bwd_apply(*args, fast=True), exact=ops.bwd_apply(*args, fast=False), shared=ops.bwd_apply(*args, fast=True, scales=scales))
    return {k: rel(v.cpu().numpy().reshape(ref.shape), ref) for k, v in got.items()}


@pytest.mark.parametrize("shape", K6_ROWS, ids=lambda s: 'x'.join(map(str, s)))
def test_k6_at_its_one_pass_threshold(shape):
    from wc_gan_amd import ops
    errs = _k6_row(ops, shape)
    print("site dispatch K6", shape, errs)
    assert all(v < 3e-6 for v in errs.values()), errs


if __name__ == '__main__':
    from wc_gan_amd import ops as _ops

    def _fmt(e):
        return '  '.join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in e.items())

    def _plan_cols(p):
        return f"{p['kernel']:<18}{p['nslab']:>6}{p['stages']:>8}{p['last']:>6}{str(p['padded']):>8}"

    head = f"{'row':<30}{'kernel':<18}{'nslab':>6}{'stages':>8}{'last':>6}{'padded':>8}  errors against float64"
    print("K1 on fp32 (ops.stats; whiten_same: ops.whiten == stats -> factor bit for bit)\n" + head)
    for shape, groups, _want, _k in K1_ROWS:
        for cond in ("ill", "well"):
            print(f"{_ID1((shape, groups)) + ' ' + cond:<30}{_plan_cols(_plan_k1(shape, groups))}  {_fmt(_k1_row(_ops, shape, groups, cond)[0])}")
    print("\nK1 on planes (ops.stats_split; `producer`: ops.resadd_stats_split -> ops.stats_presummed, under the fp32-input plan)\n" + head)
    for shape, groups, _want, producer, _k in PLANES_ROWS:
        for cond in ("ill", "well"):
            errs, perrs, _xs = _planes_row(_ops, shape, groups, cond, producer)
            print(f"{_ID1((shape, groups)) + ' ' + cond:<30}{_plan_cols(_plan_planes(shape, groups))}  {_fmt(errs)}")
            if producer:
                print(f"{'  producer':<30}{_plan_cols(_plan_fast(groups, _rows(shape) // groups, shape[-1], False))}  {_fmt(perrs)}")
    print("\nK4 (ops.bwd_reduce; _relu: behind a ReLU; _xsplit: ops.bwd_reduce_xsplit on the planes of the same x)\n" + head)
    for shape, Kc, _want, xsplit, _k in K4_ROWS:
        print(f"{_ID4((shape, Kc)):<30}{_plan_cols(_plan_k4(shape, Kc > 1))}  {_fmt(_k4_row(_ops, shape, Kc, xsplit)[0])}")
    print("\nthe site (functional.whiten_color: forward, backward, moving statistics against the oracle; `ill` is measured, not asserted)")
    for row in SITE_ROWS:
        shape, Kc, planes, fused, k1, k4 = row
        print(f"{_IDS(row):<30}K1 {k1}  K4 {k4}")
        for cond in ("well", "ill"):
            print(f"{'  ' + cond:<30}{_fmt(_site_row(shape, Kc, planes, fused, cond))}")
    print("\nK3 (ops.apply, Kc = 3) and K6 (ops.bwd_apply, Kc = 3) at their route edges")
    for shape in K3_ROWS:
        print(f"{'K3 ' + 'x'.join(map(str, shape)):<30}{_fmt(_k3_row(_ops, shape))}")
    for shape in K6_ROWS:
        print(f"{'K6 ' + 'x'.join(map(str, shape)):<30}{_fmt(_k6_row(_ops, shape))}")
