"""GPU tests of the fused batch-norm site (csrc/wc_std.hip): stage by stage through the C ABI and end to end through
functional.standardize_color against the float64 reference tests/std_reference.py, on poisoned, guard-banded device memory
(tests/_poison.py); bit-level determinism (runs, graph replay, groups); the layer against torch's route; the launches of a site; the
batch-norm generator on both routes and one captured G+D step of it.

Bounds: y, dx, dgamma, dbeta at 1e-4 relative (max-abs error over max-abs reference); mu, w and the moving statistics at
1e-6.  The reference's own arithmetic in fp32 is within 4e-7 of float64 on these inputs.  With the ReLU on, the reference's backward takes
its mask from the GPU's own forward output."""
import numpy as np
import pytest
import torch

import std_reference as R
from oracle import wc_oracle as o

from _poison import PATTERNS, Poison, run_patterns, same_bits

pytestmark = pytest.mark.gpu

TOL, TOL_STAT = 1e-4, 1e-6
K_CLASSES = 5


def _inputs(seed, shape, K=K_CLASSES, conditioning="ill", conditional=True):
    """oracle.synth_activation plus a per-channel offset of 3 sigma; coloring vectors 1 + 0.5 N(0,1), 0.3 N(0,1)."""
    rng = np.random.default_rng(seed)
    C = shape[-1]
    x = o.synth_activation(rng, shape, conditioning)
    x = x + 3.0 * x.reshape(-1, C).std(0) * rng.standard_normal(C)
    x = x.astype(np.float32)
    Kc = K if conditional else 1
    gamma = (1.0 + 0.5 * rng.standard_normal((Kc, C))).astype(np.float32)
    beta = (0.3 * rng.standard_normal((Kc, C))).astype(np.float32)
    slot = rng.integers(0, Kc, shape[0]).astype(np.int32) if conditional else None
    gy = rng.standard_normal(shape).astype(np.float32)
    mm = (0.1 * rng.standard_normal(C)).astype(np.float32)
    mv = (1.0 + 0.5 * rng.random(C)).astype(np.float32)
    return dict(x=x, gamma=gamma, beta=beta, slot=slot, gy=gy, mm=mm, mv=mv)


def _site(P, d, relu=True, training=True, ddof=0):
    """forward + backward through functional.standardize_color on guarded inputs -> dict of results"""
    from wc_gan_amd.functional import standardize_color
    x = P.guarded(d['x']).requires_grad_(True)
    gamma = P.guarded(d['gamma']).requires_grad_(True)
    beta = P.guarded(d['beta']).requires_grad_(True)
    slot = None if d['slot'] is None else P.guarded(d['slot'])
    mm, mv = P.guarded(d['mm']), P.guarded(d['mv'])
    y = standardize_color(x, gamma, beta, slot, mm, mv, training, 1e-3, 0.99, ddof, relu=relu)
    y.backward(P.guarded(d['gy']))
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, mm=mm, mv=mv)


def _check_site(d, out, relu=True, training=True, ddof=0, what=""):
    y_ref, cache = R.forward(d['x'], d['gamma'], d['beta'], d['slot'], d['mm'], d['mv'], training, 1e-3, 0.99, ddof, relu)
    y = out['y'].numpy()
    dx_ref, dg_ref, db_ref = R.backward(d['gy'], cache, mask=(y > 0) if relu else None)
    errs = dict(y=R.rel(y, y_ref), dx=R.rel(out['dx'].numpy(), dx_ref), dgamma=R.rel(out['dgamma'].numpy(), dg_ref),
                dbeta=R.rel(out['dbeta'].numpy(), db_ref))
    stat = {}
    if training:
        stat = dict(mm=R.rel(out['mm'].numpy(), cache['moving_mean']), mv=R.rel(out['mv'].numpy(), cache['moving_variance']))
    print(f"std site {what} {d['x'].shape}: " + " ".join(f"{k}={v:.2e}" for k, v in {**errs, **stat}.items()))
    assert all(v < TOL for v in errs.values()), errs
    assert all(v < TOL_STAT for v in stat.values()), stat


# ---------------------------------------------------------------------------------------------------------------------------------
# stage by stage through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conditioning", ["ill", "well"])
@pytest.mark.parametrize("shape", [(32, 16, 16, 64), (16, 32, 32, 128)])
def test_stages_against_the_reference(shape, conditioning):
    from wc_gan_amd import ops
    d = _inputs(3, shape, conditioning=conditioning)
    N, C = shape[0], shape[-1]
    M = int(np.prod(shape[:-1]))

    def run(P):
        x, gy = P.guarded(d['x']), P.guarded(d['gy'])
        gamma, beta, slot = P.guarded(d['gamma']), P.guarded(d['beta']), P.guarded(d['slot'])
        mm, mv = P.guarded(d['mm']), P.guarded(d['mv'])
        s, sq = ops.std_stats(x.view(M, C))
        mu, w, a, b = ops.std_factor(s, sq, M, C, 1e-3, 0.99, 1, True, mm, mv, gamma, beta, x.device)
        y = ops.std_apply(x, a, b, slot, relu=True)
        gsum, gxsum = ops.std_bwd_reduce(x, gy, a, b, slot, K_CLASSES, relu=True)
        dgamma, dbeta, q, r = ops.std_bwd_factor(gsum, gxsum, mu.view(-1), w.view(-1), gamma, M)
        dx = ops.std_bwd_apply(x, gy, a, b, q, r, slot, relu=True)
        return dict(s=s, sq=sq, mu=mu, w=w, a=a, b=b, y=y, gsum=gsum, gxsum=gxsum, dgamma=dgamma, dbeta=dbeta, q=q, r=r, dx=dx, mm=mm, mv=mv)

    out = run_patterns(run)[PATTERNS[0]]
    x64 = d['x'].astype(np.float64).reshape(M, C)
    y_ref, cache = R.forward(d['x'], d['gamma'], d['beta'], d['slot'], d['mm'], d['mv'], True, 1e-3, 0.99, 1, True)
    y = out['y'].numpy()
    mask = y > 0
    dx_ref, dg_ref, db_ref = R.backward(d['gy'], cache, mask=mask)
    mu, w = cache['mu'][0], cache['w'][0]
    gp = np.where(mask, d['gy'].astype(np.float64), 0.0).reshape(N, -1, C)
    gs_ref = np.zeros((K_CLASSES, C)); gx_ref = np.zeros((K_CLASSES, C))
    np.add.at(gs_ref, d['slot'], gp.sum(1)); np.add.at(gx_ref, d['slot'], (gp * x64.reshape(N, -1, C)).sum(1))
    # float64 accumulation of fp32 values: at most M * 2^-53 relative (1.8e-12 at M = 16384); 1e-10 leaves the summation order free
    sums = dict(s=R.rel(out['s'].numpy()[0], x64.sum(0)), sq=R.rel(out['sq'].numpy()[0], (x64 * x64).sum(0)),
                gsum=R.rel(out['gsum'].numpy(), gs_ref), gxsum=R.rel(out['gxsum'].numpy(), gx_ref))
    stat = dict(mu=R.rel(out['mu'].numpy()[0], mu), w=R.rel(out['w'].numpy()[0], w), mm=R.rel(out['mm'].numpy(), cache['moving_mean']),
                mv=R.rel(out['mv'].numpy(), cache['moving_variance']))
    a_ref = d['gamma'].astype(np.float64) * w
    errs = dict(a=R.rel(out['a'].numpy(), a_ref), b=R.rel(out['b'].numpy(), d['beta'] - a_ref * mu), y=R.rel(y, y_ref),
                dgamma=R.rel(out['dgamma'].numpy(), dg_ref), dbeta=R.rel(out['dbeta'].numpy(), db_ref), dx=R.rel(out['dx'].numpy(), dx_ref))
    print(f"std stages {shape} {conditioning}: " + " ".join(f"{k}={v:.2e}" for k, v in {**sums, **stat, **errs}.items()))
    assert all(v < 1e-10 for v in sums.values()), sums
    assert all(v < TOL_STAT for v in stat.values()), stat
    assert all(v < TOL for v in errs.values()), errs


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end, every site shape of the four configurations
# ---------------------------------------------------------------------------------------------------------------------------------
def _site_shapes():
    from wc_gan_amd.train import CONFIGS, wc_sites
    seen, out = set(), []
    for name, cfg in CONFIGS.items():
        K = cfg['generator']['number_of_classes'] if cfg['conditional'] else 0
        for batch in (64, 128):             # the critic-phase batch and the generator update's (batch_size x generator_batch_multiple)
            for _, N, H, W, C in wc_sites(cfg, batch):
                key = (N, H, W, C, K)
                if key not in seen:
                    seen.add(key)
                    out.append(pytest.param((N, H, W, C), K, id=f"{name}-{N}x{H}x{W}x{C}"))
    return out


@pytest.mark.parametrize("shape,K", _site_shapes())
def test_every_site_shape_of_the_four_configurations(shape, K):
    d = _inputs(sum(shape) + K, shape, K=max(K, 1), conditional=K > 0)
    outs = run_patterns(lambda P: _site(P, d))
    _check_site(d, outs[PATTERNS[0]], what="config")


@pytest.mark.parametrize("shape", [(1, 5, 7, 32), (3, 5, 7, 64), (1, 4, 4, 128), (2, 3, 3, 256), (2, 6, 6, 1024), (1, 9, 4, 1024), (5, 4, 4, 96)])
@pytest.mark.parametrize("relu", [False, True])
def test_widths_and_single_samples(shape, relu):
    d = _inputs(7, shape, conditional=shape[0] > 1)
    outs = run_patterns(lambda P: _site(P, d, relu=relu, ddof=0))
    _check_site(d, outs[PATTERNS[0]], relu=relu, what="width")


@pytest.mark.parametrize("ddof", [0, 1])
def test_ddof_scales_the_moving_variance_only(ddof):
    d = _inputs(9, (8, 6, 6, 64))
    outs = run_patterns(lambda P: _site(P, d, ddof=ddof))
    _check_site(d, outs[PATTERNS[0]], ddof=ddof, what=f"ddof{ddof}")


def test_evaluation_mode_against_the_reference():
    d = _inputs(13, (16, 8, 8, 128))
    outs = run_patterns(lambda P: _site(P, d, training=False))
    out = outs[PATTERNS[0]]
    _check_site(d, out, training=False, what="eval")
    assert np.array_equal(out['mm'].numpy(), d['mm']) and np.array_equal(out['mv'].numpy(), d['mv'])       # untouched


# ---------------------------------------------------------------------------------------------------------------------------------
# the ReLU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_relu_backward_equals_the_plain_backward_on_the_masked_gradient_bit_for_bit():
    from wc_gan_amd import ops
    shape = (16, 16, 16, 128)
    d = _inputs(17, shape)
    M, C = int(np.prod(shape[:-1])), shape[-1]
    for p in PATTERNS:
        with Poison(p) as P:
            x, gy = P.guarded(d['x']), P.guarded(d['gy'])
            gamma, beta, slot = P.guarded(d['gamma']), P.guarded(d['beta']), P.guarded(d['slot'])
            s, sq = ops.std_stats(x.view(M, C))
            mu, w, a, b = ops.std_factor(s, sq, M, C, 1e-3, 0.99, 0, True, None, None, gamma, beta, x.device)
            y = ops.std_apply(x, a, b, slot, relu=True)

            def bwd(g, relu):
                gsum, gxsum = ops.std_bwd_reduce(x, g, a, b, slot, K_CLASSES, relu=relu)
                dgamma, dbeta, q, r = ops.std_bwd_factor(gsum, gxsum, mu.view(-1), w.view(-1), gamma, M)
                return ops.std_bwd_apply(x, g, a, b, q, r, slot, relu=relu), dgamma, dbeta
            one = bwd(gy, True)
            two = bwd((gy * (y > 0)).contiguous(), False)
            P.check_guards()
            assert 0.2 < float((y > 0).float().mean()) < 0.8
            for u, v, name in zip(one, two, ("dx", "dgamma", "dbeta")):
                assert same_bits(u, v), (name, hex(p))


def test_a_nan_stays_in_its_element():
    """Through the apply stages with given tables: a NaN in x is a NaN in y and in dx at that element, and nowhere else in its row."""
    from wc_gan_amd import ops
    shape = (4, 6, 6, 64)
    d = _inputs(19, shape, conditional=False)
    xn = d['x'].copy()
    xn[2, 3, 4, 17] = np.nan
    C = shape[-1]
    with Poison(0x7B) as P:
        x, gy = P.guarded(xn), P.guarded(d['gy'])
        a, b = P.guarded(d['gamma']), P.guarded(d['beta'])
        q, r = P.guarded(0.1 * d['gamma'][0]), P.guarded(d['beta'][0])
        for relu in (False, True):
            y = ops.std_apply(x, a, b, None, relu=relu).cpu().numpy()
            dx = ops.std_bwd_apply(x, gy, a, b, q, r, None, relu=relu).cpu().numpy()
            for t in (y, dx):
                bad = np.argwhere(np.isnan(t))
                assert bad.tolist() == [[2, 3, 4, 17]], (relu, bad)
        P.check_guards()
    # end to end the channel's statistics are NaN, hence its column -- and nothing but its column
    out = None
    with Poison(0xFF) as P:
        out = _site(P, dict(d, x=xn))
        P.check_guards()
    for k in ("y", "dx"):
        nan = np.isnan(out[k].cpu().numpy())
        assert nan[..., 17].all() and not np.delete(nan, 17, axis=-1).any(), k


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_replayed_graph_are_bit_identical():
    from wc_gan_amd.functional import standardize_color
    shape = (32, 16, 16, 256)
    d = _inputs(23, shape)
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev)
    xs = t(d['x']).requires_grad_(True)
    gamma, beta = t(d['gamma']).requires_grad_(True), t(d['beta']).requires_grad_(True)
    slot, gy = t(d['slot']), t(d['gy'])
    mm, mv = t(d['mm']), t(d['mv'])

    def step():
        for p in (xs, gamma, beta):
            p.grad = None
        y = standardize_color(xs, gamma, beta, slot, mm, mv, True, 1e-3, 0.99, 0, relu=True)
        gx, gg, gb = torch.autograd.grad(y, (xs, gamma, beta), gy)
        return y.detach(), gx, gg, gb

    def fresh():
        mm.copy_(t(d['mm'])); mv.copy_(t(d['mv']))

    CALLS = 3
    eager = []
    for _ in range(2):
        fresh()
        for _ in range(CALLS):
            r = step()
        torch.cuda.synchronize()
        eager.append([v.clone() for v in r] + [mm.clone(), mv.clone()])
    for u, v in zip(*eager):
        assert same_bits(u, v)

    fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    fresh()                                      # (the capture launched nothing: the moving statistics start over)
    for _ in range(CALLS):
        graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(eager[0], list(static) + [mm, mv]):
        assert same_bits(u, v)


@pytest.mark.parametrize("conditional", [False, True])
def test_grouped_forward_equals_separate_calls_bit_for_bit(conditional):
    from wc_gan_amd.functional import standardize_color, standardize_color_grouped
    shape = (5 * 64, 8, 8, 128)
    d = _inputs(29, shape, conditional=conditional)
    for p in PATTERNS:
        with Poison(p) as P:
            x, gamma, beta = P.guarded(d['x']), P.guarded(d['gamma']), P.guarded(d['beta'])
            slot = None if d['slot'] is None else P.guarded(d['slot'])
            mm, mv = P.guarded(d['mm']), P.guarded(d['mv'])
            mm1, mv1 = P.guarded(d['mm']), P.guarded(d['mv'])
            with torch.no_grad():
                y = standardize_color_grouped(x, 5, gamma, beta, slot, mm, mv, 1e-3, 0.99, 0, relu=True)
                parts = [standardize_color(x[64 * g:64 * g + 64], gamma, beta, None if slot is None else slot[64 * g:64 * g + 64].contiguous(),
                                           mm1, mv1, True, 1e-3, 0.99, 0, relu=True) for g in range(5)]
            P.check_guards()
            assert same_bits(y, torch.cat(parts)) and same_bits(mm, mm1) and same_bits(mv, mv1)
            assert not same_bits(mm, P.guarded(d['mm']))
    y_ref, cache = R.forward(d['x'], d['gamma'], d['beta'], d['slot'], d['mm'], d['mv'], True, 1e-3, 0.99, 0, True, groups=5)
    errs = dict(y=R.rel(y.cpu().numpy(), y_ref), mm=R.rel(mm.cpu().numpy(), cache['moving_mean']), mv=R.rel(mv.cpu().numpy(), cache['moving_variance']))
    print("std grouped:", errs)
    assert errs['y'] < TOL and errs['mm'] < TOL_STAT and errs['mv'] < TOL_STAT
    xg = torch.tensor(d['x'], device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError):
        standardize_color_grouped(xg, 5, None, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer against torch's route
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_stacks(after_norm, C, K=K_CLASSES, seed=0):
    from wc_gan_amd.generator import create_norm
    torch.manual_seed(seed)
    fused = create_norm('b', after_norm, number_of_classes=K, fused_batch_norm=True)(axis=-1, name='s', channels=C).cuda()
    plain = create_norm('b', after_norm, number_of_classes=K)(axis=-1, name='s', channels=C).cuda()
    fused.npart.ddof = 1                                  # what torch's running_var holds
    with torch.no_grad():
        for p in fused.branches.parameters():
            p.add_(0.3 * torch.randn_like(p))
    plain.branches.load_state_dict(fused.branches.state_dict())
    return fused, plain


@pytest.mark.parametrize("after_norm", ["ucs", "ccs", "uccs", "n", "uconv", "ucconv"])
def test_layer_against_the_unfused_stack(after_norm):
    """Both sides fp32: 1e-5 of each tensor's maximum (the two-route generator test uses 2e-5)."""
    shape = (8, 16, 16, 64)
    d = _inputs(31, shape)
    fused, plain = _two_stacks(after_norm, shape[-1])
    x0, gy = torch.tensor(d['x'], device="cuda"), torch.tensor(d['gy'], device="cuda")
    cls = torch.tensor(d['slot'], device="cuda").view(-1, 1)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    for relu in (False, True):
        res = []
        for st in (fused, plain):
            st.zero_grad()
            x = x0.clone().requires_grad_(True)
            y = st(x, cls, relu=True) if (relu and st is fused) else (torch.relu(st(x, cls)) if relu else st(x, cls))
            y.backward(gy)
            res.append((y.detach(), x.grad, {n: p.grad.clone() for n, p in st.branches.named_parameters()}))
        (yf, dxf, gf), (yp, dxp, gp) = res
        worst = max(float((gf[n] - gp[n]).abs().max() / gp[n].abs().max()) for n in gp) if gp else 0.0
        print(f"std layer {after_norm} relu={relu}: y={float((yf - yp).abs().max() / yp.abs().max()):.2e} "
              f"dx={float((dxf - dxp).abs().max() / dxp.abs().max()):.2e} params={worst:.2e}")
        assert close(yf, yp)
        if relu:
            agree = (yf > 0) == (yp > 0)
            frac = 1.0 - float(agree.float().mean())
            print(f"   masks disagree on {frac:.2e} of the elements")
            assert frac < 1e-5
            assert float(((dxf - dxp) * agree).abs().max()) <= 1e-5 * float(dxp.abs().max())
        else:
            assert close(dxf, dxp)
        for n in gp:
            assert close(gf[n], gp[n]), n
    assert float((fused.npart.moving_mean - plain.norm_layer.bn.running_mean).abs().max()) <= 1e-6 * float(plain.norm_layer.bn.running_mean.abs().max())
    assert float((fused.npart.moving_variance - plain.norm_layer.bn.running_var).abs().max()) <= 1e-6 * float(plain.norm_layer.bn.running_var.abs().max())


def test_a_fused_site_launches_only_this_librarys_kernels():
    """A profiled forward of a fused `ucs` site under no_grad: every kernel is one of csrc/wc_std.hip's -- no torch kernel touches the
    activation."""
    from torch.profiler import ProfilerActivity, profile
    fused, _ = _two_stacks('ucs', 128)
    x = torch.randn(16, 16, 16, 128, device="cuda")
    with torch.no_grad():
        fused(x, None, relu=True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fused(x, None, relu=True)
            torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not kernels:         # (a profiler build that does not tag device events: every kernel's name still says "kernel")
        kernels = [e.name for e in prof.events() if "kernel" in e.name.lower() and not e.name.startswith(("aten::", "hip", "cuda"))]
    print("std site kernels:", kernels)
    own = ("std_reduce_kernel", "std_combine_kernel", "std_factor_kernel", "std_apply_kernel")
    assert kernels and all(any(k in name for k in own) for name in kernels), kernels
    assert sum("std_apply_kernel" in n for n in kernels) == 1 and sum("std_reduce_kernel" in n for n in kernels) == 1
    assert len(kernels) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# the generator and the step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_norm_generator_on_both_routes():
    """make_generator(**baseline_config(...)) against the same with fused_batch_norm=False, same weights and noise: images at 1e-5,
    parameter gradients at 1e-4 of each tensor's maximum."""
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import CONFIGS, baseline_config
    kw = baseline_config(CONFIGS['cifar10_uncond'])['generator']
    torch.manual_seed(3)
    Gf = make_generator(**kw).cuda()
    Gp = make_generator(**dict(kw, fused_batch_norm=False)).cuda()
    with torch.no_grad():
        for m in Gf.modules():
            if type(m).__name__ == 'BatchStandardization':
                m.ddof = 1
            if type(m).__name__ == 'CenterScale':
                m.gamma.add_(0.2 * torch.randn_like(m.gamma)); m.beta.add_(0.2 * torch.randn_like(m.beta))
    missing = Gp.load_state_dict({k: v for k, v in Gf.state_dict().items() if 'moving_' not in k}, strict=False)
    assert not missing.unexpected_keys and all('bn.' in k for k in missing.missing_keys), missing
    z = torch.randn(64, 128, device="cuda")
    gimg = torch.randn(64, 32, 32, 3, device="cuda")
    from wc_gan_amd import functional as WF
    outs, masks = [], []
    try:
        for G in (Gf, Gp):
            # ReLU decisions on values within rounding of zero differ between the routes (a handful per 16 M elements, each an O(1)
            # term of a gradient sum): torch's route takes the fused route's decisions (functional.MASK_TAP)
            WF.MASK_TAP = {'record': masks} if G is Gf else {'replay': list(masks)}
            G.zero_grad()
            img = G(z)
            img.backward(gimg)
            assert G is Gf or not WF.MASK_TAP['replay'], "the two routes did not run the same ReLU'd sites"
            outs.append((img.detach(), {n: p.grad.clone() for n, p in G.named_parameters()}))
    finally:
        WF.MASK_TAP = None
    assert len(masks) == 7
    (imf, gf), (imp, gp) = outs
    e_img = float((imf - imp).abs().max() / imp.abs().max())
    # The bias of a block convolution (conv1, conv2, shortcut) adds a per-channel constant that the next batch norm takes away again
    # (conv2's and the shortcut's pass through the next 1x1 shortcut as constants first): its gradient is ZERO in exact arithmetic and
    # what either route returns is the rounding residue of a cancelling sum, so "1e-4 of its own maximum" is 0 / 0 there.  Such a
    # tensor is held to 1e-4 of the maximum of its layer's WEIGHT gradient (the un-cancelled sum over the same positions) -- and is
    # itself asserted to be residue at that scale on both routes.
    import re
    zero = {n: re.match(r"(blocks\.\d+\.(conv1|conv2|shortcut)\.conv)\.bias$", n) for n in gp}
    scale = {n: float(gp[zero[n].group(1) + ".weight" if zero[n] else n].abs().max()) for n in gp}
    rels = {n: float((gf[n] - gp[n]).abs().max()) / scale[n] for n in gp}
    residue = {n: max(float(gf[n].abs().max()), float(gp[n].abs().max())) / scale[n] for n in gp if zero[n]}
    print("   zero-gradient biases, residue over the layer's weight-gradient maximum:", {n: f"{v:.1e}" for n, v in residue.items()})
    worst = max(rels, key=rels.get)
    print(f"std generator: images {e_img:.2e}, worst parameter gradient {worst} {rels[worst]:.2e}")
    for n in sorted(rels, key=rels.get, reverse=True)[:25]:
        print(f"   {n}: rel {rels[n]:.2e}  abs {float((gf[n] - gp[n]).abs().max()):.2e}  max|ref| {float(gp[n].abs().max()):.2e}  scale {scale[n]:.2e}")
    assert sorted(gf) == sorted(gp)
    assert e_img < 1e-5
    assert len(residue) == 9 and all(v < 1e-4 for v in residue.values()), residue
    assert all(v < 1e-4 for v in rels.values()), {n: v for n, v in rels.items() if v >= 1e-4}


def test_one_captured_step_of_the_baseline_config_and_its_single_grouped_pass():
    from wc_gan_amd.layers import supports_statistic_groups
    from wc_gan_amd.train import CONFIGS, baseline_config, build_trainer
    cfg = baseline_config(CONFIGS['cifar10_uncond'])
    torch.manual_seed(5)
    tr = build_trainer(cfg, "cuda")
    assert supports_statistic_groups(tr.G)
    reals = [(torch.rand(64, 32, 32, 3) * 2 - 1).cuda() for _ in range(2)]
    batches = []
    hook = tr.G.register_forward_pre_hook(lambda m, args: batches.append(args[0].shape[0]))
    d_loss, g_loss = tr.step(reals)
    hook.remove()
    assert sorted(batches) == [128, 320], batches                   # the critic phase's five generator passes are ONE grouped pass
    assert bool(torch.isfinite(d_loss)) and bool(torch.isfinite(g_loss))
    mv_before = [m.moving_variance.clone() for m in tr.G.modules() if hasattr(m, 'moving_variance')]
    replay = tr.capture(reals, warmup=1)
    d_loss, g_loss = replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d_loss)) and bool(torch.isfinite(g_loss))
    mv_after = [m.moving_variance for m in tr.G.modules() if hasattr(m, 'moving_variance')]
    assert len(mv_after) == 7 and all(not torch.equal(a, b) for a, b in zip(mv_before, mv_after))
