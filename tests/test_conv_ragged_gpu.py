"""The block convolutions on a partial last tile (csrc/wc_conv.hip: N*H*W of the virtual grid a multiple of 32, not of 128; DESIGN.md
section 4.21) against torch's float64 convolution of the same map, against the whole-tile route bit for bit, on guard-banded memory, and
through the MNIST recipes' networks.  Reference, inputs and tolerances are tests/test_conv_gpu.py's and tests/test_conv_dispatch_gpu.py's
(imported; the bound on dW, which both files write as the literal 2e-5 = 2 * TOL beside MIOpen's name, is written 2 * TOL here).

`PYTHONPATH=. python tests/test_conv_ragged_gpu.py` prints the measured error of every row (profiles/ragged_conv_parity.txt)."""
import copy

import pytest
import torch

from test_conv_dispatch_gpu import _ref3
from test_conv_gpu import TOL, _ref, _rel, _weights

DW_TOL = 2 * TOL

# kind, N, H, W, Cin, Cout, k, N*H*W % 128, (forward, data-gradient) k-split count, taken
ROWS = [
    ('same', 2, 4, 4, 128, 128, 3, 32, (8, 8), True),            # a single partial tile
    ('same', 6, 4, 4, 128, 128, 3, 96, (8, 8), True),
    ('same', 10, 4, 4, 128, 128, 1, 32, (1, 1), True),           # 160 points; iters = 4, no k-split
    ('same', 4, 7, 14, 128, 256, 3, 8, None, False),             # 392 = 3 * 128 + 8: no multiple of 32, refused with the flag on
    ('same', 32, 7, 7, 128, 256, 3, 32, (8, 8), True),           # 1568 points, a tile straddling images
    ('up3', 64, 7, 7, 256, 256, 3, 64, (1, 8), True),            # the recipe's conv1
    ('up3', 64, 7, 7, 128, 128, 3, 64, (1, 8), True),            # 25 * 4 = 100 workgroups, past the k-split gate; strided data gradient
    ('down3', 32, 14, 14, 128, 128, 3, 32, (8, 4), True),        # output grid 7x7, phase data gradient on a ragged grid
    ('down', 32, 14, 14, 64, 128, 4, 32, (8, 4), True),          # the 64-wide <2, 1> tile (the data gradient's)
    ('same', 32, 7, 7, 128, 128, 3, 32, (8, 8), True),           # pair backward
    ('same', 3, 8, 8, 1024, 1024, 3, 64, (8, 8), True),          # 192 points: weight-gradient splits clamped to 192 / 32 = 6
]
_ID = lambda r: '-'.join(str(v) for v in r[:7])


def _inputs(kind, N, H, W, ci, co, k):
    torch.manual_seed(N + H + ci)
    x = (torch.randn(N, H, W, ci, device='cuda') * 1.7 + 0.3).requires_grad_(True)
    w = _weights(kind if kind == 'down' else 'same', ci, co, k).requires_grad_(True)
    b = (torch.randn(co, device='cuda') * 0.1).requires_grad_(True)
    return x, w, b


def _float64(x, w, b, kind):
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    y64 = _ref(x64, w64, b64, kind) if kind == 'down' else _ref3(x64, w64, b64, kind)
    return y64, (x64, w64, b64)


def _plan_counts(plan):
    """the k-split counts of a plan's forward and data gradient, read from its workspace sizes"""
    out = []
    for (g, _, _), ws in ((plan.fwd, plan.fwd_ws), (plan.bwd, plan.bwd_ws)):
        n = g.N * g.Hout * g.Wout * g.Cout * 4
        assert ws % n == 0
        out.append(ws // n if ws else 1)
    return tuple(out)


def _row(row):
    from wc_gan_amd import conv as C
    kind, N, H, W, ci, co, k, over, counts, taken = row
    x, w, b = _inputs(kind, N, H, W, ci, co, k)
    assert not C.supported(x, w, kind)                              # today's route declines every row: the torch fallback
    assert C.supported(x, w, kind, ragged=True) == taken
    if not taken:
        with pytest.raises(RuntimeError):
            C.fast_conv(x, w, b, kind, ragged=True)
        return None
    plan = C._plan(kind, x, w, True)
    M = plan.fwd[0].N * plan.fwd[0].H * plan.fwd[0].W
    assert M % 128 == over and M % 32 == 0 and _plan_counts(plan) == counts
    y = C.fast_conv(x, w, b, kind, ragged=True)
    gy = torch.randn_like(y)
    grads = torch.autograd.grad(y, (x, w, b), gy)
    y64, leaves = _float64(x, w, b, kind)
    assert y.shape == y64.shape and grads[1].stride() == w.stride()
    ref = (y64,) + torch.autograd.grad(y64, leaves, gy.double())
    return {n: _rel(a, r) for n, a, r in zip(('y', 'dx', 'dw', 'db'), (y,) + grads, ref)}, plan


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_ID)
def test_each_ragged_row_matches_float64(row):
    got = _row(row)
    if got is None:
        return
    errs, plan = got
    print("ragged conv", _ID(row), "M % 128 =", row[7], "k-split", row[8], errs)
    assert errs['y'] < TOL and errs['dx'] < TOL and errs['db'] < TOL, errs
    assert errs['dw'] < DW_TOL, errs
    if row[:7] == ('same', 32, 7, 7, 128, 128, 3):
        assert plan.pair
    if row[0] in ('up3', 'down'):
        assert not plan.pair


class _Site:
    """a layer object as conv.split_planes sees it"""


def _res_and_tail():
    """(32, 7, 7) 128 -> 128 through wc_conv_res_f16x3 and wc_conv_tail_f16x3 (SPLIT): errors of y against float64, of the tail's planes
    against relu(y), and whether the two entries' y have the bits of the plain launch"""
    from wc_gan_amd import _lib, conv as C
    x, w, b = _inputs('same', 32, 7, 7, 128, 128, 3)
    plan = C._plan('same', x, w, True)
    assert plan.ok and plan.res and plan.tail
    gf, kf, nf = plan.fwd
    res = torch.randn(32, 7, 7, 128, device='cuda')
    with torch.no_grad():
        planes = C.split_planes(x.detach())
        img = C.weight_image(w.detach(), gf, kf, nf)
        plain = C.run(planes, img, gf, b.detach(), nbytes=plan.fwd_ws)
        y_res = C.run(planes, img, gf, b.detach(), nbytes=plan.fwd_ws, res=res)
        site = _Site()
        C.split_planes(plain, relu=True, site=site, role='x')       # the reader's record, seeded by its first call
        rec = C._reader_record(site, 'x', x.device)
        assert rec is not None
        tail = C._Tail(_lib.TAIL_SPLIT, tuple(plain.shape), x.device, record=rec, role='x')
        y_tail = C.run_tail(planes, img, gf, tail, bias=b.detach(), nbytes=plan.fwd_ws)
        hi, lo, scale = tail.planes[:3]
        back = (hi.double() + lo.double()) / float(scale[0])
    y64, _ = _float64(x, w, b, 'same')
    return dict(res=_rel(y_res, y64.detach() + res.double()), tail=_rel(y_tail, y64),
                planes=float((back - y_tail.double().clamp_min(0)).abs().max() / y_tail.abs().max()),
                res_bits=torch.equal(y_res, plain + res), tail_bits=torch.equal(y_tail, plain))


@pytest.mark.gpu
def test_the_res_and_tail_finishes_on_a_ragged_grid():
    e = _res_and_tail()
    print("ragged conv res / tail", e)
    assert e['res'] < TOL and e['tail'] < TOL
    assert e['planes'] < 2.0 ** -20                                  # test_conv_gpu.py's bound on a history-scaled split
    assert e['res_bits'] and e['tail_bits']


# kind, H, Cin, Cout, k, N (ragged), N' (whole tiles): both calls have the same k-split counts
BITS = [('same', 4, 128, 128, 3, 2, 8), ('same', 4, 256, 128, 1, 6, 8), ('down3', 8, 128, 128, 3, 2, 8), ('up3', 4, 128, 128, 3, 6, 8),
        ('same', 6, 128, 128, 3, 8, 32),                 # 288 against 1152 points: tiles that straddle images, k-split 8 in both
        ('same', 7, 128, 128, 1, 32, 128)]              # the recipes' 7x7 grid (1 x 1: no k-split at either batch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,H,ci,co,k,N,N2", BITS, ids=lambda v: str(v))
def test_same_bits_as_the_whole_tile_route(kind, H, ci, co, k, N, N2):
    """N images on a partial last tile against N' > N images -- the same first N -- on whole tiles: y[:N], and dx[:N] for an output
    gradient that is zero beyond N, have the same bits (the same tiles, the same shares of the tap loop, the same scales)"""
    from wc_gan_amd import conv as C
    torch.manual_seed(H + N)
    x = (torch.randn(N, H, H, ci, device='cuda') * 1.7 + 0.3)
    extra = torch.randn(N2 - N, H, H, ci, device='cuda') * 0.2
    assert float(extra.abs().max()) < float(x.abs().max())          # both calls measure the same scale
    x2 = torch.cat([x, extra]).requires_grad_(True)
    x = x.requires_grad_(True)
    w = _weights('same', ci, co, k)
    b = torch.randn(co, device='cuda') * 0.1
    p, p2 = C._plan(kind, x, w, True), C._plan(kind, x2, w)
    assert p.ok and p2.ok and not C.supported(x, w, kind) and C.supported(x2, w, kind)
    assert (p.fwd[0].N * p.fwd[0].H * p.fwd[0].W) % 128 != 0 and (p2.fwd[0].N * p2.fwd[0].H * p2.fwd[0].W) % 128 == 0
    assert _plan_counts(p) == _plan_counts(p2)
    y = C.fast_conv(x, w, b, kind, ragged=True)
    y2 = C.fast_conv(x2, w, b, kind)
    assert torch.equal(y, y2[:N])
    gy = torch.randn_like(y)
    gy2 = torch.cat([gy, torch.zeros_like(y2[N:])])
    dx, = torch.autograd.grad(y, (x,), gy)
    dx2, = torch.autograd.grad(y2, (x2,), gy2)
    assert torch.equal(dx, dx2[:N])


STRAY = [('same', 2, 4, 4, 128, 128, 3), ('same', 6, 4, 4, 128, 128, 3), ('up3', 64, 7, 7, 128, 128, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,H,W,ci,co,k", STRAY, ids=lambda v: str(v))
def test_no_stray_writes_and_every_valid_row_written(kind, N, H, W, ci, co, k):
    """outputs, k-split partial sums, planes and weight images allocated inside poisoned guard bands (tests/_poison.py, as
    test_poison_gpu.py does): the bands are intact behind forward and backward, the results do not depend on the fill, and under the
    NaN fill no NaN is left in y, dx, dW or db"""
    from _poison import run_patterns
    from wc_gan_amd import conv as C
    g = torch.Generator().manual_seed(N + H + ci)
    x = torch.randn(N, H, W, ci, generator=g) * 1.7 + 0.3
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    Ho, Wo = (2 * H, 2 * W) if kind == 'up3' else (H, W)
    gy = torch.randn(N, Ho, Wo, co, generator=g)

    def run(P):
        xd = P.guarded(x).requires_grad_(True)
        wd = P.guarded(w).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bd = P.guarded(b).requires_grad_(True)
        p = C._plan(kind, xd, wd, True)
        assert p.ok and (p.fwd_ws > 0 or p.bwd_ws > 0)
        y = C._FastConv.apply(xd, wd, bd, kind, p)
        return [y] + list(torch.autograd.grad(y, (xd, wd, bd), P.guarded(gy)))

    outs = run_patterns(run)
    for t in outs[0xFF]:
        assert not bool(torch.isnan(t).any())
    y64, leaves = _float64(x.cuda(), w.cuda(), b.cuda(), kind)
    ref = (y64,) + torch.autograd.grad(y64, leaves, gy.double().cuda())
    for t, r, tol in zip(outs[0xFF], ref, (TOL, TOL, DW_TOL, TOL)):
        assert _rel(t.cuda(), r) < tol


def _pair(name, batch):
    """the recipe's trainer with ragged_conv on and a second one with it off that holds the same weights"""
    from wc_gan_amd import train as T
    cfg = T.MNIST_CONFIGS[name]
    kw = dict(batch_size=batch, seed=3, lr=0.0, training_ratio=1)
    on = T.build_trainer(T.ragged_config(cfg), 'cuda', **kw)
    off = T.build_trainer(T.ragged_config(cfg, on=False), 'cuda', **kw)
    off.G.load_state_dict(on.G.state_dict())
    off.D.load_state_dict(on.D.state_dict())
    return on, off, cfg


NETWORKS = [('mnist_uncond', 8), ('mnist_uncond', 64), ('mnist_cond', 8), ('mnist_cond', 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,batch", NETWORKS)
def test_the_recipes_networks_agree_with_the_unmarked_route(name, batch):
    """generator image and critic output with the mark on against the same networks with it off (torch's convolutions on the 7x7 grids),
    at the bounds of test_conv_gpu.py's two-route test"""
    from wc_gan_amd import conv as C
    on, off, cfg = _pair(name, batch)
    torch.manual_seed(0)
    z = torch.randn(batch, 128, device='cuda')
    cls = torch.randint(0, 10, (batch, 1), dtype=torch.int32, device='cuda')
    for m in (on.G, on.D, off.G, off.D):
        m.eval()
    with torch.no_grad():
        img_on, img_off = on.G(z, cls), off.G(z, cls)
        c = cls if cfg['conditional'] else None
        out_on, out_off = on._d(img_on, c), off._d(img_on, c)
    assert img_on.shape == (batch, 28, 28, 1) and bool(torch.isfinite(img_on).all())
    assert float((img_on - img_off).abs().max()) < 2e-5            # tanh outputs in [-1, 1]
    assert float((out_on - out_off).abs().max()) < 1e-4 * float(out_off.abs().max()) + 1e-5
    # at batch 64 the marked layers did run the block kernels on the 7x7 grids, and the unmarked ones did not
    F_ = cfg['generator']['first_block_shape'][2]
    took = [C._plans.get(('same', (batch, 7, 7, 128), (128, 128, 3, 3), flag)) for flag in (True, False)]
    if batch == 64:
        assert took[0] and took[0].ok and took[1] is not None and not took[1].ok
        assert C._plans[('up3', (batch, 7, 7, F_), (F_, F_, 3, 3), True)].ok
    else:
        assert took[0] is not None and not took[0].ok               # 8 * 49 = 392 points: no multiple of 32, torch on both routes


# (batch 32: the critic's 2 x 32 images and the generator's 32 are both partial-tile grids at 7x7 -- the backward's finishes with tails too)
@pytest.mark.gpu
@pytest.mark.parametrize("name,batch", NETWORKS + [('mnist_cond', 32)])
def test_one_step_eagerly_and_from_the_captured_graph(name, batch):
    """tests/test_projection_tail_gpu.py's comparison (lr = 0 keeps the weights; the buffers a step moves are put back before the eager
    step) and its tolerance, on the MNIST recipes with the mark on"""
    from test_projection_tail_gpu import NET
    from wc_gan_amd import train as T
    cfg = T.ragged_config(T.MNIST_CONFIGS[name])
    tr = T.build_trainer(cfg, 'cuda', batch_size=batch, training_ratio=1, seed=3, lr=0.0)
    g = torch.Generator().manual_seed(9)
    real = (torch.rand(batch, 28, 28, 1, generator=g) * 2 - 1).cuda()
    labels = [torch.randint(0, 10, (batch,), generator=g, dtype=torch.int32).cuda()] if cfg['conditional'] else None
    replay = tr.capture([real], labels, warmup=2)
    saved = [copy.deepcopy(m.state_dict()) for m in (tr.D, tr.G)]
    torch.cuda.manual_seed(50)
    d_loss, g_loss = replay()
    torch.cuda.synchronize()
    got = [float(d_loss), float(g_loss)]
    assert all(torch.isfinite(torch.tensor(got)))
    for m, sd in zip((tr.D, tr.G), saved):
        m.load_state_dict(sd)
    torch.cuda.manual_seed(50)
    d_loss, g_loss = tr.step([real], labels)
    eager = [float(d_loss), float(g_loss)]
    assert all(torch.isfinite(torch.tensor(eager)))
    with torch.no_grad():
        size = max(1.0, float(tr.D(real, labels[0].reshape(-1, 1) if labels else None).abs().max()))
    tol = [2 * 2 * NET['out'] * 2 * size, 2 * NET['out'] * 2 * size]
    print("ragged step", name, batch, "replay", got, "eager", eager, "allowed", tol)
    for a, b_, t in zip(got, eager, tol):
        assert abs(a - b_) <= t, (got, eager, tol)


if __name__ == '__main__':
    import os
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                              'ragged_conv_parity.txt')
    lines = [f"{'row':<40}{'M % 128':>8}{'k-split':>10}" + ''.join(f"{n:>10}" for n in ('y', 'dx', 'dw', 'db'))]
    for row in ROWS:
        if not row[9]:
            lines.append(f"{_ID(row):<40}{row[7]:>8}{'refused':>10}")
            continue
        errs, _ = _row(row)
        lines.append(f"{_ID(row):<40}{row[7]:>8}{str(row[8]):>10}" + ''.join(f"{errs[n]:>10.2e}" for n in ('y', 'dx', 'dw', 'db')))
    e = _res_and_tail()
    lines.append(f"{'same-32-7-7-128-128-3 res finish':<40}{32:>8}{'(8, -)':>10}{e['res']:>10.2e}   same bits as run() + res: {e['res_bits']}")
    lines.append(f"{'same-32-7-7-128-128-3 tail finish':<40}{32:>8}{'(8, -)':>10}{e['tail']:>10.2e}   same bits as run(): {e['tail_bits']}; "
                 f"planes of relu(y): {e['planes']:.2e}")
    lines.append(f"bounds: y, dx, db {TOL:.0e}; dw {DW_TOL:.0e} (tests/test_conv_gpu.py)")
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
