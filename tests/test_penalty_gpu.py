"""The gradient penalty on the HIP route: the kernels of csrc/wc_gp.hip one by one, the engine of wc_gan_amd/penalty.py on the block
convolution kernels against tests/critic_reference.Critic in float64 (torch's double backward, the engine's ReLU masks forced into it), and
the 'wgan' trainer: one update against a float64 reference step, then a captured step.

BOUNDS: per tensor kind, four times the worse of the two fp32 routes against float64 -- the HIP engine, and torch's double backward through
torch's own convolutions on the same GPU --, rounded up to one digit, capped at the project's 1e-4 (the rule of tests/test_critic_gpu.py).
`PYTHONPATH=. python tests/test_penalty_gpu.py` prints the table (profiles/wgan_parity.txt)."""
import pytest
import torch

import critic_reference as R
import penalty_reference as PR

WEIGHT = 10.0
MASK_BAND = 1e-4
CEILING = 1e-4
# relative error = max |a - ref| / max |ref| per tensor, the worst tensor of a kind, the worst of the rows of profiles/wgan_parity.txt
# (first and second call of every engine case), the larger of the two routes, x 4, rounded up to one digit:
#   conv_w   hip 4.75e-07  torch fp32 2.71e-06  -> 1.1e-05 -> 2e-05
#   head     hip 3.31e-07  torch fp32 2.25e-07  -> 1.3e-06 -> 2e-06
#   norms    hip 1.24e-07  torch fp32 1.47e-07  -> 5.9e-07 -> 6e-07
#   penalty  hip 1.43e-07  torch fp32 6.61e-08  -> 5.7e-07 -> 6e-07
BOUNDS = dict(conv_w=2e-5, head=2e-6, norms=6e-7, penalty=6e-7)
assert all(b <= CEILING for b in BOUNDS.values())

SMALL = dict(input_image_shape=(16, 16, 3), block_sizes=(128, 128, 128, 128), resamples=('DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=10,
             spectral=False)
RECIPE = dict(SMALL, input_image_shape=(32, 32, 3))
# (label, critic keywords, batch): the smallest grid the block kernels take (8 x 4 x 4 = 128 rows in the last two blocks), and the recipe's own
CASES = [('16x16 N=8 head None sum', dict(SMALL, type=None, sum_pool=True), 8),
         ('16x16 N=8 head None mean', dict(SMALL, type=None, sum_pool=False), 8),
         ('16x16 N=8 PROJECTIVE sum', dict(SMALL, type='PROJECTIVE', sum_pool=True), 8),
         ('16x16 N=8 PROJECTIVE mean', dict(SMALL, type='PROJECTIVE', sum_pool=False), 8),
         ('32x32 N=64 head None sum', dict(RECIPE, type=None, sum_pool=True), 64)]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _ulp32(x64):
    """the spacing of fp32 at |x| (x float64, inside fp32's normal range or zero)"""
    a = x64.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


# ---------------------------------------------------------------------------------------------------------------------------------
# the masked split
# ---------------------------------------------------------------------------------------------------------------------------------
class _Site:
    training = True


def _tangent(shape, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    t = torch.randn(shape, generator=g)
    a = torch.randn(shape, generator=g)
    flat = a.view(-1)
    flat[::7] = 0.0                     # exact zeros and negative zeros: both take the slope (a > 0 is false)
    flat[3::11] = -0.0
    return t.cuda(), a.cuda()


def _same_planes(got, want, what):
    for g, w, name in zip(got, want, ('hi', 'lo')):
        assert torch.equal(_bits(g), _bits(w)), (what, name)
    assert torch.equal(_bits(got[2][:1]), _bits(want[2][:1])), (what, 'scale')


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 4, 128), (8, 16, 16, 128), (3, 5, 7, 12)])       # 1260 floats: no multiple of a workgroup's 1024
@pytest.mark.parametrize("slope", [0.0, 0.3])
def test_masked_split_has_the_bits_of_the_split_of_the_premultiplied_tensor(shape, slope):
    from wc_gan_amd import conv as C
    t, a = _tangent(shape, 5)

    def pre(t):
        return (t * torch.where(a > 0, 1.0, slope).to(torch.float32)).contiguous()
    _same_planes(C.split_planes_masked(t, a, slope), C.split_planes(pre(t)), 'no site')
    mine, theirs = _Site(), _Site()
    redo = lambda site, role: int(site._wc_split_hist[role][0][C.HIST_REDO:C.HIST_REDO + 1].view(torch.int32))
    for call, factor in enumerate((1.0, 1.25, 1000.0 * 1.25)):       # measuring call, history call, a 1000-fold growth
        tt = (t * factor).contiguous()
        _same_planes(C.split_planes_masked(tt, a, slope, site=mine, role='t'), C.split_planes(pre(tt), site=theirs, role='g'), f'site call {call}')
        assert redo(mine, 't') == redo(theirs, 'g') == (1 if call == 2 else 0)      # the gated second pass, taken exactly once
    assert torch.equal(_bits(mine._wc_split_hist['t'][0]), _bits(theirs._wc_split_hist['g'][0]))       # the records themselves


# ---------------------------------------------------------------------------------------------------------------------------------
# rows and interpolation
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows_case(N, L, seed, only=None):
    g = torch.randn(N, L, generator=torch.Generator().manual_seed(seed))
    scales = {0: 0.0, 1: 1e-20, 2: 1e15}
    for row, s in scales.items():
        if only is not None:
            if row == only:
                g[0] *= s
        elif row < N:
            g[row] *= s
    return g.cuda()


def _check_rows(g):
    from wc_gan_amd import penalty
    N = g.shape[0]
    norms, v, pen = penalty.penalty_rows(g, WEIGHT)
    g64 = g.double()
    n64 = g64.norm(dim=1)
    coef = torch.where(n64 > 0, (2 * WEIGHT / N) * (1 - 1 / n64), torch.zeros_like(n64))
    v64 = coef[:, None] * g64
    p64 = (WEIGHT / N) * ((n64 - 1) ** 2).sum()
    assert pen.dim() == 0 and torch.isfinite(v).all() and torch.isfinite(norms).all()
    assert ((norms.double() - n64).abs() <= 4 * _ulp32(n64)).all()
    assert ((v.double() - v64).abs() <= 4 * _ulp32(v64)).all()
    assert not v[n64 == 0].any()
    assert abs(float(pen) - float(p64)) <= 1e-6 * float(p64)
    again = penalty.penalty_rows(g, WEIGHT)
    for x, y in zip((norms, v, pen), again):
        assert torch.equal(_bits(x.reshape(-1)), _bits(y.reshape(-1)))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [768, 3072, 6912])
def test_rows_kernel_against_float64(L):
    for N in (3, 64):
        _check_rows(_rows_case(N, L, 10 + N))           # rows 0, 1, 2: zero, x 1e-20, x 1e+15
    for only in (None, 0, 1, 2):                        # N = 1: an ordinary row, then each special row alone
        _check_rows(_rows_case(1, L, 20, only=only) if only is not None else torch.randn(1, L, generator=torch.Generator().manual_seed(21)).cuda())


@pytest.mark.gpu
def test_interpolation_within_one_ulp():
    from wc_gan_amd import penalty
    g = torch.Generator().manual_seed(3)
    real, fake = (torch.randn(5, 8, 8, 3, generator=g).cuda() for _ in range(2))
    eps = torch.rand(5, generator=g).cuda()
    eps[0], eps[1] = 0.0, 1.0
    x = penalty.interpolate(real, fake, eps)
    e = eps.double().view(5, 1, 1, 1)
    x64 = e * real.double() + (1 - e) * fake.double()
    assert ((x.double() - x64).abs() <= _ulp32(x64)).all()
    assert torch.equal(x[0], fake[0]) and torch.equal(x[1], real[1])
    torch.cuda.manual_seed(11)
    a = penalty.interpolate(real, fake)
    torch.cuda.manual_seed(11)
    assert torch.equal(a, penalty.interpolate(real, fake, torch.rand(5, device='cuda')))


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------------------
def _module(kw, seed=5):
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(seed)
    D = make_discriminator(**kw)
    with torch.no_grad():
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.cuda()


def _inputs(kw, batch, seed):
    g = torch.Generator().manual_seed(seed)
    H, W, C = kw['input_image_shape']
    x = (torch.rand(batch, H, W, C, generator=g) * 2 - 1).cuda()
    cls = torch.randint(0, kw['number_of_classes'], (batch, 1), generator=g, dtype=torch.int32).cuda()
    return x, cls


def _kind(name):
    return 'conv_w' if name.startswith('blocks.') else 'head'


def _errors(D, kw, x, cls, pen, norms, grads, masks):
    """-> {kind: worst relative error} of one fp32 result against the float64 reference with that route's masks forced"""
    pen64, norms64, grads64, critic = PR.reference_penalty(kw['_state'], {k: v for k, v in kw.items() if k != '_state'}, x, cls, WEIGHT, masks)
    worst, count = R.mask_disagreement(masks, critic.pre)
    print(f"  relu masks: {count} elements differ from the float64 signs, the farthest at {worst:.2e} of its tensor's maximum")
    assert worst <= MASK_BAND, (worst, count)
    errs = dict(conv_w=0.0, head=0.0, norms=PR.rel(norms, norms64), penalty=PR.rel(pen, pen64))
    for n, g in grads.items():
        if n.endswith('.bias') or n.startswith('cls_out'):
            assert not g.any() and not grads64[n].any(), n
        else:
            assert float(grads64[n].abs().max()) > 0, n
            errs[_kind(n)] = max(errs[_kind(n)], PR.rel(g, grads64[n]))
    return errs


def _hip_errors(kw, batch, calls=2):
    """the engine on one module, `calls` times on the same inputs (the second call on history-scaled splits) -> [errors per call]"""
    from wc_gan_amd import conv as C
    from wc_gan_amd import penalty
    D = _module(kw)
    D.train()
    x, cls = _inputs(kw, batch, 7)
    kw = dict(kw, _state={k: v.detach().clone() for k, v in D.state_dict().items()})
    # every convolution with 128 input channels is one the block kernels take (a failure, not a skip: the test is about that route)
    H = kw['input_image_shape'][0]
    w3, w1 = D.blocks[1].conv1.conv.weight, D.blocks[1].shortcut.conv.weight
    for h, kind, w in ((H, 'down3', w3), (H // 2, 'same', w3), (H // 2, 'down3', w3), (H // 4, 'same', w1), (H // 4, 'same', w3)):
        assert C.supported(torch.empty(batch, h, h, 128, device='cuda'), w, kind), (batch, h, kind)
    out = []
    for call in range(calls):
        for p in D.parameters():
            p.grad = None
        pen, norms = penalty.gradient_penalty(D, x, cls if kw['type'] == 'PROJECTIVE' else None, WEIGHT)
        # 4 blocks x (conv1, conv2) + 2 shortcuts, four calls each; torch only for the data gradients of the two image layers
        assert penalty.last_route == {'hip': 38, 'torch': 2}, penalty.last_route
        assert len(penalty.last_masks) == R.relu_count(kw['block_sizes'])
        for blk in D.blocks:
            for layer in (blk.conv1, blk.conv2):
                book = layer.__dict__.get('_wc_split_hist', {})
                if layer.conv.in_channels == 128:
                    assert {'p', 't', 'd'} <= set(book) and all(book[r][1] for r in 'ptd') and not {'x', 'g'} & set(book)
        grads = {n: p.grad.detach().clone() for n, p in D.named_parameters()}
        out.append(_errors(D, kw, x, cls, pen, norms, grads, penalty.last_masks))
    return out


def _torch_errors(kw, batch):
    """what a user can write today: torch's double backward in fp32 through torch's convolutions on the same GPU"""
    import wc_gan_amd.conv as C
    import wc_gan_amd.generator as G
    D = _module(kw)
    x, cls = _inputs(kw, batch, 7)
    kw = dict(kw, _state={k: v.detach().clone() for k, v in D.state_dict().items()})
    rec, handles = {}, []
    for i, blk in enumerate(D.blocks):
        for part in ('bn1', 'bn2'):
            handles.append(getattr(blk, part).register_forward_hook(lambda _m, _i, out, key=f'{i}.{part}': rec.__setitem__(key, out.detach())))
    handles.append(D.blocks[-1].register_forward_hook(lambda _m, _i, out: rec.__setitem__('last', out.detach())))
    before = G.FAST_CONV, C.NARROW_WRW
    G.FAST_CONV = C.NARROW_WRW = False
    try:
        pen, norms, grads = PR.module_penalty(D, x, cls if kw['type'] == 'PROJECTIVE' else None, WEIGHT)
    finally:
        G.FAST_CONV, C.NARROW_WRW = before
        for h in handles:
            h.remove()
    keys = [k for i in range(len(D.blocks)) for k in ((f'{i}.bn1',) if i else ()) + (f'{i}.bn2',)] + ['last']
    return _errors(D, kw, x, cls, pen, norms, grads, [rec[k] > 0 for k in keys])


def _check(errs, label):
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (label, k, v, BOUNDS[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(' ', '_') for c in CASES])
def test_engine_on_the_hip_route_in_two_calls(case):
    label, kw, batch = CASES[case]
    for call, errs in enumerate(_hip_errors(kw, batch)):
        _check(errs, f"penalty {label} call {call + 1}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wgan_trainer_update_and_captured_step():
    from wc_gan_amd.train import WGAN_CONFIGS, build_trainer
    from wc_gan_amd import penalty
    cfg = WGAN_CONFIGS['cifar10_wgan_uncond']
    n = 16
    tr = build_trainer(cfg, 'cuda', batch_size=n, training_ratio=1, seed=3)
    assert (tr.objective, tr.gp_weight) == ('wgan', 10.0)
    with torch.no_grad():
        for name, p in tr.D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    g = torch.Generator().manual_seed(8)
    real, fake = ((torch.rand(n, 32, 32, 3, generator=g) * 2 - 1).cuda() for _ in range(2))
    eps = torch.rand(n, generator=g).cuda()
    state = {k: v.detach().clone() for k, v in tr.D.state_dict().items()}

    # the signs the critic applies its ReLUs to in the Wasserstein pass (the penalty walks the blocks itself: these hooks see that pass only)
    rec, handles = {}, []
    for i, blk in enumerate(tr.D.blocks):
        for part in ('bn1', 'bn2'):
            handles.append(getattr(blk, part).register_forward_hook(lambda _m, _i, out, key=f'{i}.{part}': rec.__setitem__(key, out.detach())))
    handles.append(tr.D.blocks[-1].register_forward_hook(lambda _m, _i, out: rec.__setitem__('last', out.detach())))
    seen, step = {}, tr.opt_d.step

    def spy(*a, **k):
        seen.update({k_: p.grad.detach().clone() for k_, p in tr.D.named_parameters()})
        return step(*a, **k)
    tr.opt_d.step = spy
    loss = tr.d_step(real, fake=fake, cls=None, eps=eps)
    tr.opt_d.step = step
    for h in handles:
        h.remove()
    kw = dict(cfg['discriminator'])
    # the float64 step: the Wasserstein loss through critic_reference.Critic with that pass's masks, the penalty with the engine's
    keys = [k for i in range(len(tr.D.blocks)) for k in ((f'{i}.bn1',) if i else ()) + (f'{i}.bn2',)] + ['last']
    w_masks = [rec[k] > 0 for k in keys]
    params, buffers = R.leaves(state)
    w_critic = R.Critic(params, buffers, iterations=0, masks=w_masks, **kw)
    out64 = w_critic(torch.cat([real, fake]).double(), None)
    w_loss = out64[n:].mean() - out64[:n].mean()
    halves = [torch.autograd.grad(part, list(params.values()), retain_graph=True) for part in (out64[n:].mean(), out64[:n].mean())]
    w_grads = {k: a - b for k, a, b in zip(params, *halves)}
    w_size = {k: float(a.abs().max() + b.abs().max()) for k, a, b in zip(params, *halves)}
    worst, count = R.mask_disagreement(w_masks, w_critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    x_hat = penalty.interpolate(real, fake, eps)
    pen64, norms64, grads64, critic = PR.reference_penalty(state, kw, x_hat, None, WEIGHT, penalty.last_masks)
    worst, count = R.mask_disagreement(penalty.last_masks, critic.pre)
    assert worst <= MASK_BAND, (worst, count)
    assert PR.rel(tr.last_penalty, pen64) < BOUNDS['penalty'] and PR.rel(tr.last_grad_norms, norms64) < BOUNDS['norms']
    # A sum of parts, each held to its own bound relative to its own maximum: the penalty to BOUNDS, the Wasserstein pass to
    # tests/test_critic_gpu.py's (out 3e-6, conv_w 6e-6, bias 2e-6, head 5e-6) -- per half of the batch, since the gradient is linear in the
    # output weights and the real half's (all -1/n) and the generated half's (all +1/n) largely cancel in the difference
    PASS = dict(out=3e-6, conv_w=6e-6, bias=2e-6, head=5e-6)
    assert abs(float(loss) - float(w_loss.detach() + pen64)) < 2 * PASS['out'] * float(out64.abs().max()) + BOUNDS['penalty'] * float(pen64)
    lr = 2e-4
    for name, p in tr.D.named_parameters():
        want = w_grads[name].detach() + grads64[name]
        kind = 'bias' if name.endswith('.bias') else _kind(name)
        tol = PASS[kind] * w_size[name] + BOUNDS.get(kind, 0.0) * float(grads64[name].abs().max())
        err = float((seen[name].double() - want).abs().max())
        print(f"  {name}: error {err:.2e}, allowed {tol:.2e}")
        assert err <= tol, (name, err, tol)
        # Adam's first update with beta1 = 0 is -lr g / (|g| + 1e-8); a gradient error of at most tol moves it by at most
        # lr tol 1e-8 / (|g| - tol + 1e-8)^2 (the map's slope at the nearest point the true gradient can lie), never by more than 2 lr
        if not want.any():          # out.bias: the Wasserstein loss's +1/n and -1/n cancel exactly, and the penalty adds nothing
            assert name == 'out.bias' and not seen[name].any() and torch.equal(p.detach(), state[name])
            continue
        moved = p.detach().double() - state[name].double()
        slack = lr * tol * 1e-8 / ((want.abs() - tol).clamp_min(0) + 1e-8) ** 2
        allowed = 1e-7 + slack.clamp_max(2 * lr)
        assert ((moved + lr * want / (want.abs() + 1e-8)).abs() <= allowed).all(), name
        assert (allowed < 1e-6).any(), name         # (the check says something)

    before = {k: p.detach().clone() for k, p in tr.D.named_parameters()}
    replay = tr.capture([real])
    for _ in range(2):
        d_loss, g_loss = replay()
    torch.cuda.synchronize()
    assert torch.isfinite(d_loss) and torch.isfinite(g_loss) and torch.isfinite(tr.last_penalty) and torch.isfinite(tr.last_grad_norms).all()
    for name, p in tr.D.named_parameters():          # (out.bias: its gradient is exactly zero under this objective)
        assert torch.equal(before[name], p.detach()) == (name == 'out.bias'), name


if __name__ == '__main__':
    kinds = ('conv_w', 'head', 'norms', 'penalty')
    print(f"{'critic':<40}{'route':<12}" + ''.join(f"{k:>10}" for k in kinds), flush=True)
    worst = {route: dict.fromkeys(kinds, 0.0) for route in ('hip', 'torch fp32')}
    BOUNDS = dict.fromkeys(kinds, CEILING)
    for label, kw, batch in CASES:
        rows = [(f"{label} call {i + 1}", 'hip', e) for i, e in enumerate(_hip_errors(kw, batch))] + [(label, 'torch fp32', _torch_errors(kw, batch))]
        for name, route, errs in rows:
            print(f"{name:<40}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" for k in kinds), flush=True)
            for k in kinds:
                worst[route][k] = max(worst[route][k], errs[k])
    for route in worst:
        print(f"{'worst':<40}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in kinds), flush=True)
