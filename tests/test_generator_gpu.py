"""The ResNet WC generator as a network against tests/generator_reference.py, a float64 restatement of the reference project's generator
layer by layer (tests/test_generator_cpu.py pins that restatement against the oracle and torch.nn.functional first).

CASES: the generators of the four train.CONFIGS entries as they stand, each at the smallest batch where the first site has at least 4 C
rows and where every route decision (`_routes`: the H W >= 64 branch, the K3 -> convolution hand-over, the fast convolution kernel, the
shortcut on planes, the residual add's planes / fp32 copy / covariance partials, the bit mask and the planes backward of every site) equals
the one the recipe's own generator update (batch 64 x 2) gives.  Biases and colorings are jittered off their initial values.

Per case: two successive training-mode calls (the second on history-scaled splits and updated moving statistics) -- image, every parameter
gradient of (image * w).sum(), moving mean and covariance of every site -- then one evaluation-mode call under no_grad (the cached plan
against the reference's whitening with the module's own moving buffers), and for the two CIFAR-10 cases one forward-only call with
statistic_groups(2) at twice the batch (its residual adds are asserted against `_routes` at that batch; the recipe's own grouped pass, five
groups of 64, also writes planes behind block 0, which two groups of 80 do not).  Every figure is max|a - ref| / max|ref| per tensor, the
worst tensor of a kind.

The reference is given the signs the HIP network applied: the sites' bit masks through functional.MASK_TAP (training calls), `y > 0` of the
sites' outputs through forward hooks where a pass keeps no mask (evaluation, grouped).  CONDITIONS on those, per site: at most 1e-4 of the
elements differ from the reference's own float64 sign, and every one of them lies within 1e-4 of zero relative to its tensor's maximum.

BOUNDS: four times the error of the reference itself in fp32 on torch's kernels, with the same forced masks, against the float64 reference
on the MI355X -- the worst over all cases and calls, rounded up to one digit, capped at the project's 1e-4 (factor 4: the HIP routes'
operands carry 22 bits against fp32's 24, and it is test_critic_gpu.py's margin).  The HIP route's own error stands beside it and does not
set it.  profiles/generator_parity.txt holds every row; `PYTHONPATH=. python tests/test_generator_gpu.py` prints that table.  Its last rows,
the worst over the four recipes (two training calls and one evaluation call each) and the two grouped calls:

    kind     hip        torch fp32   x 4        bound
    image    1.88e-05   1.72e-04     6.9e-04    1e-04  (the cap)
    conv_w   6.16e-06   6.62e-05     2.6e-04    1e-04  (the cap)
    conv_b   6.46e-06   5.44e-05     2.2e-04    1e-04  (the cap)
    gamma    5.52e-06   6.07e-05     2.4e-04    1e-04  (the cap)
    beta     1.55e-05   8.03e-05     3.2e-04    1e-04  (the cap)
    dense    4.05e-06   5.24e-05     2.1e-04    1e-04  (the cap)
    moving   2.31e-07   9.88e-06     4.0e-05    4e-05

(conv_b: the last convolution's bias gradient, and the block convolutions' bias gradients -- zero in exact arithmetic -- measured on both
sides against the maximum of the same layer's weight gradient.)  The forced signs differed from the float64 signs in at most 1.5e-6 of a
site's elements, the farthest 1.3e-6 of its tensor's maximum from zero.  The float64 reference of one training call, forward and backward,
takes 0.11 - 0.53 s on the MI355X (convolutions as unfold + matmul), so every case runs whole: no block is left out.
"""
import inspect
import time

import pytest
import torch

import generator_reference as R

MASK_BAND = 1e-4            # a forced sign that differs from the float64 sign lies this close to zero (of its tensor's maximum) ...
MASK_SHARE = 1e-4           # ... and at most this share of a site's elements differ
CEILING = 1e-4
BOUNDS = dict(image=1e-4, conv_w=1e-4, conv_b=1e-4, gamma=1e-4, beta=1e-4, dense=1e-4, moving=4e-5)          # (the table above)
assert set(BOUNDS) == set(R.KINDS) and all(b <= CEILING for b in BOUNDS.values())

# recipe -> batch.  First site: batch x 16 (x 36: STL-10) rows >= 4 C; the routes of `_routes` equal those at RECIPE_BATCH (asserted).
# Scanned in steps of 4 from 8: below 80 the residual add of block 1 (16 x 16) writes no planes, so block 2's norm1 and shortcut read fp32
# and that site's backward reads no planes; STL-10 below 128 loses the bits-only backward of the 12 x 12 sites (96: 13824 rows) as well --
# its case is the recipe's own batch.
CASES = {'cifar10_uncond': 80, 'cifar10_cond': 80, 'stl10_uncond': 128, 'tinyimagenet_cond_sa': 80}
GROUPED = ('cifar10_uncond', 'cifar10_cond')
RECIPE_BATCH = 128          # GanTrainer's batch_size 64 x generator_batch_multiple 2 (run.py:293-294)
REFERENCE_SECONDS = {}      # label of a call -> what its float64 reference alone took


def _kw(recipe):
    from wc_gan_amd.train import CONFIGS
    return CONFIGS[recipe]['generator']


def _module(recipe, device, seed=7):
    """the recipe's generator with its biases, coloring kernels and class matrices off their initial values (a term that is dropped, or a
    bias that starts at zero, would not show otherwise)"""
    from wc_gan_amd.generator import make_generator
    torch.manual_seed(seed)
    G = make_generator(**_kw(recipe))
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith(('.bias', '.beta', '.gamma', '.kernel', '.class_matrix')):
                p.add_(0.05 * torch.randn_like(p))
    return G.to(device)


def _inputs(recipe, batch, device, seed):
    kw = _kw(recipe)
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    z = torch.randn(batch, 128, generator=g, dtype=torch.float64)
    cls = torch.randint(0, kw['number_of_classes'], (batch, 1), generator=g, dtype=torch.int32)
    H, W, _ = kw['first_block_shape']
    s = 2 ** len(kw['block_sizes'])
    w = torch.randn(batch, H * s, W * s, 3, generator=g, dtype=torch.float64)
    return z.float().to(device), (cls.to(device) if kw['gan_type'] is not None else None), w.to(device)


def _site_kw(G):
    """the layers' own ddof (functional.whiten_color is called with 1), epsilon and momentum"""
    n = G.final_norm.npart
    return dict(ddof=1, epsilon=n.epsilon, momentum=n.momentum)


def _sites(G):
    """(state-dict prefix, module) of every ReLU'd norm in the order the network applies them"""
    out = []
    for i, blk in enumerate(G.blocks):
        out += [(f'blocks.{i}.bn1', blk.bn1), (f'blocks.{i}.bn2', blk.bn2)]
    return out + [('final_norm', G.final_norm)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the route decisions of a pass, on the host from the library's predicates (shapes only: no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def _routes(G, recipe, batch, mode='train', groups=1):
    """[(where, {decision: value})] of one pass at this batch: mode 'train' (training mode with autograd), 'eval' (no_grad, moving
    statistics) or 'grouped' (training mode, no_grad, statistic_groups(groups))"""
    from wc_gan_amd import conv as C, functional as WF, ops
    from wc_gan_amd.layers import statistic_groups
    kw = _kw(recipe)
    N, K = batch, kw['number_of_classes']
    train = mode == 'train'
    was = G.training
    G.train(mode != 'eval')
    out = []

    def site(name, norm, shape, consumer, kind, split_in):
        cond = any(br.conditional for br in norm.branches)
        per_sample = cond and K > N // groups
        planes = (consumer is not None and consumer.takes_planes(shape, kind)
                  and WF.conv_handoff_supported(shape, True, 1 if not cond else (N if per_sample else K)))
        d = dict(per_sample=per_sample, planes_out=planes)
        if train:
            d.update(bits=(N * shape[1] * shape[2]) % 32 == 0, bwd_bits=ops.bwd_bits_supported(shape, cond),
                     bwd_planes=split_in and WF.backward_reads_planes(shape, cond))
        out.append((name, d))

    try:
        with statistic_groups(groups):
            H, W, ch = kw['first_block_shape']
            split_in = False
            for i, blk in enumerate(G.blocks):
                name, x = f'blocks.{i}', (N, H, W, ch)
                is_up = blk.resample == 'UP'
                merged = is_up and H * W >= 64                      # upsample + 3x3 as one 4x4 transposed kernel
                hs = (N, 2 * H, 2 * W, blk.conv2.conv.out_channels) if is_up else (N, H, W, blk.conv2.conv.out_channels)
                site(name + '.bn1', blk.bn1, x, blk.conv1 if (merged or not is_up) else None, 'up3' if merged else 'same', split_in)
                w1 = tuple(blk.conv1.conv.weight.shape)
                out.append((name + '.conv1', dict(merged=merged, fast=C.takes_planes(x, w1, 'up3') if merged else
                                                  C.takes_planes((N, hs[1], hs[2], ch), w1, 'same'))))
                out.append((name + '.shortcut', dict(on_planes=split_in, fast=C.takes_planes(x, tuple(blk.shortcut.conv.weight.shape), 'same'))))
                site(name + '.bn2', blk.bn2, hs, blk.conv2, 'same', False)
                out.append((name + '.conv2', dict(fast=C.takes_planes(hs, tuple(blk.conv2.conv.weight.shape), 'same'))))
                readers = (G.blocks[i + 1].bn1, G.blocks[i + 1].shortcut) if i + 1 < len(G.blocks) else (G.final_norm,)
                planes = blk.split_output and all(r.takes_split(hs) for r in readers) and ops.resadd_split_supported(hs)
                x32 = planes and train and not all(r.backward_takes_split(hs) for r in readers if hasattr(r, 'backward_takes_split'))
                sg = max([r.wants_moments(hs) for r in readers if hasattr(r, 'wants_moments')] + [0]) if planes else 0
                out.append((name + '.add', dict(planes=planes, x32=x32, moments=bool(sg) and ops.resadd_stats_supported(hs, is_up, sg))))
                split_in, (_, H, W, ch) = planes, hs
            site('final_norm', G.final_norm, (N, H, W, ch), None, 'same', split_in)
            if train:
                out.append(('final_conv', dict(narrow_wrw=bool(C._lib.load().wc_conv_wrw_narrow_supported(N, H, W, 3, ch, 3)))))
    finally:
        G.train(was)
    return out


def _assert_recipe_routes(G, recipe):
    """the case's batch decides every route as the recipe's generator update does; no >= 128-channel block convolution is turned down"""
    from wc_gan_amd.train import GanTrainer
    sig = inspect.signature(GanTrainer.__init__).parameters
    assert sig['batch_size'].default * sig['generator_batch_multiple'].default == RECIPE_BATCH
    for mode in ('train', 'eval'):
        here, there = _routes(G, recipe, CASES[recipe], mode), _routes(G, recipe, RECIPE_BATCH, mode)
        assert here == there, [(a, b) for a, b in zip(here, there) if a != b]
    for where, d in _routes(G, recipe, CASES[recipe]):
        assert d.get('fast', True), where
    return _routes(G, recipe, CASES[recipe])


# ---------------------------------------------------------------------------------------------------------------------------------
# what the HIP network did
# ---------------------------------------------------------------------------------------------------------------------------------
def _unpack(words, shape):
    """a site's bit mask ([M / 32][C] words, bit b of word (t, c) = row 32 t + b, column c passed the ReLU: _mask_ref of test_fast_gpu.py)
    -> bool NHWC"""
    C = shape[-1]
    bits = (words.view(-1, 1, C) >> torch.arange(32, device=words.device, dtype=torch.int32).view(1, 32, 1)) & 1
    return bits.view(*shape).bool()


class _Probe:
    """While entered: keeps the shape and, with `signs`, `y > 0` of every ReLU'd site's output (forward hooks); counts the convolutions with
    >= 128 input and output channels that the fast kernel turned down, the residual adds that returned split handles, and factor_mix's calls
    with per-sample indices."""

    def __init__(self, G, signs=False):
        self.G, self.signs = G, signs
        self.shapes, self.masks, self.missed, self.split, self.mixed = [], [], [], [], []

    def _hook(self, _mod, _inp, out):
        from wc_gan_amd import functional as WF
        self.shapes.append(tuple(out.shape))
        if self.signs:
            self.masks.append(WF.materialize(out).detach() > 0)         # (the planes of a handle hang on `out` itself, not on a detached view)

    def __enter__(self):
        from wc_gan_amd import conv as C, functional as WF, generator as gen
        self.mods = (C, WF, gen)
        self.orig = (C.fast_conv_or_none, WF.factor_mix, gen.residual_add)
        conv0, mix0, add0 = self.orig

        def conv(x, w, *a, **k):
            y = conv0(x, w, *a, **k)
            if y is None and x.shape[-1] >= 128 and w.shape[0] >= 128:
                self.missed.append((tuple(x.shape), tuple(w.shape)))
            return y

        def mix(dictionary, alpha, idx=None, base=None):
            self.mixed.append(idx is not None)
            return mix0(dictionary, alpha, idx, base)

        def add(*a, **k):
            out = add0(*a, **k)
            self.split.append(WF.split_of(out) is not None)
            return out
        C.fast_conv_or_none, WF.factor_mix, gen.residual_add = conv, mix, add
        self.handles = [m.register_forward_hook(self._hook) for _, m in _sites(self.G)]
        return self

    def __exit__(self, *exc):
        C, WF, gen = self.mods
        C.fast_conv_or_none, WF.factor_mix, gen.residual_add = self.orig
        for h in self.handles:
            h.remove()


def _moving(G):
    return {prefix: (m.npart.moving_mean.detach().clone(), m.npart.moving_cov.detach().clone()) for prefix, m in _sites(G)}


def _check_masks(masks, ref, label):
    """the conditions on the forced signs, per site"""
    per_site = R.site_disagreement(masks, ref.pre)
    band, share = max(b for b, _ in per_site), max(s for _, s in per_site)
    print(f"  {label}: relu masks differ from the float64 signs in at most {share:.1e} of a site, the farthest at {band:.1e} of its tensor's maximum")
    for prefix, (b, s) in zip(ref.sites, per_site):
        assert b <= MASK_BAND and s <= MASK_SHARE, (label, prefix, b, s)
    return band, share


def _hip_call(G, recipe, z, cls, w=None, mode='train', groups=1):
    """One pass of the module -> (state before it, masks, image, gradients | None, moving statistics | None); asserts the routes."""
    import wc_gan_amd.functional as WF
    from wc_gan_amd.layers import statistic_groups
    kw = _kw(recipe)
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    G.train(mode != 'eval')
    for p in G.parameters():
        p.grad = None
    probe = _Probe(G, signs=mode != 'train')
    rec = []
    with probe:
        if mode == 'train':
            WF.MASK_TAP = {'record': rec}
            try:
                img = G(z, cls)
            finally:
                WF.MASK_TAP = None
            (img * w.float()).sum().backward()
        else:
            with torch.no_grad(), statistic_groups(groups):
                img = G(z, cls)
    n_relu = R.relu_count(kw['block_sizes'])
    assert len(probe.shapes) == n_relu
    masks = [_unpack(m, s) for m, s in zip(rec, probe.shapes)] if mode == 'train' else probe.masks
    assert len(masks) == n_relu, (len(masks), n_relu)          # one mask per ReLU'd site: 7 for three blocks, 9 for four
    assert probe.missed == [], probe.missed
    want = [d['planes'] for where, d in _routes(G, recipe, z.shape[0], mode, groups) if where.endswith('.add')]
    assert probe.split == want, (probe.split, want)
    if mode == 'train':
        assert probe.split == [d['planes'] for where, d in _routes(G, recipe, RECIPE_BATCH) if where.endswith('.add')]
    if kw['block_after_norm'] == 'ufconv' and kw['number_of_classes'] > z.shape[0] // groups:
        assert probe.mixed == [True] * (2 * len(G.blocks)), probe.mixed          # per-sample tables through factor_mix at every block site
    grads = {n: p.grad for n, p in G.named_parameters() if p.grad is not None} if mode == 'train' else None
    return state, masks, img.detach(), grads, (_moving(G) if mode != 'eval' else None)


def _compare(G, recipe, z, cls, w, mode, groups, label, fp32=False):
    """-> ({kind: error} of the HIP route, the same of the fp32 restatement | None)"""
    state, masks, img, grads, moving = _hip_call(G, recipe, z, cls, w, mode, groups)
    kw = dict(_kw(recipe), **_site_kw(G))
    wr = w if mode == 'train' else None
    torch.cuda.synchronize(); t0 = time.time()
    ref, ref_img, ref_grads = R.run(state, kw, z, cls, wr, masks, training=mode != 'eval', groups=groups)
    torch.cuda.synchronize(); REFERENCE_SECONDS[label] = time.time() - t0
    _check_masks(masks, ref, label)
    if grads is not None:
        assert set(grads) == set(n for n, _ in G.named_parameters())
    errs = R.errors(img, grads, moving, ref, ref_img, ref_grads)
    errs32 = None
    if fp32:
        r32, img32, grads32 = R.run(state, kw, z, cls, wr, masks, training=mode != 'eval', groups=groups, dtype=torch.float32)
        errs32 = R.errors(img32, grads32, r32.moving if moving is not None else None, ref, ref_img, ref_grads)
    return errs, errs32


def _case(recipe, fp32=False, grouped=False):
    """-> [(label, hip errors, fp32 errors | None)] of the calls of one case, on one module"""
    G = _module(recipe, 'cuda')
    batch = CASES[recipe]
    _assert_recipe_routes(G, recipe)
    rows = []
    if grouped:
        z, cls, w = _inputs(recipe, 2 * batch, 'cuda', 30)
        rows.append((f"{recipe} grouped(2) x {batch}",) + _compare(G, recipe, z, cls, None, 'grouped', 2, f"{recipe} grouped", fp32))
        return rows
    for call in (1, 2):
        z, cls, w = _inputs(recipe, batch, 'cuda', 20 + call)
        rows.append((f"{recipe} train call {call}",) + _compare(G, recipe, z, cls, w, 'train', 1, f"{recipe} train call {call}", fp32))
    z, cls, w = _inputs(recipe, batch, 'cuda', 23)
    rows.append((f"{recipe} eval",) + _compare(G, recipe, z, cls, None, 'eval', 1, f"{recipe} eval", fp32))
    return rows


def _check(rows):
    bad = []
    for label, errs, _ in rows:
        print(label, {k: f"{v:.2e}" for k, v in errs.items()})
        bad += [(label, k, v, BOUNDS[k]) for k, v in errs.items() if not v < BOUNDS[k]]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", list(CASES))
def test_recipe_generator_in_two_training_calls_and_one_eval_call(recipe):
    """image, every parameter gradient and the moving statistics of two successive training calls, then the evaluation-mode image through
    the cached plan: each against the float64 reference built from the state the module had before that call"""
    _check(_case(recipe))


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", GROUPED)
def test_recipe_generator_with_two_statistic_groups(recipe):
    """forward only, statistic_groups(2) at twice the batch: image and moving statistics against the reference with groups=2"""
    _check(_case(recipe, grouped=True))


if __name__ == '__main__':
    print(f"batches: {CASES}; grouped: {GROUPED} at twice the batch in two statistic groups", flush=True)
    print("ref s: the float64 reference of that call alone, forward and backward (training calls) or forward", flush=True)
    print(f"{'generator':<44}{'route':<12}" + ''.join(f"{k:>10}" for k in R.KINDS) + f"{'ref s':>8}", flush=True)
    worst = {route: dict.fromkeys(R.KINDS, 0.0) for route in ('hip', 'torch fp32')}
    for recipe, grouped in [(r, False) for r in CASES] + [(r, True) for r in GROUPED]:
        rows = _case(recipe, fp32=True, grouped=grouped)
        for label, errs, errs32 in rows:
            dt = [v for k, v in REFERENCE_SECONDS.items() if label.startswith(k)][0]
            for route, e in (('hip', errs), ('torch fp32', errs32)):
                print(f"{label:<44}{route:<12}" + ''.join(f"{e[k]:>10.2e}" for k in R.KINDS) + f"{dt:>8.2f}", flush=True)
                for k in R.KINDS:
                    worst[route][k] = max(worst[route][k], e[k])
    for route in worst:
        print(f"{'worst over all cases and calls':<44}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in R.KINDS), flush=True)
    print(f"{'bound: 4 x torch fp32, one digit up, <= 1e-4':<56}" + ''.join(f"{BOUNDS[k]:>10.0e}" for k in R.KINDS), flush=True)
