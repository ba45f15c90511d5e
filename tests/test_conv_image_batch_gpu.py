"""A pass's weight images in one launch (csrc/wc_conv.hip: conv_weights_batch_kernel behind wc_conv_weights_batch_f32, conv_absmax_batch_kernel
behind wc_conv_absmax_batch_f32; conv.prepare_images and the layers' pick-up) against the per-layer entries wc_conv_weights_f32 /
wc_conv_weights_pair_f32.  Every comparison in this file is torch.equal: each job's workgroups run conv_weights_body on the arguments the
per-layer entry would pass, the body's result does not depend on how its groups map to workgroups, and the scale comes from the same
partials or from a maximum, which has no order.  Image and scale buffers are pattern-filled and guard-banded (tests/_poison.py)."""
import collections
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _poison import Poison

KINDS = {                     # name: (conv kind, kernel size); grids of the smallest legal size, N * H * W = 128 (the images do not depend on it)
    'same3': ('same', 3), 'same1': ('same', 1), 'down3': ('down3', 3), 'up3': ('up3', 3), 'down4': ('down', 4), 'up4': ('up', 4),
}
CHANNELS = ((32, 64), (128, 128), (64, 192), (256, 256))
N, H, W = 2, 8, 8


def _lib():
    from wc_gan_amd import _lib as L
    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _weight(name, ci, co, channels_last, seed=0):
    kind, k = KINDS[name]
    g = torch.Generator().manual_seed(1000 * ci + co + seed)
    shape = (ci, co, 4, 4) if kind == 'up' else (co, ci, k, k)
    w = (torch.randn(*shape, generator=g) / (ci * k * k) ** 0.5).cuda()
    return w.contiguous(memory_format=torch.channels_last) if channels_last else w.contiguous()


def _geoms(name, w):
    """((forward geometry, k_axis, n_axis), (data-gradient geometry, k_axis, n_axis)) of the kind on the smallest grid"""
    from wc_gan_amd import conv as C
    kind, _ = KINDS[name]
    if kind in ('down', 'down3'):
        return C._geoms(kind, N, 2 * H, 2 * W, w)
    return C._geoms(kind, N, H, W, w)


def _known(w):
    """a view of w that carries `_wc_amax` as the spectral-norm op leaves it: floats whose maximum is max|w|, the unused ones zero"""
    v = w.view_as(w)
    assert v.data_ptr() == w.data_ptr() and v.stride() == w.stride()
    parts = torch.zeros(37, device='cuda')
    chunks = w.detach().abs().flatten().sort().values.chunk(29)
    parts[:len(chunks)] = torch.stack([c.max() for c in chunks])
    v._wc_amax = parts
    return v


def _measure(ws):
    """wc_conv_absmax_batch_f32 on a list of weights -> [len(ws), 512] partial maxima"""
    L = _lib()
    lib = L.load()
    parts = torch.empty(len(ws), L.ABSMAX_FLOATS, device='cuda')
    jobs = (L.ConvAbsmaxJob * len(ws))()
    for i, w in enumerate(ws):
        jobs[i].x, jobs[i].n, jobs[i].partial = w.data_ptr(), w.numel(), parts[i].data_ptr()
    L.check(lib.wc_conv_absmax_batch_f32(ctypes.addressof(jobs), len(ws), _stream()), "wc_conv_absmax_batch_f32")
    return parts


def _fill_jobs(specs, images, scales):
    L = _lib()
    jobs = (L.ConvWeightsJob * len(specs))()
    for j, (w, (g, ka, na), amax, pair_of) in enumerate(specs):
        job = jobs[j]
        job.w, job.n_elems, job.g = w.data_ptr(), w.numel(), ctypes.addressof(g)
        job.stride_k, job.stride_n, job.stride_r, job.stride_s = w.stride(ka), w.stride(na), w.stride(2), w.stride(3)
        job.image = images[j].data_ptr() if images is not None else 16
        job.scale = scales.data_ptr() + 4 * j if scales is not None else 16
        job.amax, job.amax_count, job.pair_of = (None, 0, pair_of) if amax is None else (amax.data_ptr(), amax.numel(), pair_of)
    return jobs


def _batch(specs):
    """specs: [(weight, (geometry, k_axis, n_axis), amax tensor | None, pair_of)] through wc_conv_weights_batch_f32 itself
    -> (images, scales, launches); call inside a Poison context"""
    L = _lib()
    lib = L.load()
    images = [torch.empty(lib.wc_conv_weights_bytes(ctypes.addressof(s[1][0])), dtype=torch.uint8, device='cuda') for s in specs]
    scales = torch.empty(len(specs), dtype=torch.float32, device='cuda')
    jobs = _fill_jobs(specs, images, scales)
    launches = lib.wc_conv_weights_batch_launches(ctypes.addressof(jobs), len(specs))
    L.check(lib.wc_conv_weights_batch_f32(ctypes.addressof(jobs), len(specs), _stream()), "wc_conv_weights_batch_f32")
    return images, scales, launches


_refs = {}


def _reference(name, channels_last):
    """per (Cin, Cout): the weight, its geometries and the per-layer entries' images: measured (pair and single entry) and known maximum.
    Built once, shared, never written to."""
    key = (name, channels_last)
    if key in _refs:
        return _refs[key]
    from wc_gan_amd import conv as C
    out = []
    for ci, co in CHANNELS:
        w = _weight(name, ci, co, channels_last)
        fwd, bwd = _geoms(name, w)
        wk = _known(w)
        single = C.weight_image(w, *fwd)              # (takes its maximum inside where the weight is small, else sweeps: scale[1:] holds the sweep's partials)
        out.append(dict(w=w, wk=wk, fwd=fwd, bwd=bwd, pair=C.weight_image_pair(w, fwd, bwd), pair_known=C.weight_image_pair(wk, fwd, bwd),
                        single=single, inline=w.numel() <= 32768))
    torch.cuda.synchronize()
    _refs[key] = out
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("channels_last", [True, False], ids=['channels-last', 'contiguous'])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_batch_entry_has_the_bytes_of_the_per_layer_entries(name, channels_last):
    """every kind x every channel pair, each weight as a pair of jobs with its maximum known, measured (wc_conv_absmax_batch_f32) and --
    where the per-layer entry would take it inside -- taken inside the job; under two fill patterns, so that a byte the kernel left alone
    shows; guard bands intact"""
    refs = _reference(name, channels_last)
    sweep = _measure([r['w'] for r in refs])
    for r, parts in zip(refs, sweep):
        if not r['inline']:        # the per-layer single entry swept this weight: the batched sweep leaves the same partials
            assert torch.equal(parts, r['single'][1][1:1 + 512]), (name, tuple(r['w'].shape))
    inline_seen = False
    for pattern in (0x00, 0xFF):
        with Poison(pattern) as P:
            specs, want = [], []
            for r, parts in zip(refs, sweep):
                sources = [('known', r['wk'], r['wk']._wc_amax, r['pair_known']), ('measured', r['w'], parts, r['pair'])]
                if r['inline']:
                    sources.append(('inline', r['w'], None, r['pair']))
                    inline_seen = True
                for what, w, amax, ref in sources:
                    j = len(specs)
                    specs += [(w, r['fwd'], amax, -1), (w, r['bwd'], amax, j)]
                    want += [(ref[0], what), (ref[1], what)]
            images, scales, launches = _batch(specs)
            P.check_guards()
            assert launches >= (len(specs) + 15) // 16
            for j, ((ref_img, ref_scale), what) in enumerate(want):
                assert _same(images[j], ref_img), (name, what, j, hex(pattern))
                assert _same(scales[j:j + 1], ref_scale.reshape(1)[:1]), (name, what, j, hex(pattern))
            # the single entry's image (its own choice of the maximum's source) is the pair's forward image
            for r in refs:
                assert _same(r['single'][0], r['pair'][0][0]) and _same(r['single'][1][:1], r['pair'][0][1])
            P.release()
    assert inline_seen == any(r['inline'] for r in refs)


@pytest.mark.gpu
def test_the_inline_maximum_of_the_128_wide_shortcut():
    """128 x 128 x 1 x 1 (16384 floats): wc_conv_weights_f32 takes the maximum inside its one launch, and so does the job"""
    refs = _reference('same1', True)
    r = [r for r in refs if tuple(r['w'].shape) == (128, 128, 1, 1)][0]
    assert r['inline']
    with Poison(0xFF) as P:
        images, scales, launches = _batch([(r['w'], r['fwd'], None, -1)])
        P.check_guards()
        assert launches == 1 and _same(images[0], r['single'][0]) and _same(scales[:1], r['single'][1][:1])
        P.release()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 17])
def test_list_lengths(count):
    """1, 2 and one more than a launch's 16 jobs: the last really takes two launches; a list of eight kinds of geometry takes two as well
    (six tap-source tables per launch)"""
    refs = _reference('same3', True)
    r = refs[1]
    specs = [(r['w'], r['fwd'] if j % 2 == 0 else r['bwd'], r['wk']._wc_amax, -1) for j in range(count)]
    with Poison(0x7B) as P:
        images, scales, launches = _batch(specs)
        P.check_guards()
        assert launches == (2 if count > 16 else 1)
        for j in range(count):
            ref = r['pair_known'][j % 2]
            assert _same(images[j], ref[0]) and _same(scales[j:j + 1], ref[1].reshape(1)), j
        P.release()
    if count == 17:
        specs, want = [], []
        for name in sorted(KINDS):
            q = _reference(name, True)[1]
            specs += [(q['w'], q['fwd'], None if q['inline'] else _measure([q['w']])[0], -1), (q['wk'], q['bwd'], q['wk']._wc_amax, -1)]
            want += [q['pair'][0], q['pair_known'][1]]
        with Poison(0xFF) as P:
            images, scales, launches = _batch(specs)
            P.check_guards()
            assert len(specs) == 12 and launches == 2
            for j, ref in enumerate(want):
                assert _same(images[j], ref[0]) and _same(scales[j:j + 1], ref[1].reshape(1)), j
            P.release()


@pytest.mark.gpu
def test_argument_checks_return_codes_without_a_launch():
    L = _lib()
    lib = L.load()
    r = _reference('same3', True)[3]          # 256 x 256 x 3 x 3: too large for the maximum inside the job
    up = _reference('up3', True)[3]
    parts = r['wk']._wc_amax
    ok = [(r['w'], r['fwd'], parts, -1), (r['w'], r['bwd'], parts, 0)]
    img = torch.full((lib.wc_conv_weights_bytes(ctypes.addressof(r['fwd'][0])),), 0x5A, dtype=torch.uint8, device='cuda')
    images, scales = [img, img], torch.full((2,), 7.0, device='cuda')

    def code(specs, imgs=images, count=None):
        jobs = _fill_jobs(specs, imgs, scales)
        n = len(specs) if count is None else count
        rc = lib.wc_conv_weights_batch_f32(ctypes.addressof(jobs), n, _stream())
        assert lib.wc_conv_weights_batch_launches(ctypes.addressof(jobs), n) == rc
        return rc

    assert lib.wc_conv_weights_batch_f32(None, 2, _stream()) == -1 and lib.wc_conv_weights_batch_launches(None, 2) == -1
    assert code(ok, count=0) == -2
    jobs = _fill_jobs(ok, images, scales)
    for field in ('w', 'g', 'image', 'scale'):
        keep = getattr(jobs[1], field)
        setattr(jobs[1], field, None)
        assert lib.wc_conv_weights_batch_f32(ctypes.addressof(jobs), 2, _stream()) == -1, field
        setattr(jobs[1], field, keep)
    assert code([(r['w'], r['fwd'], None, -1)]) == -5                                  # no maximum given, and too large to take it inside
    assert code([(r['w'], r['fwd'], parts, -1), (r['w'], up['bwd'], parts, 0)]) == -5  # a pair whose geometries disagree in bound_mul (1 and 4)
    assert code([(r['w'], r['fwd'], parts, 1), (r['w'], r['bwd'], parts, -1)]) == -5   # the first of a pair comes first
    assert code([(r['w'], r['fwd'], parts, -1), (r['wk'], r['bwd'], parts[:8], 0)]) == -5      # a pair reads one maximum
    aj = (L.ConvAbsmaxJob * 1)()
    aj[0].x, aj[0].n, aj[0].partial = r['w'].data_ptr(), r['w'].numel(), scales.data_ptr()
    assert lib.wc_conv_absmax_batch_f32(None, 1, _stream()) == -1 and lib.wc_conv_absmax_batch_f32(ctypes.addressof(aj), 0, _stream()) == -2
    aj[0].x = r['w'].data_ptr() + 4
    assert lib.wc_conv_absmax_batch_f32(ctypes.addressof(aj), 1, _stream()) == -5
    aj[0].x, aj[0].partial = r['w'].data_ptr(), None
    assert lib.wc_conv_absmax_batch_f32(ctypes.addressof(aj), 1, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((img == 0x5A).all()) and bool((scales == 7.0).all())                   # nothing ran


# ---------------------------------------------------------------------------------------------------------------------------------
# the networks: conv.BATCH_IMAGES on against off, from the same state
# ---------------------------------------------------------------------------------------------------------------------------------
COUNTED = ('wc_conv_weights_f32', 'wc_conv_weights_pair_f32', 'wc_conv_weights_batch_f32', 'wc_conv_absmax_batch_f32')


class _Counting:
    """the library with a call counter around the image entries"""

    def __init__(self, lib):
        self._lib, self.counts = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in COUNTED:
            return fn

        def counted(*a):
            self.counts[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counts(monkeypatch):
    L = _lib()
    proxy = _Counting(L.load())
    monkeypatch.setattr(L, '_lib', proxy)
    return proxy.counts


class _route:
    def __init__(self, batch):
        self.batch = batch

    def __enter__(self):
        from wc_gan_amd import conv as C
        self.old, C.BATCH_IMAGES = C.BATCH_IMAGES, self.batch

    def __exit__(self, *exc):
        from wc_gan_amd import conv as C
        C.BATCH_IMAGES = self.old
        return False


def _critic(seed=5):
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.train import CONFIGS
    torch.manual_seed(seed)
    D = make_discriminator(**CONFIGS['cifar10_uncond']['discriminator'])
    with torch.no_grad():
        for name, p in D.named_parameters():
            if name.endswith('.bias'):
                p.add_(0.05 * torch.randn_like(p))
    return D.cuda().train()


def _images_in(seeds, n=2, hw=32):
    return [(torch.rand((n, hw, hw, 3), generator=torch.Generator().manual_seed(s)) * 2 - 1).cuda() for s in seeds]


def _hinge(D, x):
    out = D(x, None)
    n = x.shape[0] // 2
    return F.relu(1.0 - out[:n]).mean() + F.relu(1.0 + out[n:]).mean()


@pytest.fixture
def deterministic_images():
    """The gradient of the critic's 3-channel input comes from MIOpen's data gradient of the two image-side layers, whose default choice
    adds its partial sums in no fixed order: two calls of ONE route then differ in that tensor.  The comparisons below presume a route
    that repeats itself, so they ask the library for its deterministic kernels."""
    old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = old


def _critic_call(D, x, batch):
    """forward and backward -> every output of the call: loss, the input's gradient, the gradient that leaves the HIP blocks (block 0's
    output), the parameters' gradients, the buffers behind it"""
    kept = []

    def keep(module, inputs, output):
        output.retain_grad()
        kept.append(output)

    hook = D.blocks[0].register_forward_hook(keep)
    try:
        with _route(batch):
            D.zero_grad(set_to_none=True)
            x = x.clone().requires_grad_(True)
            loss = _hinge(D, x)
            loss.backward()
    finally:
        hook.remove()
    out = {'loss': loss.detach().clone(), 'dx': x.grad.clone(), 'd block0': kept[0].grad.clone()}
    out.update({'grad ' + n: p.grad.clone() for n, p in D.named_parameters() if p.grad is not None})
    out.update({'buffer ' + n: b.clone() for n, b in D.named_buffers()})
    return out


def _assert_equal(a, b, label, keys=None):
    if keys is None:
        assert sorted(a) == sorted(b), label
        keys = sorted(a)
    differ = [n for n in keys if not torch.equal(a[n], b[n])]
    assert not differ, (label, differ)


def _delta(counts, before):
    return {k: counts[k] - before[k] for k in COUNTED}


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [False, True], ids=['d-step', 'g-step'])
def test_critic_batches_its_images_and_keeps_every_bit(counts, deterministic_images, frozen):
    """the CIFAR-10 critic at batch 2, three calls on each route from the same state; frozen: the parameters' requires_grad switched off as
    g_step does -- another key, another log.  From the second call on the per-layer entries are not called and the batch entry once."""
    a = _critic()
    if frozen:
        for p in a.parameters():
            p.requires_grad_(False)
    b = copy.deepcopy(a)
    for k, x in enumerate(_images_in((1, 2, 3))):
        before = counts.copy()
        on = _critic_call(a, x, True)
        d = _delta(counts, before)
        print("critic", "g-step" if frozen else "d-step", "call", k, d)
        if k == 0:
            assert d['wc_conv_weights_batch_f32'] == 0 and d['wc_conv_weights_f32'] + d['wc_conv_weights_pair_f32'] == 8
        else:
            assert d == {'wc_conv_weights_f32': 0, 'wc_conv_weights_pair_f32': 0, 'wc_conv_weights_batch_f32': 1, 'wc_conv_absmax_batch_f32': 0}
        before = counts.copy()
        off = _critic_call(b, x, False)
        d = _delta(counts, before)
        assert d['wc_conv_weights_batch_f32'] == 0 and d['wc_conv_weights_f32'] + d['wc_conv_weights_pair_f32'] == 8
        _assert_equal(on, off, f"call {k}")
        assert frozen == (not any(n.startswith('grad ') for n in on))
    assert len(a._wc_image_logs) == 1 and all(m.__dict__.get('_wc_images') is None for m in a.modules())


@pytest.mark.gpu
def test_nothing_is_reused_across_passes_and_a_wrong_log_costs_launches_only(counts, deterministic_images):
    a = _critic()
    b = copy.deepcopy(a)
    x0, x1, x2 = _images_in((1, 2, 3))
    for x in (x0, x1):
        _assert_equal(_critic_call(a, x, True), _critic_call(b, x, False), "before the change")
    # one convolution weight changed in place through .data: no version bump, no optimizer
    for D in (a, b):
        w = D.blocks[2].conv1.conv.weight
        v = w._version
        w.data.mul_(1.5)
        w.data[3, 5] = 0.25
        assert w._version == v
    before = counts.copy()
    on, off = _critic_call(a, x2, True), _critic_call(b, x2, False)
    assert _delta(counts, before)['wc_conv_weights_batch_f32'] == 1
    _assert_equal(on, off, "after the change")
    # a log whose geometries are not this pass's: the log of batch 2 under the key of batch 4 -- every layer builds its own, silently
    from wc_gan_amd import conv as C
    (key2, log2), = a._wc_image_logs.items()
    x4 = _images_in((7,), n=4)[0]
    with torch.enable_grad():
        key4 = C.pass_key(a, x4.clone().requires_grad_(True))
    assert key4 != key2
    a._wc_image_logs[key4] = log2
    before = counts.copy()
    on = _critic_call(a, x4, True)
    d = _delta(counts, before)
    assert d['wc_conv_weights_batch_f32'] == 1 and d['wc_conv_weights_f32'] + d['wc_conv_weights_pair_f32'] == 8, d
    _assert_equal(on, _critic_call(b, x4, False), "wrong log")
    assert key4 not in a._wc_image_logs                          # dropped; the next pass of this key logs it anew, the one after batches
    _assert_equal(_critic_call(a, x4, True), _critic_call(b, x4, False), "logged again")
    before = counts.copy()
    _assert_equal(_critic_call(a, x4, True), _critic_call(b, x4, False), "batched again")
    d = _delta(counts, before)
    assert d['wc_conv_weights_batch_f32'] == 1 and d['wc_conv_weights_f32'] + d['wc_conv_weights_pair_f32'] == 8      # (8: route b's)


@pytest.mark.gpu
def test_a_captured_critic_pass_replays_the_eager_bits(counts, deterministic_images):
    """two eager calls (the second already batched), the third captured and replayed twice, against four eager calls of the per-layer route"""
    a = _critic()
    b = copy.deepcopy(a)
    xs = _images_in((1, 2, 3, 4))
    eager = [_critic_call(b, x, False) for x in xs]
    for k in (0, 1):
        _assert_equal(_critic_call(a, xs[k], True), eager[k], f"eager {k}")
    with _route(True):
        static_x = xs[0].clone().requires_grad_(True)
        a.zero_grad(set_to_none=True)
        before = counts.copy()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = _hinge(a, static_x)
            loss.backward()
        d = _delta(counts, before)
        assert d == {'wc_conv_weights_f32': 0, 'wc_conv_weights_pair_f32': 0, 'wc_conv_weights_batch_f32': 1, 'wc_conv_absmax_batch_f32': 0}
    for k in (2, 3):
        with torch.no_grad():
            static_x.copy_(xs[k])
        graph.replay()
        torch.cuda.synchronize()
        got = {'loss': loss.detach(), 'dx': static_x.grad}
        got.update({'grad ' + n: p.grad for n, p in a.named_parameters()})
        got.update({'buffer ' + n: t for n, t in a.named_buffers()})
        _assert_equal(got, eager[k], f"replay {k}", keys=sorted(got))
        assert sorted(got) == sorted(n for n in eager[k] if n != 'd block0')


@pytest.mark.gpu
def test_a_critic_without_spectral_norm_sweeps_its_weights_in_one_launch(counts, deterministic_images):
    """the WGAN-GP recipe's critic (no spectral norm: nobody leaves max|w| behind): from the second call on one launch for the maxima of
    the 3x3 weights, one for the images -- the 128 x 128 x 1 x 1 shortcut takes its maximum inside its job -- and every bit of the
    per-layer route, whose pair entry sweeps each weight on its own"""
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.train import WGAN_CONFIGS
    torch.manual_seed(9)
    a = make_discriminator(**WGAN_CONFIGS['cifar10_wgan_uncond']['discriminator']).cuda().train()
    b = copy.deepcopy(a)
    for k, x in enumerate(_images_in((1, 2, 3))):
        before = counts.copy()
        on = _critic_call(a, x, True)
        d = _delta(counts, before)
        print("critic without spectral norm, call", k, d)
        if k == 0:
            assert d['wc_conv_weights_batch_f32'] == 0 and d['wc_conv_absmax_batch_f32'] == 0
            assert d['wc_conv_weights_f32'] + d['wc_conv_weights_pair_f32'] == 8
        else:
            assert d == {'wc_conv_weights_f32': 0, 'wc_conv_weights_pair_f32': 0, 'wc_conv_weights_batch_f32': 1, 'wc_conv_absmax_batch_f32': 1}
        _assert_equal(on, _critic_call(b, x, False), f"call {k}")
