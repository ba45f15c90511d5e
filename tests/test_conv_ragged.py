"""CPU tests of the partial last tile's host side (csrc/wc_conv.hip wc_conv_ragged_supported and the dispatch behind it, wc_gan_amd/conv.py's
opt-in, train.MNIST_CONFIGS): which geometries the predicates take, what the layer entry answers with the mark off and on, what the k-split
asks for as workspace when tiles are counted as ceil(N*H*W / 128), and the four MNIST recipes' values.  No kernel is launched (the library
loads without a device).  DESIGN.md section 4.21."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


class _W:
    def __init__(self, *shape):
        self.shape = shape


def _geoms(kind, N, H, W, ci, co, k):
    """(forward geometry, data-gradient geometry) of conv.py's layer `kind` on an (N, H, W, ci) input"""
    from wc_gan_amd import conv as C
    w = _W(ci, co, k, k) if kind == 'up' else _W(co, ci, k, k)
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, w)
    return gf, gd


# kind, N, H, W, Cin, Cout, k -> N*H*W of the forward's virtual grid (the output's grid for 'down' / 'down3')
GEOMETRIES = [
    ('same', 2, 8, 8, 128, 128, 3, 128), ('same', 2, 4, 4, 128, 128, 3, 32), ('same', 6, 4, 4, 128, 128, 3, 96),
    ('same', 64, 7, 7, 128, 128, 3, 3136), ('same', 3, 7, 7, 128, 128, 3, 147), ('same', 4, 7, 14, 128, 256, 3, 392),
    ('same', 4, 8, 8, 256, 128, 1, 256), ('same', 10, 4, 4, 128, 128, 1, 160), ('same', 64, 7, 7, 256, 256, 1, 3136),
    ('same', 5, 6, 6, 256, 256, 1, 180),
    ('down', 2, 16, 16, 128, 128, 4, 128), ('down', 32, 14, 14, 64, 128, 4, 1568), ('down', 3, 14, 14, 64, 128, 4, 147),
    ('down3', 8, 16, 16, 128, 128, 3, 512), ('down3', 32, 14, 14, 128, 128, 3, 1568), ('down3', 8, 14, 14, 128, 128, 3, 392),
    ('up', 2, 8, 8, 128, 128, 4, 128), ('up', 64, 7, 7, 128, 128, 4, 3136), ('up', 8, 6, 6, 256, 256, 4, 288), ('up', 3, 7, 7, 128, 128, 4, 147),
    ('up3', 8, 8, 8, 128, 128, 3, 512), ('up3', 64, 7, 7, 256, 256, 3, 3136), ('up3', 16, 6, 6, 256, 256, 3, 576), ('up3', 8, 7, 7, 256, 256, 3, 392),
]


@pytest.mark.parametrize("row", GEOMETRIES, ids=lambda r: '-'.join(str(v) for v in r[:7]))
def test_predicates(lib, row):
    """wc_conv_supported keeps its value (whole tiles); wc_conv_ragged_supported is 1 exactly for N*H*W % 32 == 0, for the forward and the
    data-gradient geometry alike (they share their virtual grid's size in every kind)"""
    kind, N, H, W, ci, co, k, M = row
    gf, gd = _geoms(kind, N, H, W, ci, co, k)
    for g in (gf, gd):
        assert g.N * g.H * g.W == M
        assert lib.wc_conv_supported(ctypes.addressof(g)) == (1 if M % 128 == 0 else 0)
        assert lib.wc_conv_ragged_supported(ctypes.addressof(g)) == (1 if M % 32 == 0 else 0)


def test_the_other_rules_are_unchanged(lib):
    assert lib.wc_conv_ragged_supported(None) == 0
    gf, _ = _geoms('same', 3, 7, 7, 128, 128, 3)                     # 147 points: no multiple of 32
    assert lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 0
    for field, bad in (('Cin', 48), ('Cout', 96), ('ntaps', 17), ('nphase', 5), ('W', 1)):
        gf, _ = _geoms('same', 2, 4, 4, 128, 128, 3)
        assert lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 1
        setattr(gf, field, bad)
        assert lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 0 and lib.wc_conv_supported(ctypes.addressof(gf)) == 0, field
    # the rows past the grid must stay below 2^31 (the multiply-shift division): N*H*W <= 2^31 - 128 on a partial last tile
    gf, _ = _geoms('same', 2, 4, 4, 128, 128, 3)
    gf.N, gf.H, gf.W, gf.Hin, gf.Win = 2 ** 17 - 1, 128, 128, 128, 128           # 2^31 - 2^14 points: whole tiles
    assert lib.wc_conv_supported(ctypes.addressof(gf)) == 1 and lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 1
    gf.N, gf.H, gf.W, gf.Hin, gf.Win = 2 ** 16 - 1, 128, 256, 128, 256
    assert lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 1
    gf.N, gf.H, gf.W, gf.Hin, gf.Win = 2 ** 26 - 1, 4, 8, 4, 8                   # 2^31 - 32 points
    assert lib.wc_conv_supported(ctypes.addressof(gf)) == 0 and lib.wc_conv_ragged_supported(ctypes.addressof(gf)) == 0


class _T:
    """a tensor as conv.supported sees it, without a device"""
    is_cuda, dtype = True, None

    def __init__(self, *shape):
        import torch
        self.shape, self.dtype = tuple(shape), torch.float32

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


LAYERS = [('same', (64, 7, 7, 128), (128, 128, 3, 3)), ('up3', (64, 7, 7, 128), (128, 128, 3, 3)), ('down3', (64, 14, 14, 128), (128, 128, 3, 3))]


@pytest.mark.parametrize("kind,shape,wshape", LAYERS, ids=[r[0] for r in LAYERS])
def test_the_layer_entry_takes_a_partial_tile_only_for_a_marked_layer(lib, kind, shape, wshape):
    from wc_gan_amd import conv as C
    x, w = _T(*shape), _T(*wshape)
    assert C.supported(x, w, kind) is False and C.supported(x, w, kind, ragged=True) is True
    assert C.takes_planes(shape, wshape, kind) is False and C.takes_planes(shape, wshape, kind, ragged=True) is True
    assert C.supported(x, w, kind) is False                         # (the plan cache keeps the two answers apart)
    p_off, p_on = C._plan(kind, x, w), C._plan(kind, x, w, True)
    assert p_off is not p_on and not p_off.ok and p_on.ok and p_on.wrw_ws > 0

    class Site:
        ragged_conv = True
    assert C._ragged(Site()) is True and C._ragged(object()) is False and C._ragged(None) is False


def test_an_aligned_layer_answers_the_same_either_way(lib):
    from wc_gan_amd import conv as C
    x, w = _T(128, 8, 8, 128), _T(128, 128, 3, 3)
    p_off, p_on = C._plan('same', x, w), C._plan('same', x, w, True)
    for f in ('ok', 'fwd_ws', 'bwd_ws', 'wrw_ws', 'pair', 'res', 'tail', 'bwd_tail'):
        assert getattr(p_off, f) == getattr(p_on, f), f
    assert C.supported(_T(3, 7, 7, 128), w, 'same', ragged=True) is False          # 147 points: the torch fallback stays


# kind, N, H, W, Cin, Cout, k, (forward k, data-gradient k), N*H*W % 128: the parity rows of tests/test_conv_ragged_gpu.py.
# k by the dispatch rule with tiles = ceil(N*H*W / 128): wgs = tiles * nphase * Cout / (256 | 128 | 64); k = 1 when wgs > 96 or
# iters = ntaps * Cin / 32 < 8, else min(ceil(256 / wgs), iters / 4, 8)
WORKSPACE = [
    ('same', 2, 4, 4, 128, 128, 3, (8, 8), 32),          # 1 tile, iters 36
    ('same', 6, 4, 4, 128, 128, 3, (8, 8), 96),
    ('same', 10, 4, 4, 128, 128, 1, (1, 1), 32),         # iters 4: no k-split
    ('same', 32, 7, 7, 128, 256, 3, (8, 8), 32),         # 13 tiles; the data gradient 128 wide: 13 workgroups too
    ('up3', 64, 7, 7, 256, 256, 3, (1, 8), 64),          # 25 tiles x 4 phases = 100 workgroups > 96; the dense data gradient: 25
    ('up3', 64, 7, 7, 128, 128, 3, (1, 8), 64),
    ('down3', 32, 14, 14, 128, 128, 3, (8, 4), 32),      # data gradient: 13 x 4 = 52 workgroups -> 5, iters 16 -> 4
    ('down', 32, 14, 14, 64, 128, 4, (8, 4), 32),
    ('same', 32, 7, 7, 128, 128, 3, (8, 8), 32),
    ('same', 3, 8, 8, 1024, 1024, 3, (8, 8), 64),        # 2 tiles x 4 = 8 workgroups
]


@pytest.mark.parametrize("row", WORKSPACE, ids=lambda r: '-'.join(str(v) for v in r[:7]))
def test_workspace_counts_tiles_as_ceil(lib, row):
    kind, N, H, W, ci, co, k, (kf, kd), over = row
    gf, gd = _geoms(kind, N, H, W, ci, co, k)
    for g, want in ((gf, kf), (gd, kd)):
        assert (g.N * g.H * g.W) % 128 == over
        n = g.N * g.Hout * g.Wout * g.Cout * 4
        assert lib.wc_conv_workspace_bytes(ctypes.addressof(g)) == (want * n if want > 1 else 0)


def test_the_weight_gradient_covers_the_chunks_exactly(lib):
    """(3, 8, 8) at 1024 -> 1024: 192 points = 6 chunks of 32, the splits clamped to 6 (not to 192 / 128 tiles)"""
    gf, _ = _geoms('same', 3, 8, 8, 1024, 1024, 3)
    assert lib.wc_conv_wrw_workspace_bytes(ctypes.addressof(gf)) == 6 * 9 * 1024 * 1024 * 4
    gf, _ = _geoms('same', 2, 4, 4, 128, 128, 3)                     # one chunk
    assert lib.wc_conv_wrw_workspace_bytes(ctypes.addressof(gf)) == 1 * 9 * 128 * 128 * 4


def test_pair_res_and_tail_answer_under_their_own_rules(lib):
    gf, gd = _geoms('same', 32, 7, 7, 128, 128, 3)
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)
    assert lib.wc_conv_bwd_pair_supported(pd, pf) == 1 and lib.wc_conv_res_supported(pf) == 1 and lib.wc_conv_tail_supported(pf) == 1
    gf, gd = _geoms('up3', 64, 7, 7, 128, 128, 3)                   # an up-sampling layer; a forward without a k-split
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)
    assert lib.wc_conv_bwd_pair_supported(pd, pf) == 0 and lib.wc_conv_res_supported(pf) == 0 and lib.wc_conv_tail_supported(pd) == 1
    gf, gd = _geoms('same', 3, 7, 7, 128, 128, 3)                   # 147 points
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)
    assert lib.wc_conv_bwd_pair_supported(pd, pf) == 0 and lib.wc_conv_res_supported(pf) == 0 and lib.wc_conv_tail_supported(pf) == 0
    from wc_gan_amd import conv as C
    p = C._plan('same', _T(32, 7, 7, 128), _T(128, 128, 3, 3), True)
    assert p.ok and p.pair and p.res and p.tail and p.bwd_tail
    p = C._plan('same', _T(32, 7, 7, 128), _T(128, 128, 3, 3))
    assert not (p.ok or p.pair or p.res or p.tail or p.bwd_tail)


def test_small_rows_have_a_fifth_of_their_elements_in_the_last_tile():
    """the GPU file's condition on its shape table: where N*H*W < 512, at least 15 % of y's and dx's rows are the partial tile's"""
    small = [r for r in WORKSPACE if r[1] * r[2] * r[3] * (1 if r[0] in ('same', 'up3') else 0.25) < 512]
    assert len(small) == 4
    for kind, N, H, W, *_ in small:
        M = N * H * W
        assert M % 128 and (M % 128) / M >= 0.15, (kind, N, H, W)


NAMES = ('mnist_uncond', 'mnist_cond', 'fashionmnist_uncond', 'fashionmnist_cond')


def test_mnist_configs():
    from wc_gan_amd import train as T
    assert tuple(T.MNIST_CONFIGS) == NAMES and tuple(T.MNIST_SCHEDULES) == NAMES
    assert not set(NAMES) & set(T.CONFIGS)
    want = {'mnist_uncond': (256, 'uconv', None, 5, None), 'mnist_cond': (128, 'ucconv', 'PROJECTIVE', 5, None),
            'fashionmnist_uncond': (256, 'uconv', None, 20, 'linear'), 'fashionmnist_cond': (128, 'ucconv', 'PROJECTIVE', 20, 'linear')}
    for name in NAMES:
        F, after, gan_type, epochs, schedule = want[name]
        c = T.MNIST_CONFIGS[name]
        g, d = c['generator'], c['discriminator']
        assert g['output_channels'] == 1 and g['first_block_shape'] == (7, 7, F)
        assert g['block_sizes'] == (F, F) and g['resamples'] == ("UP", "UP")
        assert g['block_norm'] == 'd' and g['block_after_norm'] == after and g['last_norm'] == 'd' and g['last_after_norm'] == 'uconv'
        assert g['gan_type'] == gan_type and g['number_of_classes'] == 10
        assert d['input_image_shape'] == (28, 28, 1) and d['block_sizes'] == (128, 128, 128, 128)
        assert d['resamples'] == ('DOWN', 'DOWN', 'SAME', 'SAME') and d['spectral'] is True and d['sum_pool'] is True
        assert d['type'] == gan_type and d['number_of_classes'] == 10 and not d.get('fused_projection', False)
        assert c['image_shape'] == (28, 28, 1) and c['conditional'] is (gan_type is not None)
        assert g['ragged_conv'] is T.MNIST_RAGGED_SHIPS and d['ragged_conv'] is T.MNIST_RAGGED_SHIPS
        assert T.MNIST_SCHEDULES[name] == dict(lr_decay_schedule=schedule, number_of_epochs=epochs)


def test_the_shipped_mark_follows_from_the_measured_step():
    """the rule set before measuring: ragged_conv=True ships only if that leg is faster in every round on both recipes (tools/mnist_step.py)"""
    import json
    from wc_gan_amd import train as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'profiles', 'mnist_step.json')) as f:
        prof = json.load(f)
    assert prof['rounds'] == 7 and prof['batch'] == 64 and sorted(prof['configs']) == ['mnist_cond', 'mnist_uncond']
    faster = True
    for c in prof['configs'].values():
        on, off = c['ragged']['ms'], c['off']['ms']
        assert len(on) == len(off) == 7
        faster = faster and all(a < b for a, b in zip(on, off))
    assert T.MNIST_RAGGED_SHIPS is faster


def test_ragged_config_marks_both_networks_of_a_copy():
    from wc_gan_amd import train as T
    for table in (T.MNIST_CONFIGS, T.CONFIGS):
        for name, c in table.items():
            before = (c['generator'].get('ragged_conv', False), c['discriminator'].get('ragged_conv', False))
            on, off = T.ragged_config(c), T.ragged_config(c, on=False)
            assert on['generator']['ragged_conv'] is True and on['discriminator']['ragged_conv'] is True
            assert off['generator']['ragged_conv'] is False and off['discriminator']['ragged_conv'] is False
            assert (c['generator'].get('ragged_conv', False), c['discriminator'].get('ragged_conv', False)) == before
            assert {k: v for k, v in on['generator'].items() if k != 'ragged_conv'} == {k: v for k, v in c['generator'].items() if k != 'ragged_conv'}


@pytest.mark.parametrize("name", ['mnist_uncond', 'mnist_cond'])
def test_the_networks_build_on_the_cpu_and_carry_the_mark(name):
    from wc_gan_amd import train as T
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.generator import Conv2D, make_generator
    for on in (False, True):
        c = T.ragged_config(T.MNIST_CONFIGS[name], on=on)
        G, D = make_generator(**c['generator']), make_discriminator(**c['discriminator'])
        convs = [m for net in (G, D) for m in net.modules() if isinstance(m, Conv2D)]
        assert len(convs) == 2 * 3 + 1 + 3 + 3 + 2 + 2          # generator: two blocks and the last layer; critic: blocks 0-3
        assert all(m.ragged_conv is on for m in convs)
        assert G.final_conv.conv.out_channels == 1 and D.blocks[0].conv1.conv.in_channels == 1
        assert len(G.blocks) == 2 and G.first_block_shape == (7, 7, c['generator']['first_block_shape'][2])
    cifar = T.CIFAR10_COND                                     # a recipe that does not name the keyword: the mark is off
    assert make_generator(**cifar['generator']).blocks[0].conv1.ragged_conv is False
    assert make_discriminator(**cifar['discriminator']).blocks[1].conv1.ragged_conv is False


def test_wc_sites_of_the_unconditional_recipe():
    from wc_gan_amd import train as T
    sites = T.wc_sites(T.MNIST_CONFIGS['mnist_uncond'], 64)
    assert [(s[1], s[2], s[3], s[4]) for s in sites] == [(64, 7, 7, 256), (64, 14, 14, 256), (64, 14, 14, 256), (64, 28, 28, 256), (64, 28, 28, 256)]


def test_the_one_channel_layers_are_the_narrow_kernels(lib):
    """the critic's 1 -> 128 convolutions (k*k*Cin = 9 and 1 < 32) and the generator's F -> 1 last layer's weight gradient"""
    for n in (8, 64):
        assert lib.wc_conv_narrow64_supported(n, 28, 28, 1, 128, 3) == 1 and lib.wc_conv_narrow64_supported(n, 28, 28, 1, 128, 1) == 1
        assert lib.wc_conv_wrw_narrow_supported(n, 28, 28, 1, 256, 3) == 1 and lib.wc_conv_wrw_narrow_supported(n, 28, 28, 1, 128, 3) == 1
