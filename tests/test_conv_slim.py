"""CPU tests of the 64- and 32-channel block convolutions' host side (csrc/wc_conv.hip wc_conv_slim_supported and the plans behind it,
wc_gan_amd/conv.py's opt-in, train.IMAGENET_CONFIGS): which geometries the predicates take, that the older predicates keep their values, what
the k-split and the weight gradient ask for as workspace at 32 outputs (no tile count of zero), what the layer entry answers with the mark
off and on, and the ImageNet recipe's values.  No kernel is launched (the library loads without a device).  DESIGN.md section 4.22."""
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
    (gf, _, _), (gd, _, _) = C._geoms(kind, N, H, W, _W(co, ci, k, k))
    return gf, gd


# kind, N, H, W, Cin, Cout, k: the row table of tests/test_conv_slim_gpu.py (which imports it)
ROWS = [
    ('same', 2, 8, 8, 32, 32, 3),            # one 128-point tile
    ('same', 6, 8, 8, 32, 32, 3),            # an odd tile count
    ('same', 8, 6, 8, 32, 32, 3),            # H != W, HW = 48: tiles straddle images
    ('same', 4, 56, 56, 32, 32, 3),          # 98 tiles: past the k-split gate, the direct epilogue
    ('same', 2, 8, 8, 64, 32, 1),            # the shortcut; its data gradient is 32 -> 64
    ('same', 8, 6, 8, 64, 32, 1),
    ('up3', 2, 8, 8, 64, 32, 3),             # conv1 of the 64 -> 32 block; a strided data gradient with Cin = 32, Cout = 64
    ('up3', 8, 6, 8, 64, 32, 3),
    ('same', 2, 8, 8, 32, 64, 3),            # the 32-wide side as the weight gradient's other operand
    ('same', 2, 8, 8, 96, 96, 3),            # % 64 == 32 beyond 32: three tiles of 32 outputs
    ('up3', 2, 8, 8, 128, 64, 3),            # 64-wide layers: the kernels they always had, through the marked entry
    ('same', 2, 8, 8, 64, 64, 3),
    ('same', 2, 8, 8, 128, 64, 1),
]
ROW_ID = lambda r: '-'.join(str(v) for v in r)


def slim_side(row):
    """does the layer have a side that is 32 beyond a multiple of 64?"""
    return row[4] % 64 == 32 or row[5] % 64 == 32


def route_labels(lib):
    """{(pass, 'direct' | 'ksplit')} over the table's geometries with 32 outputs, from wc_conv_workspace_bytes (0 = direct)"""
    seen = set()
    for row in ROWS:
        for name, g in zip(('forward', 'dgrad'), _geoms(*row)):
            if g.Cout == 32:
                seen.add((name, 'ksplit' if lib.wc_conv_workspace_bytes(ctypes.addressof(g)) else 'direct'))
    return seen


@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_predicates(lib, row):
    for g in _geoms(*row):
        p = ctypes.addressof(g)
        assert (g.N * g.H * g.W) % 128 == 0
        assert lib.wc_conv_slim_supported(p) == 1
        # the older predicates: what they always answered -- 0 at an output width that is no multiple of 64, 1 for these whole-tile grids else
        whole = 1 if g.Cout % 64 == 0 else 0
        assert lib.wc_conv_supported(p) == whole and lib.wc_conv_ragged_supported(p) == whole


@pytest.mark.parametrize("row", [r for r in ROWS if slim_side(r)], ids=ROW_ID)
def test_the_fused_routes_stay_off_at_a_32_wide_side(lib, row):
    gf, gd = _geoms(*row)
    pf, pd = ctypes.addressof(gf), ctypes.addressof(gd)
    for p in (pf, pd):
        assert lib.wc_conv_res_supported(p) == 0 and lib.wc_conv_tail_supported(p) == 0
    assert lib.wc_conv_bwd_pair_supported(pd, pf) == 0


def test_what_the_new_predicate_declines(lib):
    assert lib.wc_conv_slim_supported(None) == 0
    for field, bad in (('Cout', 48), ('Cout', 16), ('Cin', 48), ('N', 3), ('W', 1), ('ntaps', 17), ('nphase', 5)):
        gf, _ = _geoms('same', 2, 8, 8, 32, 32, 3)
        assert lib.wc_conv_slim_supported(ctypes.addressof(gf)) == 1
        setattr(gf, field, bad)                                     # (N = 3: 192 points, no whole tiles; W = 1: the division's rule)
        assert lib.wc_conv_slim_supported(ctypes.addressof(gf)) == 0, field
    # a slim width on a partial last tile is in no set
    gf, gd = _geoms('same', 3, 8, 8, 32, 32, 3)
    for g in (gf, gd):
        p = ctypes.addressof(g)
        assert lib.wc_conv_slim_supported(p) == 0 and lib.wc_conv_ragged_supported(p) == 0 and lib.wc_conv_supported(p) == 0


# 128-wide geometries: the three predicates and the plans answer what they answered before (values of the parent commit, written out)
WIDE = [('same', 2, 8, 8, 128, 128, 3, 8, 8), ('same', 4, 8, 8, 256, 128, 1, 2, 1), ('up3', 8, 8, 8, 128, 128, 3, 4, 8),
        ('same', 128, 16, 16, 256, 256, 3, 1, 1), ('same', 2, 4, 4, 128, 128, 3, None, None)]


@pytest.mark.parametrize("row", WIDE, ids=lambda r: '-'.join(str(v) for v in r[:7]))
def test_wide_geometries_are_unchanged(lib, row):
    kf, kd = row[7:]
    gf, gd = _geoms(*row[:7])
    for g, k in ((gf, kf), (gd, kd)):
        p = ctypes.addressof(g)
        if k is None:                                               # 32 points: ragged only
            assert lib.wc_conv_supported(p) == 0 and lib.wc_conv_ragged_supported(p) == 1 and lib.wc_conv_slim_supported(p) == 0
            continue
        assert lib.wc_conv_supported(p) == 1 and lib.wc_conv_ragged_supported(p) == 1 and lib.wc_conv_slim_supported(p) == 1
        assert lib.wc_conv_workspace_bytes(p) == (k * g.N * g.Hout * g.Wout * g.Cout * 4 if k > 1 else 0)


@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_workspaces(lib, row):
    gf, gd = _geoms(*row)
    for g in (gf, gd):
        ws = lib.wc_conv_workspace_bytes(ctypes.addressof(g))
        one = g.N * g.Hout * g.Wout * g.Cout * 4
        assert ws == 0 or (ws % one == 0 and 2 <= ws // one <= 8), (ws, one)
    wrw = lib.wc_conv_wrw_workspace_bytes(ctypes.addressof(gf))
    slices = gf.nphase * gf.ntaps * gf.Cin * gf.Cout * 4
    assert wrw > 0 and wrw % slices == 0 and 1 <= wrw // slices <= 256


def test_the_table_covers_both_epilogues_at_32_outputs(lib):
    assert route_labels(lib) == {('forward', 'direct'), ('forward', 'ksplit'), ('dgrad', 'direct'), ('dgrad', 'ksplit')}


class _T:
    """a tensor as conv.supported sees it, without a device"""
    is_cuda = True

    def __init__(self, *shape):
        import torch
        self.shape, self.dtype = tuple(shape), torch.float32

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True


@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_the_layer_entry_takes_these_widths_only_for_a_marked_layer(lib, row):
    from wc_gan_amd import conv as C
    kind, N, H, W, ci, co, k = row
    x, w = _T(N, H, W, ci), _T(co, ci, k, k)
    assert not C._plan(kind, x, w) and not C._plan(kind, x, w, slim=False)
    p = C._plan(kind, x, w, slim=True)
    assert p and p.ok and p.wrw_ws > 0
    if slim_side(row):
        assert not (p.pair or p.res or p.tail or p.bwd_tail)
    assert C.supported(x, w, kind) is False and C.supported(x, w, kind, slim=True) is True
    assert C.supported(x, w, kind, ragged=True) is False and C.supported(x, w, kind, ragged=True, slim=True) is True
    assert C.supported(x, w, kind) is False                         # (the plan cache keeps the answers apart)
    assert C.takes_planes((N, H, W, ci), (co, ci, k, k), kind) is False      # the planes hand-overs do not pass the mark


def test_the_mark(lib):
    from wc_gan_amd import conv as C

    class Site:
        slim_conv = True
    assert C._slim(Site()) is True and C._slim(object()) is False and C._slim(None) is False
    # a layer marked both ways at a slim width on a partial last tile keeps torch's route; a 128-wide layer answers as it always did
    assert C.supported(_T(3, 8, 8, 32), _T(32, 32, 3, 3), 'same', ragged=True, slim=True) is False
    x, w = _T(128, 8, 8, 128), _T(128, 128, 3, 3)
    p_off, p_on = C._plan('same', x, w), C._plan('same', x, w, slim=True)
    for f in ('ok', 'fwd_ws', 'bwd_ws', 'wrw_ws', 'pair', 'res', 'tail', 'bwd_tail'):
        assert getattr(p_off, f) == getattr(p_on, f), f
    # the critic's kinds are not the mark's: 'down3' at 64 channels stays where it was
    assert not C._plan('down3', _T(2, 16, 16, 64), _T(64, 64, 3, 3), slim=True)
    # the 32 -> 3 last layer is declined with the mark on too
    assert C.supported(_T(2, 8, 8, 32), _T(3, 32, 3, 3), 'same', slim=True) is False


def test_layers_carry_the_mark():
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.generator import Conv2D, make_generator
    assert Conv2D(32, 32).slim_conv is False and Conv2D(32, 32, slim_conv=True).slim_conv is True
    kw = dict(block_sizes=(64, 32), resamples=('UP', 'UP'), first_block_shape=(4, 4, 64), block_norm='d', block_after_norm='uconv',
              last_norm='d', last_after_norm='uconv')
    for on in (False, True):
        G = make_generator(slim_conv=on, **kw)
        marks = [m.slim_conv for m in G.modules() if isinstance(m, Conv2D)]
        assert len(marks) == 7 and all(v is on for v in marks)
    with pytest.raises(TypeError):
        make_discriminator(slim_conv=True)                          # the critic has no such mark


def test_the_imagenet_recipe():
    """every value from scripts/imagenet_resnet_sn_cond_sa.sh and run.py:147-237 (--dataset imagenet), written out"""
    from wc_gan_amd import train as T
    assert list(T.IMAGENET_CONFIGS) == ['imagenet_cond_sa'] and 'imagenet_cond_sa' not in T.CONFIGS
    cfg = T.IMAGENET_CONFIGS['imagenet_cond_sa']
    assert cfg['generator'] == dict(
        block_sizes=(128, 128, 128, 64, 32), resamples=('UP', 'UP', 'UP', 'UP', 'UP'), first_block_shape=(4, 4, 128), number_of_classes=1000,
        block_norm='d', block_after_norm='ufconv', filters_emb=32, last_norm='d', last_after_norm='uconv', gan_type='PROJECTIVE',
        slim_conv=T.IMAGENET_SLIM_SHIPS)
    assert cfg['discriminator'] == dict(
        input_image_shape=(128, 128, 3), block_sizes=(64, 128, 256, 512, 1024, 1024),
        resamples=('DOWN', 'DOWN', 'DOWN', 'DOWN', 'DOWN', 'SAME'), number_of_classes=1000, type='PROJECTIVE', spectral=True, sum_pool=True,
        conv_singular=False, filters_emb=32)
    assert cfg['image_shape'] == (128, 128, 3) and cfg['conditional'] is True
    assert set(cfg) == {'generator', 'discriminator', 'image_shape', 'conditional'}
    assert isinstance(T.IMAGENET_SLIM_SHIPS, bool)
    assert T.IMAGENET_SCHEDULES == {'imagenet_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=450, generator_lr=5e-4,
                                                             discriminator_lr=5e-4)}
    # five UP blocks from 4 x 4: 128 x 128 images
    assert cfg['generator']['first_block_shape'][0] * 2 ** len(cfg['generator']['resamples']) == cfg['image_shape'][0]


def test_slim_config_toggles_the_generators_mark_alone():
    import copy
    from wc_gan_amd import train as T
    cfg = T.IMAGENET_CONFIGS['imagenet_cond_sa']
    before = copy.deepcopy(cfg)
    on, off = T.slim_config(cfg), T.slim_config(cfg, on=False)
    assert cfg == before                                            # the entry itself is left alone
    assert on['generator']['slim_conv'] is True and off['generator']['slim_conv'] is False
    for out in (on, off):
        assert {k: v for k, v in out['generator'].items() if k != 'slim_conv'} == {k: v for k, v in cfg['generator'].items() if k != 'slim_conv'}
        assert out['discriminator'] == cfg['discriminator'] and 'slim_conv' not in out['discriminator']
        assert {k: out[k] for k in out if k not in ('generator', 'discriminator')} == {k: cfg[k] for k in cfg if k not in ('generator', 'discriminator')}
