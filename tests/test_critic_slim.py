"""CPU tests of the critic's opt-in for 64-wide block layers (make_discriminator(slim_blocks=True), wc_gan_amd/conv.py's `blocks=`,
train.slim_blocks_config): what the layer entry, the fused nodes' plans and the recipe helper answer with the mark off and on, and the
k-split classes of the rows tests/test_critic_slim_gpu.py runs.  No kernel is launched.  DESIGN.md section 4.23."""
import copy
import ctypes
import os

import pytest

from test_conv_slim import _T


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# kind, N, H, W, Cin, Cout, k: the layer rows of tests/test_critic_slim_gpu.py (which imports them)
ROWS = [
    ('down3', 2, 16, 16, 64, 64, 3),         # one output tile
    ('down3', 6, 16, 16, 64, 64, 3),         # three tiles
    ('down3', 8, 12, 16, 64, 64, 3),         # tiles straddle images, H != W
    ('down3', 4, 112, 112, 64, 64, 3),       # 98 tiles: the direct epilogue
    ('same', 2, 8, 8, 64, 128, 3),
    ('same', 4, 56, 56, 64, 128, 3),
    ('same', 2, 8, 8, 64, 128, 1),
    ('same', 2, 8, 8, 64, 64, 3),
]
ROW_ID = lambda r: '-'.join(str(v) for v in r)


def _xw(row):
    kind, N, H, W, ci, co, k = row
    return kind, _T(N, H, W, ci), _T(co, ci, k, k)


@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_the_layer_entry_takes_64_wide_critic_layers_only_for_a_marked_layer(lib, row):
    from wc_gan_amd import conv as C
    kind, x, w = _xw(row)
    assert not C._plan(kind, x, w) and C.supported(x, w, kind) is False
    if kind == 'down3':
        assert not C._plan(kind, x, w, slim=True)                   # the generator's mark does not open the critic's kind
    p = C._plan(kind, x, w, blocks=True)
    assert p and p.ok and p.wrw_ws > 0
    assert C.supported(x, w, kind, blocks=True) is True and C.supported(x, w, kind, ragged=True, blocks=True) is True
    assert C.supported(x, w, kind) is False                         # (the plan cache keeps the answers apart)
    if row[5] == 64:                                                # a 64-output geometry: the two-launch routes inside the nodes
        assert not (p.pair or p.res or p.tail)


def test_the_mark_and_the_plan_key(lib):
    from wc_gan_amd import conv as C

    class Site:
        slim_blocks = True
    assert C._blocks(Site()) is True and C._blocks(object()) is False and C._blocks(None) is False
    x, w = _T(2, 16, 16, 64), _T(64, 64, 3, 3)
    C._plan('down3', x, w), C._plan('down3', x, w, slim=True), C._plan('down3', x, w, blocks=True)
    base = ('down3', (2, 16, 16, 64), (64, 64, 3, 3), False)
    assert base in C._plans and base + (True,) in C._plans and base + ('blocks',) in C._plans
    assert C._plans[base] is False and C._plans[base + (True,)] is False and C._plans[base + ('blocks',)].ok
    # a 128-wide layer's plan is the same marked and unmarked
    for kind, x, w in (('same', _T(128, 8, 8, 128), _T(128, 128, 3, 3)), ('down3', _T(8, 16, 16, 128), _T(128, 128, 3, 3))):
        p_off, p_on = C._plan(kind, x, w), C._plan(kind, x, w, blocks=True)
        for f in ('ok', 'fwd_ws', 'bwd_ws', 'wrw_ws', 'pair', 'res', 'tail', 'bwd_tail'):
            assert getattr(p_off, f) == getattr(p_on, f), f
    # 32-wide critic layers, and the mark's other kinds, stay declined
    assert not C._plan('same', _T(2, 8, 8, 32), _T(32, 32, 3, 3), blocks=True)
    assert not C._plan('down3', _T(2, 16, 16, 32), _T(64, 32, 3, 3), blocks=True)
    assert not C._plan('same', _T(2, 8, 8, 64), _T(96, 64, 3, 3), blocks=True)
    assert not C._plan('up3', _T(2, 8, 8, 64), _T(64, 64, 3, 3), blocks=True)


def test_a_layer_marked_both_ways_follows_the_ragged_predicate(lib):
    from wc_gan_amd import conv as C
    # 3 x 8 x 8 = 192 points: a partial last tile -- the whole-tile predicate declines, the ragged one takes it
    x, w = _T(3, 8, 8, 64), _T(128, 64, 3, 3)
    gf, gd = (g[0] for g in C._geoms('same', 3, 8, 8, w))
    for g in (gf, gd):
        assert lib.wc_conv_supported(ctypes.addressof(g)) == 0 and lib.wc_conv_ragged_supported(ctypes.addressof(g)) == 1
    assert C.supported(x, w, 'same', blocks=True) is False
    assert C.supported(x, w, 'same', ragged=True, blocks=True) is True
    assert C.supported(x, w, 'same', ragged=True) is False


def test_fused_node_plans(lib):
    from wc_gan_amd import conv as C
    x = (8, 8, 8, 64)
    shapes = (x, (128, 64, 3, 3), (128, 128, 3, 3), (128, 64, 1, 1), True)
    assert C.critic_block_plans(*shapes) is None and C.critic_block_plans(*shapes, ragged=True) is None
    plans = C.critic_block_plans(*shapes, blocks=True)
    assert plans is not None and all(p.ok for p in plans)
    # identity shortcut at 64
    same = ((8, 8, 8, 64), (64, 64, 3, 3), (64, 64, 3, 3), None, False)
    assert C.critic_block_plans(*same) is None
    p1, p2, ps = C.critic_block_plans(*same, blocks=True)
    assert p1.ok and p2.ok and ps is None and not (p1.pair or p1.res or p1.tail or p2.pair or p2.res or p2.tail)
    # a 128-wide block: the very plan objects' fields, marked or not
    wide = ((8, 8, 8, 128), (128, 128, 3, 3), (128, 128, 3, 3), None, False)
    for a, b in zip(C.critic_block_plans(*wide), C.critic_block_plans(*wide, blocks=True)):
        assert (a is None and b is None) or all(getattr(a, f) == getattr(b, f) for f in ('ok', 'fwd_ws', 'bwd_ws', 'wrw_ws', 'pair', 'res', 'tail'))


def _critic(on, sizes=(64, 128, 128), resamples=('DOWN', 'DOWN', 'SAME'), **kw):
    from wc_gan_amd.discriminator import make_discriminator
    return make_discriminator(input_image_shape=(16, 16, 3), block_sizes=sizes, resamples=resamples, type=None, spectral=False,
                              conv_singular=False, sum_pool=True, slim_blocks=on, **kw)


def test_make_discriminator_marks_every_conv2d_and_the_blocks_answer():
    from wc_gan_amd.generator import Conv2D
    import torch
    torch.manual_seed(0)
    assert Conv2D(64, 64).slim_blocks is False and Conv2D(64, 64, slim_blocks=True).slim_blocks is True
    for on in (False, True):
        D = _critic(on)
        marks = [m.slim_blocks for m in D.modules() if isinstance(m, Conv2D)]
        assert len(marks) == 3 + 3 + 2 and all(v is on for v in marks)
        first = D.blocks[0]._first_plan_of((8, 16, 16, 3))
        second = D.blocks[1]._plans_of((8, 8, 8, 64))
        if on:
            assert first is not None and first.ok and second is not None and all(p.ok for p in second)
        else:
            assert first is None and second is None
        assert D.blocks[2]._plans_of((8, 4, 4, 128)) is not None    # the 128-wide block: taken either way
    with pytest.raises(TypeError):
        _critic(False, slim_conv=True)


def test_slim_blocks_config_toggles_the_critics_mark_alone():
    from wc_gan_amd import train as T
    cfg = T.IMAGENET_CONFIGS['imagenet_cond_sa']
    before = copy.deepcopy(cfg)
    on, off = T.slim_blocks_config(cfg), T.slim_blocks_config(cfg, on=False)
    assert cfg == before and 'slim_blocks' not in cfg['discriminator']
    assert on['discriminator']['slim_blocks'] is True and off['discriminator']['slim_blocks'] is False
    for out in (on, off):
        assert {k: v for k, v in out['discriminator'].items() if k != 'slim_blocks'} == cfg['discriminator']
        assert out['generator'] == cfg['generator']
        assert {k: out[k] for k in out if k not in ('generator', 'discriminator')} == {k: cfg[k] for k in cfg if k not in ('generator', 'discriminator')}
    assert isinstance(T.IMAGENET_SLIM_BLOCKS_SHIPS, bool)
    # slim_config never touches the critic, marked or not
    assert T.slim_config(on)['discriminator'] == on['discriminator']
    # any recipe
    assert T.slim_blocks_config(T.CONFIGS['cifar10_cond'])['discriminator']['slim_blocks'] is True


# ---- the k-split classes of the GPU rows: both epilogues, and the F1 tail at Cin = 64 -----------------------------------------------------
def classes(lib):
    """{row: (forward 'direct' | 'ksplit', data gradient likewise)} from wc_conv_workspace_bytes (0 = direct)"""
    from wc_gan_amd import conv as C
    out = {}
    for row in ROWS:
        kind, x, w = _xw(row)
        (gf, _, _), (gd, _, _) = C._geoms(kind, row[1], row[2], row[3], w)
        out[row] = tuple('ksplit' if lib.wc_conv_workspace_bytes(ctypes.addressof(g)) else 'direct' for g in (gf, gd))
    return out


def test_the_rows_cover_both_epilogues_and_the_f1_tail_at_64_inputs(lib):
    from wc_gan_amd import conv as C
    cl = classes(lib)
    down = {cl[r] for r in ROWS if r[0] == 'down3'}
    assert {c[0] for c in down} == {'direct', 'ksplit'} and {c[1] for c in down} == {'direct', 'ksplit'}, cl
    same = {cl[r] for r in ROWS if r[0] == 'same'}
    assert {c[0] for c in same} == {'direct', 'ksplit'}, cl
    assert cl[('down3', 4, 112, 112, 64, 64, 3)][0] == 'direct' and cl[('down3', 2, 16, 16, 64, 64, 3)][0] == 'ksplit'
    # a 64 -> 128 conv1 at a small grid shares its tap loop: its finish can write conv2's planes (F1) with Cin = 64
    kind, x, w = _xw(('same', 2, 8, 8, 64, 128, 3))
    p = C._plan(kind, x, w, blocks=True)
    assert p.fwd_ws > 0 and p.tail and p.fwd[0].Cin == 64
    # ... and so it does in the cut-down critic of the GPU tests (batch 8 on 16 x 16 images: block 1 reads 8 x 8 x 64)
    p1, p2, ps = C.critic_block_plans((8, 8, 8, 64), (128, 64, 3, 3), (128, 128, 3, 3), (128, 64, 1, 1), True, blocks=True)
    assert p1.tail and p1.fwd_ws > 0
