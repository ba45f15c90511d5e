"""The launch arithmetic of the kernels that move the bytes -- K3, the fused apply (affine_ring_kernel, apply_split_kernel) and K6, the
backward apply (onepass_ring_kernel, affine_f16x3_kernel), with rows_gemm_kernel behind both -- restated in a few lines each, ONLY to
label the rows of test_apply_dispatch_gpu.py: which kernel a shape reaches, its tiles and grid, {tiles per workgroup: how many
workgroups}, idle workgroup pairs, and whether tiles straddle samples.  These kernels pick their s_waitcnt schedule from the number of
tiles a workgroup owns (csrc/wc_fast.hip W0...W4: n = 1, 2, 3, 4, >= 5; csrc/wc_split.hip: `def_mode = n >= 6`; affine_f16x3_kernel:
n = 1, 2, >= 3), so every row states its class as literals and this file checks them against the restatement: a later change to a
launch function fails a row instead of emptying it of its purpose.  The restatement is pinned to the library through the support
predicates here and, on the GPU, through the number of per-workgroup maxima the planes forms write (= the grid).

Also here, on the CPU: the conditions on the GPU test's inputs (slot draws, straddling tiles, a per-tile offset in every tile) and two
sensitivity checks in numpy -- the errors the GPU rows are there to catch are four orders of magnitude above their bounds."""
import functools
from collections import Counter

import numpy as np
import pytest

K3_TOL = 3e-6       # K3, K6 and apply_split against float64 (test_fast_gpu.py, test_split_gpu.py, test_site_dispatch_gpu.py)


def _ceil(a, b):
    return -(-a // b)


def nhwc(shape):
    return shape[0], int(np.prod(shape[1:-1])), shape[-1]


# ---- host predicates, restated (csrc/wc_fast.hip, csrc/wc_split.hip) ---------------------------------------------------------------
def fast_affine_supported(shape):
    """wc_fast_affine_supported: whole 16384 / C-row tiles, at least 1024 rows"""
    N, HW, C = nhwc(shape)
    return C in (32, 64, 128, 256) and N * HW >= 1024 and N * HW % (16384 // C) == 0


def split_apply_supported(shape):
    N, HW, C = nhwc(shape)
    return C in (128, 256) and N * HW % (8192 // C) == 0


def onepass_supported(shape):
    """K6 with K4's scales takes onepass_ring_kernel (bwd_apply_impl, csrc/wc_abi.hip)"""
    N, HW, C = nhwc(shape)
    return fast_affine_supported(shape) and C == 256 and N * HW % 16 == 0 and N * HW >= 4096


# ---- the five launches, restated to label rows with --------------------------------------------------------------------------------
def _plan(kernel, T, owned, grid, straddle):
    counts = dict(Counter(len(o) for o in owned if o))
    return dict(kernel=kernel, T=T, ntiles=sum(len(o) for o in owned), grid=grid, counts=counts, idle=sum(1 for o in owned if not o),
                straddle=straddle, owned=owned)


def _tiles(kernel, shape, T, has_slot):
    """launch_affine_ring<C>, launch_apply_split<C>, launch_affine<C>: up to 256 workgroups of equal ceil(ntiles / nwg) tiles --
    contiguous runs with a slot table (the last one short), interleaved (tile = block + i * grid) without"""
    N, HW, C = nhwc(shape)
    ntiles = N * HW // T
    nwg = min(ntiles, 256)
    tpw = _ceil(ntiles, nwg)
    nwg = _ceil(ntiles, tpw)
    owned = [list(range(w * tpw, min(ntiles, (w + 1) * tpw))) if has_slot else list(range(w, ntiles, nwg)) for w in range(nwg)]
    return _plan(kernel, T, owned, nwg, has_slot and HW % T != 0)


def plan_rows(shape, has_slot):
    """wc_launch_rows_gemm: 128-row blocks, per sample when slots are given, times ceil(C / 128) column blocks; `counts` = {rows of a
    block: how many row blocks}"""
    N, HW, C = nhwc(shape)
    seg = [HW] * N if has_slot else [N * HW]
    rows = [min(128, s - 128 * i) for s in seg for i in range(_ceil(s, 128))]
    return dict(kernel='rows_gemm_kernel', T=128, ntiles=len(rows), grid=len(rows) * _ceil(C, 128), counts=dict(Counter(rows)), idle=0,
                straddle=False, owned=[[i] for i in range(len(rows))])


def plan_ring(shape, has_slot):
    """K3 on fp32 (wc_apply_act_f32 / wc_apply_mask_f32 / wc_apply_planes_f32 with a plan): affine_ring_kernel<C> on 8192 / C-row
    tiles where wc_fast_affine_supported, else rows_gemm_kernel"""
    if not fast_affine_supported(shape):
        return plan_rows(shape, has_slot)
    return _tiles('affine_ring_kernel', shape, 8192 // shape[-1], has_slot)


def plan_split(shape, has_slot):
    """K3 on planes (wc_apply_split_ex_f16x2): apply_split_kernel<C>, the same arithmetic; its second schedule from 6 tiles on"""
    assert split_apply_supported(shape)
    return _tiles('apply_split_kernel', shape, 8192 // shape[-1], has_slot)


def plan_onepass(shape, has_slot):
    """wc_launch_bwd_apply_onepass: 16-row tiles over min(ntiles, 128) workgroup PAIRS rounded up to a multiple of 8; `grid` = 2 x pairs,
    `counts` per pair, pairs past the last tile idle (`n <= 0` returns)"""
    assert onepass_supported(shape)
    N, HW, C = nhwc(shape)
    ntiles = N * HW // 16
    pairs = _ceil(min(ntiles, 128), 8) * 8
    tpp = _ceil(ntiles, pairs)
    owned = [list(range(p * tpp, min(ntiles, (p + 1) * tpp))) if has_slot else list(range(p, ntiles, pairs)) for p in range(pairs)]
    return _plan('onepass_ring_kernel', 16, owned, 2 * pairs, has_slot and HW % 16 != 0)


def plan_acc(shape, has_slot):
    """launch_affine<C>: affine_f16x3_kernel on 16384 / C-row tiles (the accumulating pass of a two-pass K6)"""
    assert fast_affine_supported(shape)
    return _tiles('affine_f16x3_kernel', shape, 16384 // shape[-1], has_slot)


def label(p):
    return (p['kernel'], p['ntiles'], p['grid'], p['counts'], p['idle'], p['straddle'])


# ---- the rows: shape, Kc (1: no slot table), the class as literals ------------------------------------------------------------------
# (kernel, tiles, grid, {tiles per workgroup: workgroups}, idle pairs, tiles straddle samples)
RING, SPLIT, ONE, ACC, ROWS = 'affine_ring_kernel', 'apply_split_kernel', 'onepass_ring_kernel', 'affine_f16x3_kernel', 'rows_gemm_kernel'

BASE = [(4, 16, 16, 256), (257, 8, 4, 256), (65, 16, 16, 256), (97, 16, 16, 256), (129, 16, 16, 256), (161, 16, 16, 256)]
_BASE_SLOT = [{1: 32}, {2: 128, 1: 1}, {3: 173, 1: 1}, {4: 194}, {5: 206, 2: 1}, {6: 214, 4: 1}]
_BASE_NONE = [{1: 32}, {2: 128, 1: 1}, {3: 172, 2: 2}, {4: 194}, {5: 204, 4: 3}, {6: 213, 5: 2}]
_BASE_TILES = [(32, 32), (257, 129), (520, 174), (776, 194), (1032, 207), (1288, 215)]

# K3 on fp32.  8224 = 257 x 32 rows are no whole 64-row tiles (the fast path wants 16384 / C-row multiples, so the ring kernel's tile
# count at C = 256 is always even): wc_fast_affine_supported declines (257, 8, 4, 256), (58, 12, 12, 256) and (259, 8, 8, 128), and
# rows_gemm_kernel takes them.  They stay as rows (apply_split_kernel takes the same shapes); (60, 12, 12, 256) and (260, 8, 8, 128)
# are their nearest neighbours on the ring kernel.
RING_ROWS = [(s, Kc, (RING, t, g, (cs if Kc > 1 else cn), 0, False))
             for s, (t, g), cs, cn in zip(BASE, _BASE_TILES, _BASE_SLOT, _BASE_NONE) for Kc in (1, 3) if s != (257, 8, 4, 256)] + [
    ((257, 8, 4, 256), 1, (ROWS, 65, 130, {128: 64, 32: 1}, 0, False)),
    ((257, 8, 4, 256), 3, (ROWS, 257, 514, {32: 257}, 0, False)),
    ((58, 12, 12, 256), 3, (ROWS, 116, 232, {128: 58, 16: 58}, 0, False)),
    ((60, 12, 12, 256), 3, (RING, 270, 135, {2: 135}, 0, True)),            # HW = 144: tiles straddle samples, redone per row
    ((128, 4, 4, 256), 3, (RING, 64, 64, {1: 64}, 0, True)),               # HW = 16 < the tile: every tile spans two samples
    ((130, 16, 16, 128), 3, (RING, 520, 174, {3: 173, 1: 1}, 0, False)),
    ((259, 8, 8, 128), 3, (ROWS, 259, 259, {64: 259}, 0, False)),
    ((260, 8, 8, 128), 3, (RING, 260, 130, {2: 130}, 0, False)),           # HW = 64 equals the tile
    ((161, 16, 16, 64), 3, (RING, 322, 161, {2: 161}, 0, False)),
    ((129, 32, 16, 32), 3, (RING, 258, 129, {2: 129}, 0, False)),          # C = 32: 66048 = 129 x 512 rows
]

SPLIT_ROWS = [(s, Kc, (SPLIT, t, g, (cs if Kc > 1 else cn), 0, False))
              for s, (t, g), cs, cn in zip(BASE, _BASE_TILES, _BASE_SLOT, _BASE_NONE) for Kc in (1, 3)] + [
    ((225, 16, 16, 256), 1, (SPLIT, 1800, 225, {8: 225}, 0, False)),        # the second schedule with steady tiles
    ((225, 16, 16, 256), 3, (SPLIT, 1800, 225, {8: 225}, 0, False)),
    ((193, 16, 16, 256), 1, (SPLIT, 1544, 221, {7: 218, 6: 3}, 0, False)),
    ((193, 16, 16, 256), 3, (SPLIT, 1544, 221, {7: 220, 4: 1}, 0, False)),  # ... and a short last workgroup on the first schedule
    ((58, 12, 12, 256), 3, (SPLIT, 261, 131, {2: 130, 1: 1}, 0, True)),
    ((128, 4, 4, 256), 3, (SPLIT, 64, 64, {1: 64}, 0, True)),
    ((1, 8, 4, 256), 1, (SPLIT, 1, 1, {1: 1}, 0, False)),
    ((321, 16, 16, 128), 1, (SPLIT, 1284, 214, {6: 214}, 0, False)),        # the second schedule at C = 128
    ((321, 16, 16, 128), 3, (SPLIT, 1284, 214, {6: 214}, 0, False)),
]

# K6 with K4's scales at C = 256; the last column: the bit-mask and planes forms run too (wc_bwd_bits_supported / wc_bwd_xsplit_supported)
ONEPASS_ROWS = [
    ((64, 8, 8, 256), 1, (ONE, 256, 256, {2: 128}, 0, False), False),
    ((64, 8, 8, 256), 3, (ONE, 256, 256, {2: 128}, 0, False), False),
    ((65, 8, 8, 256), 1, (ONE, 260, 256, {3: 4, 2: 124}, 0, False), False),
    ((65, 8, 8, 256), 3, (ONE, 260, 256, {3: 86, 2: 1}, 41, False), False),
    ((67, 8, 8, 256), 3, (ONE, 268, 256, {3: 89, 1: 1}, 38, False), False),           # a one-tile last pair
    ((97, 8, 8, 256), 1, (ONE, 388, 256, {4: 4, 3: 124}, 0, False), False),
    ((97, 8, 8, 256), 3, (ONE, 388, 256, {4: 97}, 31, False), False),
    ((129, 8, 8, 256), 1, (ONE, 516, 256, {5: 4, 4: 124}, 0, False), False),
    ((129, 8, 8, 256), 3, (ONE, 516, 256, {5: 103, 1: 1}, 24, False), False),         # a one-tile tail behind full schedules
    ((128, 6, 6, 256), 3, (ONE, 288, 256, {3: 96}, 32, True), False),                # HW = 36: the one-pass kernel's per-row redo
    ((65, 16, 16, 256), 1, (ONE, 1040, 256, {9: 16, 8: 112}, 0, False), True),
    ((65, 16, 16, 256), 3, (ONE, 1040, 256, {9: 115, 5: 1}, 12, False), True),
    ((66, 16, 16, 256), 1, (ONE, 1056, 256, {9: 32, 8: 96}, 0, False), True),
    ((66, 16, 16, 256), 3, (ONE, 1056, 256, {9: 117, 3: 1}, 10, False), True),
]

# the accumulating pass dx += (x - mu) S of a two-pass K6 (shared table: no slot in THIS pass, whatever Kc): shape, Kc, scales given
ACC_ROWS = [
    ((16, 8, 8, 256), 3, False, (ACC, 16, 16, {1: 16}, 0, False)),
    ((97, 16, 16, 256), 3, False, (ACC, 388, 194, {2: 194}, 0, False)),
    ((129, 16, 16, 256), 3, False, (ACC, 516, 172, {3: 172}, 0, False)),
    ((130, 16, 16, 128), 3, True, (ACC, 260, 130, {2: 130}, 0, False)),
    ((260, 16, 16, 128), 3, True, (ACC, 520, 174, {3: 172, 2: 2}, 0, False)),
    ((260, 16, 16, 64), 3, True, (ACC, 260, 130, {2: 130}, 0, False)),
]

# wc_bwd_apply_xsplit_f32 at C = 128 with a slot table: the planes kernel, then affine_f16x3_kernel<128, ACC, SLOT> -- ONE table per
# 128-row tile.  Last column: does the library take the shape (wc_bwd_xsplit_supported)?  It must not where HW % 128 != 0.
XSPLIT128_ROWS = [
    ((64, 16, 16, 128), 3, (ACC, 128, 128, {1: 128}, 0, False), True),             # HW = 256: two tiles per sample, the control
    ((256, 8, 8, 128), 3, (ACC, 128, 128, {1: 128}, 0, True), False),              # HW = 64: every tile holds two samples
    ((32, 24, 24, 128), 3, (ACC, 144, 144, {1: 144}, 0, True), False),             # HW = 576 = 4.5 tiles
    ((320, 8, 8, 128), 3, (ACC, 160, 160, {1: 160}, 0, True), False),              # ... at 20480 rows, where the layers hand a site planes
]

# rows_gemm_kernel: `fast=False`, and shapes the fast path declines
GEMM_ROWS = [
    ((5, 3, 3, 96), 3, (ROWS, 5, 5, {9: 5}, 0, False)),                     # HW = 9: one ragged block per sample
    ((3, 13, 11, 160), 3, (ROWS, 6, 12, {128: 3, 15: 3}, 0, False)),        # HW = 143: the second block ragged; two column blocks, the second 32 wide
    ((7, 5, 5, 512), 1, (ROWS, 2, 8, {128: 1, 47: 1}, 0, False)),           # M = 175
]


def row_id(r):
    return 'x'.join(map(str, r[0])) + f'-Kc{r[1]}'


def _check(plan, want):
    assert label(plan) == want, (label(plan), want)


@pytest.mark.parametrize("row", RING_ROWS, ids=row_id)
def test_ring_rows_are_in_their_class(row):
    _check(plan_ring(row[0], row[1] > 1), row[2])


@pytest.mark.parametrize("row", SPLIT_ROWS, ids=row_id)
def test_split_rows_are_in_their_class(row):
    _check(plan_split(row[0], row[1] > 1), row[2])


@pytest.mark.parametrize("row", ONEPASS_ROWS, ids=row_id)
def test_onepass_rows_are_in_their_class(row):
    _check(plan_onepass(row[0], row[1] > 1), row[2])


@pytest.mark.parametrize("row", ACC_ROWS, ids=row_id)
def test_accumulating_rows_are_in_their_class(row):
    shape, Kc, scales, want = row
    _check(plan_acc(shape, False), want)
    assert not (scales and onepass_supported(shape))        # with scales C = 256 would take the one-pass kernel instead


@pytest.mark.parametrize("row", XSPLIT128_ROWS, ids=row_id)
def test_xsplit128_rows_are_in_their_class(row):
    _check(plan_acc(row[0], True), row[2])
    assert row[3] == (not row[2][5])        # taken exactly where no tile straddles samples


@pytest.mark.parametrize("row", GEMM_ROWS, ids=row_id)
def test_gemm_rows_are_in_their_class(row):
    _check(plan_rows(row[0], row[1] > 1), row[2])
    assert not fast_affine_supported(row[0])


def test_every_schedule_class_has_a_row():
    """n = 1, 2, 3, 4, 5 and 6 tiles per workgroup on both K3 kernels and 1...5 per pair on the one-pass kernel, with and without
    slots; the split kernel's second schedule with steady tiles (n >= 7); idle pairs; a straddling row on each ring; n = 1, 2, 3 on
    the accumulating kernel"""
    for rows, with_slots, without in ((RING_ROWS, {1, 2, 3, 4, 5, 6}, {1, 3, 4, 5, 6}), (SPLIT_ROWS, {1, 2, 3, 4, 5, 6, 7, 8}, {1, 2, 3, 4, 5, 6, 7, 8}),
                                      (ONEPASS_ROWS, {1, 2, 3, 4, 5}, {2, 3, 4, 5})):
        for has_slot, want in ((True, with_slots), (False, without)):
            seen = {n for r in rows if (r[1] > 1) == has_slot and r[2][0] != ROWS for n in r[2][3]}
            assert want <= seen, (rows[0][2][0], has_slot, seen)
        assert any(r[2][5] for r in rows)
    assert any(r[2][4] > 0 for r in ONEPASS_ROWS)
    assert {n for r in ACC_ROWS for n in r[3][3]} >= {1, 2, 3}


# ---- the restated predicates against the library's ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import os
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _all_shapes():
    return sorted({(r[0], r[1]) for rows in (RING_ROWS, SPLIT_ROWS, ONEPASS_ROWS, ACC_ROWS, XSPLIT128_ROWS, GEMM_ROWS) for r in rows})


def test_the_restated_predicates_are_the_librarys(lib):
    for shape, Kc in _all_shapes():
        N, HW, C = nhwc(shape)
        fast = fast_affine_supported(shape)
        nb = lib.wc_apply_workspace_bytes(N, HW, C, Kc)
        assert (nb > 256) == fast and (fast or nb == 256), (shape, nb)        # 256 off the fast path
        assert lib.wc_apply_planes_supported(N, HW, C) == int(fast and C in (128, 256)), shape
        assert lib.wc_apply_split_supported(N, HW, C) == int(split_apply_supported(shape)), shape
        if lib.wc_bwd_bits_supported(N, HW, C, int(Kc > 1)):
            assert onepass_supported(shape) and N * HW >= 16384, shape
        if lib.wc_bwd_xsplit_supported(N, HW, C, int(Kc > 1)):
            assert N * HW >= 16384 and (onepass_supported(shape) if C == 256 else split_apply_supported(shape) and fast), shape


def test_the_predicates_of_the_bit_mask_and_planes_rows(lib):
    for shape, Kc, _want, forms in ONEPASS_ROWS:
        N, HW, C = nhwc(shape)
        assert lib.wc_bwd_bits_supported(N, HW, C, int(Kc > 1)) == int(forms), shape
        assert lib.wc_bwd_xsplit_supported(N, HW, C, int(Kc > 1)) == int(forms), shape
    for shape, Kc, _want, taken in XSPLIT128_ROWS:
        N, HW, C = nhwc(shape)
        assert lib.wc_bwd_xsplit_supported(N, HW, C, 1) == int(taken), shape
        assert lib.wc_bwd_xsplit_supported(N, HW, C, 0) == 1, shape              # without a slot table no tile can take a wrong one


# ---- the inputs of the GPU rows (numpy; the GPU test uploads exactly these) ---------------------------------------------------------
SHIFTED = 8         # channels that carry the per-tile offset


def shifted_channels(C):
    return np.array([1, 2, 3, C // 2, C // 2 + 1, C - 3, C - 2, C - 1])


def tile_offsets(ntiles):
    """(ntiles, SHIFTED): 3 to 8 standard deviations, another value in every tile and on every channel (golden-ratio style sequences:
    test_every_tile_carries_its_own_offset checks that consecutive tiles of a workgroup differ by standard deviations)"""
    alpha = np.sqrt(np.array([2, 3, 5, 7, 11, 13, 17, 19], np.float64)) % 1.0
    return 3.0 + 5.0 * ((np.arange(1, ntiles + 1)[:, None] * alpha[None, :]) % 1.0)


def draw_slot(N, Kc):
    """uniform draws; every odd sample is then moved off its predecessor's slot where the two agree, so that at least half of the
    adjacent pairs differ at any N (even samples may still repeat their predecessor: both cases occur)"""
    slot = np.random.default_rng(17).integers(0, Kc, N).astype(np.int32)
    if Kc > 1:
        odd = np.arange(1, N, 2)
        slot[odd] = np.where(slot[odd] == slot[odd - 1], (slot[odd] + 1) % Kc, slot[odd])
    return slot


def _shift(M, C, T):
    out = np.zeros((M, C))
    out[:, shifted_channels(C)] = np.repeat(tile_offsets(_ceil(M, T)), T, axis=0)[:M]
    return out


@functools.lru_cache(maxsize=2)
def k3_inputs(shape, Kc, T):
    """test_fast_apply_matches_float64's inputs (channels of different magnitude), plus the per-tile offset; never written to"""
    rng = np.random.default_rng(11)
    N, HW, C = nhwc(shape)
    mag = np.exp(rng.uniform(-3, 3, C))
    x = ((rng.standard_normal((N * HW, C)) + _shift(N * HW, C, T)) * mag + 3 * mag).astype(np.float32).reshape(shape)
    mu = (3 * mag).astype(np.float32)
    A = (rng.standard_normal((Kc, C, C)) / np.sqrt(C) / mag[None, :, None]).astype(np.float32)
    b = rng.standard_normal((Kc, C)).astype(np.float32)
    out = dict(x=x, mu=mu, A=A, b=b, slot=draw_slot(N, Kc), T=T)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def k6_inputs(shape, Kc, T):
    """test_fast_bwd_apply_matches_float64's inputs, plus the per-tile offset on both streams"""
    rng = np.random.default_rng(13)
    N, HW, C = nhwc(shape)
    sh = _shift(N * HW, C, T)
    x = (rng.standard_normal((N * HW, C)) + sh + 0.5).astype(np.float32).reshape(shape)
    gy = ((rng.standard_normal((N * HW, C)) + sh[:, ::-1]) * 1e-3).astype(np.float32).reshape(shape)
    mu = np.full(C, 0.5, np.float32)
    A = (rng.standard_normal((Kc, C, C)) / np.sqrt(C)).astype(np.float32)
    At = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    S = rng.standard_normal((C, C)).astype(np.float32) * 1e-4
    S = (S + S.T) / 2
    gm = (rng.standard_normal(C) * 1e-4).astype(np.float32)
    out = dict(x=x, gy=gy, mu=mu, At=At, S=S, gm=gm, slot=draw_slot(N, Kc), T=T)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def k3_ref(x, mu, A, b, rowslot):
    """float64 y = (x - mu) A[s] + b[s] with one table index PER ROW (M,)"""
    C = x.shape[-1]
    f = x.reshape(-1, C).astype(np.float64) - mu.astype(np.float64)
    y = np.empty_like(f)
    for k in np.unique(rowslot):
        y[rowslot == k] = f[rowslot == k] @ A[k].astype(np.float64) + b[k].astype(np.float64)
    return y


def k6_ref(gy, x, mu, At, S, gm, rowslot):
    """float64 dx = gy At[s] + (x - mu) S - gmean with one table index per row"""
    C = x.shape[-1]
    g = gy.reshape(-1, C).astype(np.float64)
    dx = (x.reshape(-1, C).astype(np.float64) - mu.astype(np.float64)) @ S.astype(np.float64) - gm.astype(np.float64)
    for k in np.unique(rowslot):
        dx[rowslot == k] += g[rowslot == k] @ At[k].astype(np.float64)
    return dx


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _slot_rows():
    for rows, plan in ((RING_ROWS, plan_ring), (SPLIT_ROWS, plan_split), (ONEPASS_ROWS, plan_onepass), (XSPLIT128_ROWS, lambda s, h: plan_acc(s, True)),
                       (GEMM_ROWS, plan_rows)):
        for r in rows:
            if r[1] > 1:
                yield r[0], r[1], plan(r[0], True)
    for r in ACC_ROWS:
        yield r[0], r[1], plan_acc(r[0], False)


def _straddling(p, shape, slot):
    """the tiles whose rows belong to samples of different slots"""
    N, HW, C = nhwc(shape)
    rowslot = np.repeat(slot, HW)[:p['ntiles'] * p['T']].reshape(p['ntiles'], p['T'])
    return int((rowslot != rowslot[:, :1]).any(1).sum())


def test_slot_draws_and_straddling_tiles():
    """the GPU rows cannot hide behind their inputs: with slots at least a quarter of the adjacent samples differ, and in a straddling
    row at least 8 tiles hold samples of different slots"""
    for shape, Kc, p in _slot_rows():
        slot = draw_slot(shape[0], Kc)          # (k3_inputs and k6_inputs take exactly this draw)
        assert slot.min() >= 0 and slot.max() < Kc
        if shape[0] > 1:
            assert (slot[1:] != slot[:-1]).mean() >= 0.25, (shape, Kc)
        if p['kernel'] == ROWS:         # blocks are cut per sample
            continue
        if p['straddle']:
            assert _straddling(p, shape, slot) >= 8, (shape, _straddling(p, shape, slot))
        else:
            assert _straddling(p, shape, slot) == 0


def test_every_tile_carries_its_own_offset():
    """any two consecutive tiles of a workgroup differ by at least 3 standard deviations (Euclidean, over the 8 shifted channels) -- under
    every plan of every row (the stale buffer of a ring is the SAME workgroup's previous tile)"""
    seen = set()
    for rows, plan in ((RING_ROWS, plan_ring), (SPLIT_ROWS, plan_split), (ONEPASS_ROWS, plan_onepass), (GEMM_ROWS, plan_rows)):
        seen |= {(p['ntiles'], tuple(map(tuple, p['owned']))) for r in rows for p in [plan(r[0], r[1] > 1)]}
    seen |= {(p['ntiles'], tuple(map(tuple, p['owned']))) for r in ACC_ROWS for p in [plan_acc(r[0], False)]}
    seen |= {(p['ntiles'], tuple(map(tuple, p['owned']))) for r in XSPLIT128_ROWS for p in [plan_acc(r[0], True)]}
    for ntiles, owned in seen:
        off = tile_offsets(ntiles)
        for o in owned:
            o = np.array(o, int)
            if len(o) > 1:
                d = np.abs(off[o[1:]] - off[o[:-1]])
                assert (np.sqrt((d ** 2).sum(1)) >= 3.0).all(), (ntiles, o[:4], np.sqrt((d ** 2).sum(1)).min())


# ---- sensitivity: what the GPU rows are there to catch is far above their bounds ----------------------------------------------------
def _first_sample_rowslot(p, shape, slot):
    """`the table of the tile's first sample for every row of the tile`"""
    N, HW, C = nhwc(shape)
    T = p['T']
    return np.repeat(slot[(np.arange(p['ntiles']) * T) // HW], T)


def test_one_table_per_straddling_tile_is_far_outside_the_bound():
    shape, Kc = (256, 8, 8, 128), 3             # K6 on planes at C = 128, 128-row tiles over 64-row samples
    p = plan_acc(shape, True)
    d = k6_inputs(shape, Kc, p['T'])
    ref = k6_ref(d['gy'], d['x'], d['mu'], d['At'], d['S'], d['gm'], np.repeat(d['slot'], 64))
    wrong = k6_ref(d['gy'], d['x'], d['mu'], d['At'], d['S'], d['gm'], _first_sample_rowslot(p, shape, d['slot']))
    assert rel(wrong, ref) > 1e-2, rel(wrong, ref)
    shape = (58, 12, 12, 256)                   # K3 on planes, 32-row tiles over 144-row samples
    p = plan_split(shape, True)
    d = k3_inputs(shape, Kc, p['T'])
    ref = k3_ref(d['x'], d['mu'], d['A'], d['b'], np.repeat(d['slot'], 144))
    wrong = k3_ref(d['x'], d['mu'], d['A'], d['b'], _first_sample_rowslot(p, shape, d['slot']))
    assert rel(wrong, ref) > 1e-2, rel(wrong, ref)


def test_k3_ref_with_one_slot_per_sample_is_the_suites_reference():
    from test_fast_gpu import _ref_apply
    shape, Kc = (128, 4, 4, 256), 3
    d = k3_inputs(shape, Kc, 32)
    a = k3_ref(d['x'], d['mu'], d['A'], d['b'], np.repeat(d['slot'], 16))
    b = _ref_apply(d['x'], d['mu'], d['A'], d['b'], d['slot']).reshape(a.shape)
    assert rel(a, b) < 1e-13


def _stale(p, a):
    """a (M, C) with every tile but a workgroup's first replaced by the tile that workgroup held before it"""
    T = p['T']
    out = a.reshape(p['ntiles'], T, -1).copy()
    src = a.reshape(p['ntiles'], T, -1)
    for o in p['owned']:
        for prev, t in zip(o[:-1], o[1:]):
            out[t] = src[prev]
    return out.reshape(a.shape)


@pytest.mark.parametrize("kernel,shape,Kc", [(RING, (129, 16, 16, 256), 3), (SPLIT, (129, 16, 16, 256), 1), (ONE, (129, 8, 8, 256), 3),
                                             (ACC, (129, 16, 16, 256), 3)])
def test_a_tile_computed_from_the_previous_tiles_buffer_is_far_outside_the_bound(kernel, shape, Kc):
    """(rows_gemm_kernel has no such row: its workgroups hold one block each and carry nothing from block to block)"""
    N, HW, C = nhwc(shape)
    if kernel in (RING, SPLIT):
        p = (plan_ring if kernel == RING else plan_split)(shape, Kc > 1)
        d = k3_inputs(shape, Kc, p['T'])
        rs = np.repeat(d['slot'], HW)
        ref = k3_ref(d['x'], d['mu'], d['A'], d['b'], rs)
        wrong = k3_ref(_stale(p, d['x'].reshape(-1, C)), d['mu'], d['A'], d['b'], rs)
    else:
        p = plan_onepass(shape, Kc > 1) if kernel == ONE else plan_acc(shape, False)
        d = k6_inputs(shape, Kc, p['T'])
        rs = np.repeat(d['slot'], HW)
        ref = k6_ref(d['gy'], d['x'], d['mu'], d['At'], d['S'], d['gm'], rs)
        gy = _stale(p, d['gy'].reshape(-1, C)) if kernel == ONE else d['gy']        # the accumulating pass stages x alone
        wrong = k6_ref(gy, _stale(p, d['x'].reshape(-1, C)), d['mu'], d['At'], d['S'], d['gm'], rs)
    assert p['kernel'] == kernel
    assert rel(wrong, ref) > 1e-2, rel(wrong, ref)
