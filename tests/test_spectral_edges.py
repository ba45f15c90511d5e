"""The spectral-norm op's edges, the CPU half: the shape table of tests/spectral_reference.py against the restated
workgroup plan, the float32 precondition of every case of tests/test_spectral_edges_gpu.py, and the argument checks and
workspace layout of the wc_spectral_norm_* entries (no kernel is launched)."""
import ctypes
import os

import numpy as np
import pytest

import spectral_reference as S


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---- the plan and the shape table ------------------------------------------------------------------------------------------
def test_every_row_of_the_table_has_its_workgroup_count():
    assert [S.plan(*s) for s in S.SHAPES] == [n for _, n, _ in S.TABLE]


def test_the_rows_sit_on_the_plans_boundaries():
    """Each regime's last and first size, one element apart where the table says so."""
    assert S.plan(7, 585) == 1 and S.plan(7, 586) == 2                       # 4095 | 4102 elements
    assert S.plan(64, 64) == 1 and S.plan(64, 65) == 2                       # 4096 itself is one workgroup's
    assert S.plan(256, 512) == 32 and 256 * 512 == 32 * 4096                 # the last size of the 4096 form ...
    assert 257 * 511 > 32 * 4096 and -(-257 * 511 // 16384) == 9 and S.plan(257, 511) == 32      # ... and the clamp from below
    assert S.plan(512, 1024) == 32 and 512 * 1024 == 32 * 16384              # the clamp's last size
    assert S.plan(1024, 513) == 33 and 1024 * 513 - 32 * 16384 == 1024       # one column more than (1024, 512)
    assert S.plan(130, 16000) == 127 and S.plan(1040, 2001) == 128 and 1040 * 2001 - 127 * 16384 == 272
    assert S.plan(1300, 1601) == 128 and 1300 % 128 != 0 and S.plan(4096, 4096) == 128
    assert S.plan(1, 8192) == 1 and S.plan(3, 2000) == 2 and S.plan(3, 1 << 20) == 3       # never more than the rows
    assert S.lds_bytes(130, 16000) == 65560 and S.lds_bytes(20000, 3) == 81052           # the two rows behind the LDS opt-in
    assert sorted(s for s in S.SHAPES if S.lds_bytes(*s) > 48 * 1024) == [(130, 16000), (20000, 3)]
    assert max(r * k for r, k in S.SHAPES) == 1300 * 1601


def test_the_rows_reach_the_column_slice_forms():
    """t = W^T u: nc < 256 with row groups, nc == 256, nc > 256 (the c0 loop), empty and ragged slices."""
    def ncs(R, K):
        return [b - a for a, b in S.slices(K, S.plan(R, K))]
    assert ncs(1, 257) == [257] and ncs(1, 8192) == [8192] and ncs(3, 2000) == [1000, 1000]      # c0 loop: 2, 32, 4 passes
    assert ncs(64, 64) == [64] and 256 // 64 == 4                                                   # four row groups
    assert ncs(2, 50) == [50] and 256 // 50 == 5 > 2                                                # groups clamped to R
    assert ncs(4097, 1) == [0, 1] and ncs(20000, 3).count(0) == 12 and sum(ncs(20000, 3)) == 3
    assert set(ncs(100, 4133)) == {129, 130} and 256 // 129 == 1                                    # one row group, 126 idle threads
    assert sorted(set(ncs(33, 127))) == [63, 64] and [b - a for a, b in S.slices(33, 2)] == [16, 17]
    assert set(ncs(1300, 1601)) == {12, 13} and {b - a for a, b in S.slices(1300, 128)} == {10, 11}
    assert ncs(16, 256) == [256]                                                                    # every thread a column, no second pass


# ---- the float32 precondition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,family", S.CASES, ids=[f"{s[0]}x{s[1]}-{f}" for s, f in S.CASES])
def test_float32_model_is_a_quarter_of_the_bound_from_the_oracle(shape, family):
    """No case of the GPU file can fail on a correct float32 kernel: the op's formulas in NumPy float32 are within
    5e-6 of the float64 oracle in every measure the GPU test bounds by 2e-5."""
    c = S.case(*shape, family)
    for it in S.ITERATIONS:
        c.precondition(it)


def test_every_family_is_used_where_it_exists():
    assert len(S.CASES) == 90 and {f for _, f in S.CASES} == set(S.FAMILIES)
    for s in S.SHAPES:
        assert (s, "gauss") in S.CASES and (s, "tiny") in S.CASES
    assert [f for s, f in S.CASES if s == (1, 1)] == ["gauss", "tiny"]
    assert [f for s, f in S.CASES if s == (4097, 1)] == ["gauss", "rowscale", "tiny"]
    c = S.case(33, 127, "twin")
    sv = np.linalg.svd(c.W.astype(np.float64), compute_uv=False)
    assert np.allclose(sv[:3], [1.0, 0.999, 0.1], atol=1e-6)
    assert np.linalg.matrix_rank(S.case(33, 127, "rank1").W.astype(np.float64), tol=1e-5) == 1
    assert c.W.dtype == c.u0.dtype == c.v0.dtype == c.g.dtype == np.float32
    assert abs(np.linalg.norm(c.u0.astype(np.float64)) - 1) < 1e-6 and abs(np.linalg.norm(c.v0.astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("shape", S.EPS_SHAPES, ids=[f"{r}x{k}" for r, k in S.EPS_SHAPES])
def test_eps_cases_clamp_both_products_and_tell_the_shortcut_from_the_norm(shape):
    """eps = 1e-2 with the matrix scaled by 1e-4: |W^T u| and |W v| stay below eps in both iterations, so v = t / eps,
    u = s / eps, sigma = |s|^2 / eps; the float32 model holds the precondition, W / sigma stays finite in float32, and
    sigma taken as |s| (what it equals when nothing is clamped) would be off by the factor eps / |s| > 100."""
    c = S.eps_case(*shape)
    W = c.W.astype(np.float64)
    u, v = c.u0.astype(np.float64), c.v0.astype(np.float64)
    for it in (1, 2):
        t = W.T @ u
        assert np.linalg.norm(t) < c.eps / 10
        v = t / c.eps
        s = W @ v
        assert np.linalg.norm(s) < c.eps / 100
        u = s / c.eps
        w_o, s_o, u_o, v_o, _ = c.oracle(it)
        assert np.array_equal(v, v_o) and np.array_equal(u, u_o)
        assert abs(s_o - (s @ s) / c.eps) <= 1e-12 * s_o and np.linalg.norm(s) / s_o > 100
        assert np.abs(w_o).max() < 1e30 and s_o > 1e-30                   # float32: far from overflow and from denormals
        c.precondition(it)
        m = S.model_f32(c.W, c.u0, c.v0, it, c.eps)
        assert S.rel(m[2], u_o) < S.PRECONDITION and S.rel(m[3], v_o) < S.PRECONDITION     # u, v are not unit here: relative


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def _fwd(lib, R=4, K=4, it=1, eps=1e-12, ws_bytes=None, null=None, keep=True):
    one = ctypes.c_void_p(16)          # never dereferenced: every call here is rejected before a launch
    a = dict(W=one, u=one, v=one, w_sn=one, sigma=one, u_used=one if keep else None, v_used=one if keep else None, ws=one)
    if null:
        a[null] = None
    if ws_bytes is None:
        ws_bytes = lib.wc_spectral_norm_workspace_bytes(R, K)
    return lib.wc_spectral_norm_f32(a['W'], R, K, a['u'], a['v'], it, eps, a['w_sn'], a['sigma'], a['u_used'], a['v_used'],
                                    a['ws'], ws_bytes, None)


def _bwd(lib, R=4, K=4, ws_bytes=0, null=None, fd=1):
    one = ctypes.c_void_p(16)
    a = dict(g=one, w_sn=one, u=one, v=one, sigma=one, dW=one, ws=one)
    if null:
        a[null] = None
    return lib.wc_spectral_norm_bwd_f32(a['g'], a['w_sn'], a['u'], a['v'], a['sigma'], R, K, fd, a['dW'], a['ws'], ws_bytes, None)


NULL, SHAPE, WORKSPACE, ARG = -1, -2, -4, -5


def test_forward_entry_checks_its_arguments(lib):
    short = lambda R, K: lib.wc_spectral_norm_workspace_bytes(R, K) - 1
    for name in ("W", "u", "v", "w_sn", "sigma", "ws"):
        assert _fwd(lib, null=name) == NULL, name
    assert _fwd(lib, keep=False, ws_bytes=short(4, 4)) == WORKSPACE          # u_used / v_used may be NULL: it got past that check
    for R, K in ((0, 4), (4, 0), (-1, 4), (4, -1), (-3, -3)):
        assert _fwd(lib, R, K, ws_bytes=1 << 30) == SHAPE, (R, K)
    assert _fwd(lib, 1 << 14, (1 << 14) + 1, ws_bytes=1 << 30) == SHAPE       # rows * cols > 2^28
    assert _fwd(lib, 1 << 14, 1 << 14, ws_bytes=short(1 << 14, 1 << 14)) == WORKSPACE     # 2^28 itself is taken
    assert _fwd(lib, 1 << 16, 1 << 16, ws_bytes=1 << 30) == SHAPE             # (the product does not wrap in 32 bits)
    assert _fwd(lib, it=-1) == ARG and _fwd(lib, it=0, ws_bytes=short(4, 4)) == WORKSPACE
    assert _fwd(lib, eps=-1e-12) == ARG and _fwd(lib, eps=float("nan")) == ARG and _fwd(lib, eps=float("-inf")) == ARG
    assert _fwd(lib, eps=0.0, ws_bytes=short(4, 4)) == WORKSPACE              # eps = 0 is allowed
    for R, K in ((4, 4), (1, 1), (130, 16000), (1300, 1601)):
        assert _fwd(lib, R, K, ws_bytes=short(R, K)) == WORKSPACE and _fwd(lib, R, K, ws_bytes=0) == WORKSPACE
    # u and v live in LDS: 4 (R + K + 260) bytes, refused above 150 KB (R + K = 38140 is the last size taken)
    assert _fwd(lib, 1, 40000, ws_bytes=1 << 30) == SHAPE and _fwd(lib, 40000, 1, ws_bytes=1 << 30) == SHAPE
    assert _fwd(lib, 1, 38140, ws_bytes=1 << 30) == SHAPE and _fwd(lib, 1, 38139, ws_bytes=short(1, 38139)) == WORKSPACE
    assert _fwd(lib, 2, 38138, ws_bytes=short(2, 38138)) == WORKSPACE and _fwd(lib, 2, 38139, ws_bytes=1 << 30) == SHAPE


def test_backward_entry_checks_its_arguments(lib):
    for name in ("g", "w_sn", "u", "v", "sigma", "dW", "ws"):
        assert _bwd(lib, null=name, ws_bytes=1 << 30) == NULL, name
    for R, K in ((0, 4), (4, 0), (-1, 4), (4, -1)):
        assert _bwd(lib, R, K, ws_bytes=1 << 30) == SHAPE, (R, K)
    assert _bwd(lib, 1 << 14, (1 << 14) + 1, ws_bytes=1 << 30) == SHAPE
    assert _bwd(lib, 1 << 14, 1 << 14, ws_bytes=lib.wc_spectral_norm_workspace_bytes(1 << 14, 1 << 14) - 1) == WORKSPACE
    for fd in (0, 1):
        for R, K in ((4, 4), (1, 1), (1300, 1601)):
            assert _bwd(lib, R, K, ws_bytes=lib.wc_spectral_norm_workspace_bytes(R, K) - 1, fd=fd) == WORKSPACE
    # the backward keeps nothing in LDS: the forward's refusal is not its own (such a weight never had a forward, though)
    assert _bwd(lib, 1, 40000, ws_bytes=lib.wc_spectral_norm_workspace_bytes(1, 40000) - 1) == WORKSPACE


def _items(kind, n):
    """n items that pass every check (pointers that are never dereferenced, 4 x 4 matrices)."""
    from wc_gan_amd import _lib
    cls = _lib.SnItem if kind == "fwd" else _lib.SnBwdItem
    items = (cls * n)()
    for i in range(n):
        for name, typ in cls._fields_:
            setattr(items[i], name, 4 if typ is ctypes.c_int else 16)
    return items


def _items_with(kind, n, i, name, val):
    items = _items(kind, n)
    setattr(items[i], name, val)
    return items


def test_batched_entries_check_their_arguments(lib):
    fwd = lambda items, count, it=1, eps=1e-12: lib.wc_spectral_norm_batched_f32(
        ctypes.addressof(items) if items is not None else None, count, it, eps, None)
    bwd = lambda items, count, fd=1: lib.wc_spectral_norm_bwd_batched_f32(
        ctypes.addressof(items) if items is not None else None, count, fd, None)
    ok_f, ok_b = _items("fwd", 3), _items("bwd", 3)
    assert fwd(None, 3) == NULL and bwd(None, 3) == NULL
    for count in (0, -1):
        assert fwd(ok_f, count) == SHAPE and bwd(ok_b, count) == SHAPE
    assert fwd(ok_f, 3, it=-1) == ARG and fwd(ok_f, 3, eps=-1.0) == ARG and fwd(ok_f, 3, eps=float("nan")) == ARG
    for i in (0, 2):                      # the first and the last item: every item is looked at
        for name in ("W", "u", "v", "w_sn", "sigma", "ws"):
            assert fwd(_items_with("fwd", 3, i, name, None), 3) == NULL, (i, name)
        for name in ("g", "w_sn", "u", "v", "sigma", "dW", "ws"):
            assert bwd(_items_with("bwd", 3, i, name, None), 3) == NULL, (i, name)
        for kind, call in (("fwd", fwd), ("bwd", bwd)):
            assert call(_items_with(kind, 3, i, "rows", 0), 3) == SHAPE and call(_items_with(kind, 3, i, "cols", -2), 3) == SHAPE
            big = _items_with(kind, 3, i, "rows", 1 << 14); big[i].cols = (1 << 14) + 1
            assert call(big, 3) == SHAPE
        wide = _items_with("fwd", 3, i, "rows", 1); wide[i].cols = 40000
        assert fwd(wide, 3) == SHAPE                                            # the LDS refusal, per item


def test_workspace_layout_identities(lib):
    """bytes, the offset of the per-workgroup maxima and of the error word: t[K] | s[R] | partial[128] | amax[128] |
    padding to 16 | 16 bytes (error word first) | 16 bytes of meeting words."""
    Rs = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 128, 130, 257, 1024, 1300, 4097, 20000]
    for R in Rs:
        for K in Rs:
            b, a, e = (lib.wc_spectral_norm_workspace_bytes(R, K), lib.wc_spectral_norm_amax_offset(R, K),
                       lib.wc_spectral_norm_error_offset(R, K))
            assert e == b - 32 and a == 4 * (R + K + 128) and a + 512 <= e and b % 16 == 0, (R, K)
            assert e - (a + 512) < 16 and e % 16 == 0                            # nothing but the padding in between
    for R, K in ((0, 4), (4, 0), (-1, 4), (4, -1), (0, 0), (-5, -5)):
        assert (lib.wc_spectral_norm_workspace_bytes(R, K), lib.wc_spectral_norm_amax_offset(R, K),
                lib.wc_spectral_norm_error_offset(R, K)) == (0, 0, 0), (R, K)
