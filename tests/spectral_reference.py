"""What the spectral-norm edge tests share (not collected: no test_ prefix): the workgroup plan restated, the op's
formulas in NumPy float32, the matrix families, the warm start and the float64 oracle's results per case.

Nothing here imports the library: `plan` is written from the description of csrc/wc_sn.hip's host plan, so a change
there that moves a boundary shows up as a disagreement, and `model_f32` is the yardstick that says whether a case CAN
be held to the suite's 2e-5 in float32 at all (each case asserts it a factor four inside, at 5e-6, before the kernel
is looked at)."""
from __future__ import annotations

import functools
import zlib

import numpy as np

from oracle import wc_oracle as O

MAXWG = 128
BOUND = 2e-5                    # the project's own: relative for w_sn, sigma, dW; absolute for the unit vectors u, v
PRECONDITION = BOUND / 4        # the float32 model against the oracle, asserted for every case on the CPU
ITERATIONS = (0, 1, 3)

# (R, K), the workgroup count the plan gives it, the edge it is the smallest shape for
TABLE = [
    ((1, 1), 1, "minimum"),
    ((1, 7), 1, "single row"),
    ((1, 257), 1, "c0 loop, ragged second pass"),
    ((1, 8192), 1, "DCGAN head: R clamp, 32 passes of the c0 loop"),
    ((2, 50), 1, "row groups clamped to R"),
    ((7, 585), 1, "4095 elements"),
    ((7, 586), 2, "first two-workgroup size"),
    ((64, 64), 1, "nc < 256 with four row groups"),
    ((33, 127), 2, "nothing divides"),
    ((3, 2000), 2, "R clamp, nc = 1000 across workgroups"),
    ((4097, 1), 2, "one empty column slice"),
    ((20000, 3), 15, "twelve empty column slices; 81 KB of LDS"),
    ((256, 512), 32, "top of the 4096 form"),
    ((257, 511), 32, "first shape of the 16384 form, clamped to 32"),
    ((100, 4133), 32, "nc = 129..130: one row group"),
    ((512, 1024), 32, "last clamped"),
    ((1024, 513), 33, "16384 form just above the clamp"),
    ((130, 16000), 127, "65.5 KB of LDS: the opt-in"),
    ((1040, 2001), 128, "first 128"),
    ((1300, 1601), 128, "R not a multiple of 128"),
    ((16, 256), 1, "nc == 256: every thread a column, one pass, one row group"),
]
SHAPES = [s for s, _, _ in TABLE]
FAMILIES = ("gauss", "twin", "rank1", "rowscale", "tiny")


def plan(R, K):
    """Workgroups of one weight: ceil(RK / 4096) up to 32; past that ceil(RK / 16384), at least 32 and at most 128;
    never more than the rows; at least one."""
    n = -(-(R * K) // 4096)
    if n > 32:
        n = max(32, -(-(R * K) // 16384))
    return max(1, min(n, MAXWG, R))


def lds_bytes(R, K):
    """u and v, the four wave sums and the 256 partial column sums, as floats."""
    return 4 * (R + K + 4 + 256)


def slices(n, nwg):
    """The bounds n * b / nwg of the column (n = K) or row (n = R) slices."""
    return [(n * b // nwg, n * (b + 1) // nwg) for b in range(nwg)]


def family_exists(family, R, K):
    if family in ("gauss", "tiny"):
        return True
    if family == "rowscale":
        return R >= 2               # one row: a scalar multiple of gauss
    if family == "rank1":
        return R >= 2 and K >= 2    # one row or column: every matrix is rank one
    if family == "twin":
        return min(R, K) >= 3       # the three leading singular values 1, 0.999, 0.1
    raise ValueError(family)


CASES = [(s, f) for s in SHAPES for f in FAMILIES if family_exists(f, *s)]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def matrix(family, R, K, seed):
    """float32 (R, K).  gauss: N(0, 1) / sqrt(K); twin: orthonormal factors around the singular values 1, 0.999, 0.1,
    0.1 / 2, 0.1 / 3 ... (the power iteration is far from converged: u, v still move); rank1: a b^T; rowscale: gauss
    rows times exp(U(-4, 4)) (3.5 decades between rows); tiny: gauss * 1e-6."""
    rng = np.random.default_rng(seed)
    if family in ("gauss", "tiny", "rowscale"):
        W = rng.standard_normal((R, K)) / np.sqrt(K)
        if family == "tiny":
            W *= 1e-6
        if family == "rowscale":
            W *= np.exp(rng.uniform(-4.0, 4.0, (R, 1)))
    elif family == "rank1":
        W = np.outer(rng.standard_normal(R), rng.standard_normal(K)) / np.sqrt(K)
    elif family == "twin":
        r = min(R, K)
        U, _ = np.linalg.qr(rng.standard_normal((R, r)))
        V, _ = np.linalg.qr(rng.standard_normal((K, r)))
        sv = np.concatenate([[1.0, 0.999], 0.1 / np.arange(1, r - 1)])
        W = (U * sv) @ V.T
    else:
        raise ValueError(family)
    return np.ascontiguousarray(W, dtype=np.float32)


def warm_start(W, seed):
    """u, v after two float64 oracle iterations from a random unit start, rounded to float32: what an evaluation pass
    or a later training step finds in the layer's buffers (so sigma = u^T W v at iterations = 0 is a sum without
    cancellation, as in use)."""
    rng = np.random.default_rng(seed)
    R, K = W.shape
    u0 = rng.standard_normal(R); u0 /= np.linalg.norm(u0)
    v0 = rng.standard_normal(K); v0 /= np.linalg.norm(v0)
    _, _, u, v = O.spectral_normalize(W, u0, v0, 2)
    return u.astype(np.float32), v.astype(np.float32)


def gradient(R, K, seed):
    return np.random.default_rng(seed).standard_normal((R, K)).astype(np.float32)


def model_f32(W, u, v, iterations, eps=1e-12):
    """The op's formulas in float32 (sums in NumPy's order, not the kernel's): (w_sn, sigma, u, v)."""
    f = np.float32
    W = np.asarray(W, f); u = np.asarray(u, f).copy(); v = np.asarray(v, f).copy(); eps = f(eps)
    sigma = None
    for _ in range(int(iterations)):
        t = W.T @ u
        v = t * (f(1) / max(np.sqrt(np.dot(t, t)), eps))
        s = W @ v
        n2 = np.dot(s, s)
        inv_u = f(1) / max(np.sqrt(n2), eps)
        u = s * inv_u
        sigma = n2 * inv_u                      # u^T (W v) with u = (W v) / max(|W v|, eps)
    if sigma is None:
        sigma = np.dot(u, W @ v)
    return W * (f(1) / f(sigma)), f(sigma), u, v


def model_bwd_f32(g, w_sn, u, v, sigma, fully_diff):
    f = np.float32
    c = np.dot(np.asarray(g, f).reshape(-1), np.asarray(w_sn, f).reshape(-1)) if fully_diff else f(0)
    return (np.asarray(g, f) - c * np.outer(u, v).astype(f)) * (f(1) / f(sigma))


def rel(a, b, floor=0.0):
    """max |a - b| over max |b|; `floor` stands in for a reference that is zero throughout."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    den = float(np.abs(b).max())
    return float(np.abs(a - b).max() / (den if den > 0.0 else floor))


def absd(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def forward_errors(got, ref):
    """got, ref: (w_sn, sigma, u, v).  The project's measures: relative to the largest entry for w_sn, relative for
    sigma, absolute for u and v."""
    return dict(w_sn=rel(got[0], ref[0]), sigma=abs(float(got[1]) - float(ref[1])) / abs(float(ref[1])),
                u=absd(got[2], ref[2]), v=absd(got[3], ref[3]))


class Case:
    """One matrix with its warm start and gradient (float32), and per iteration count the float64 oracle's forward and
    both backwards, computed on first use."""

    def __init__(self, R, K, family, eps=1e-12, scale=None):
        self.R, self.K, self.family, self.eps = R, K, family, eps
        self.W = matrix(family, R, K, _seed(R, K, family, "W"))
        self.u0, self.v0 = warm_start(self.W, _seed(R, K, family, "uv"))
        if scale is not None:                   # (the eps cases: the warm start is the unscaled matrix's)
            self.W = (self.W * np.float32(scale)).astype(np.float32)
        self.g = gradient(R, K, _seed(R, K, family, "g"))
        self._ref = {}

    def oracle(self, iterations):
        """(w_sn, sigma, u, v, {fully_diff: dW}) in float64 from the float32 inputs."""
        if iterations not in self._ref:
            w, s, u, v = O.spectral_normalize(self.W, self.u0, self.v0, iterations, self.eps)
            d = {fd: O.spectral_normalize_backward(self.g, w, u, v, s, fd) for fd in (True, False)}
            self._ref[iterations] = (w, s, u, v, d)
        return self._ref[iterations]

    def dw_error(self, dW, iterations, fully_diff):
        """Relative to the largest entry of the oracle's dW.  For a 1 x 1 weight the fully differentiable gradient is
        zero throughout (w_sn = +-1 whatever W is: g and c u v^T cancel), so there the scale is that of the two terms
        that cancel, |g| / sigma."""
        w, s, u, v, d = self.oracle(iterations)
        return rel(dW, d[fully_diff], floor=float(np.abs(self.g).max() / abs(s)))

    def model_errors(self, iterations):
        """The float32 model against the oracle: the forward's four measures and dW for both fully_diff values."""
        w, s, u, v, d = self.oracle(iterations)
        m = model_f32(self.W, self.u0, self.v0, iterations, self.eps)
        e = forward_errors(m, (w, s, u, v))
        for fd in (True, False):
            e["dW_full" if fd else "dW_const"] = self.dw_error(model_bwd_f32(self.g, m[0], m[2], m[3], m[1], fd), iterations, fd)
        return e

    def precondition(self, iterations):
        """A case the float32 formulas themselves cannot hold a factor four inside the bound is re-chosen, never
        loosened; returns the model's errors."""
        e = self.model_errors(iterations)
        bad = {k: x for k, x in e.items() if not x <= PRECONDITION}
        assert not bad, f"({self.R}, {self.K}) {self.family} it={iterations}: the float32 model is off by {bad}"
        return e


@functools.lru_cache(maxsize=3)
def case(R, K, family):
    return Case(R, K, family)


EPS_CLAMP = 1e-2
EPS_SCALE = 1e-4                # both products of a gauss matrix * 1e-4 stay below eps = 1e-2 from unit u
EPS_SHAPES = [(1, 257), (33, 127), (64, 64), (1024, 513)]


@functools.lru_cache(maxsize=2)
def eps_case(R, K):
    return Case(R, K, "gauss", eps=EPS_CLAMP, scale=EPS_SCALE)
