"""The narrow (image-layer) convolution kernels of csrc/wc_conv.hip -- conv_fwd_narrow_kernel<2|5|10|14|16>, conv_fwd_narrow_split_kernel,
conv_wrw_narrow_kernel, conv_wrw_narrow_masked_kernel, conv_wrw_narrow_reduce_kernel -- for tests/test_narrow_edges.py (no GPU) and
tests/test_narrow_edges_gpu.py (not collected: no test_ prefix):

  * the host plan, restated ONLY to label rows (plan): which forward instantiation, how many 32-pixel tiles, tiles per wave and
    workgroups; pixels per wave, partials and channel groups of the weight gradient; the reduce kernel's trips;
  * the multiply-shift division of the kernels' pixel index (magic_u31, mulshift);
  * NumPy float64 direct sums in the kernels' own terms, A[p][m] with m = tap * Cin + c and row nrow = 1: forward (+ ReLU), the
    mirrored forward (the data gradient of an F -> Cout layer), weight and bias gradient, the exchanged weight gradient, the masked
    weight gradient with threshold_backward's predicate;
  * the row table: every row states its class as literals, and tests/test_narrow_edges.py holds them to the restated plan and the
    restated plan to the library's predicates and workspace sizes.

Inputs are float32 draws of a generator seeded by the row's name; the references are computed from those float32 values in float64."""
import zlib
from functools import lru_cache

import numpy as np

Y_BOUND = 1e-5          # y and the mirrored data gradient: max |error| over max |reference| (tests/test_conv_gpu.py's _rel)
DW_BOUND = 2e-6         # dW and db (test_narrow_input_weight_gradient_against_float64's bounds)
SPLIT_BLOCKS = 512      # kAmaxBlocks: the split variant's grid owns at least one pair of the reader's record per workgroup


# ---- the multiply-shift division ---------------------------------------------------------------------------------------------------
def magic_u31(d):
    """magic_u31 of csrc/wc_conv.hip: (mag, sh) with umulhi(m, mag) >> sh == m / d for m < 2^31 and d >= 2 (32-bit unsigned words)"""
    s = 0
    while (1 << s) < d:
        s += 1
    mag = (((1 << (31 + s)) + d - 1) // d) & 0xFFFFFFFF
    return mag, (s - 1) & 0xFFFFFFFF


def mulshift(m, mag, sh):
    """the device's quotient: __umulhi(m, mag) >> sh -- a 32-bit shift takes the low five bits of its count"""
    return ((m * mag) >> 32) >> (sh & 31)


# ---- the host plan -----------------------------------------------------------------------------------------------------------------
def reduce_trips(nparts):
    """conv_wrw_narrow_reduce_kernel: (16-deep unrolled trips, single tail trips) summed over the eight partial groups of a workgroup"""
    unrolled = tail = 0
    for pg in range(8):
        z = pg
        while z + 8 * 15 < nparts:
            unrolled, z = unrolled + 1, z + 8 * 16
        while z < nparts:
            tail, z = tail + 1, z + 8
    return unrolled, tail


def plan(N, H, W, Cin, Cout, k):
    """narrow_fwd_args, wc_conv_fwd_narrow_f32's dispatch and narrow_wrw_parts, restated"""
    nrow = k * k * Cin
    ks2 = (nrow + 2) // 2
    inst = 2 if ks2 <= 2 else 5 if ks2 <= 5 else 10 if ks2 <= 10 else 14 if ks2 <= 14 else 16
    M = N * H * W
    ntiles = (M + 31) // 32
    tpw = max(1, (ntiles + 1023) // 1024)
    grid = ((ntiles + 4 * tpw - 1) // (4 * tpw), Cout // 64)
    ppw = max(16, (M + 2047) // 2048)
    ppw += ppw & 1
    nparts = (M + 8 * ppw - 1) // (8 * ppw)
    return dict(nrow=nrow, inst=inst, ntiles=ntiles, tpw=tpw, grid=grid, ppw=ppw, nparts=nparts, ngrp=(Cout + 127) // 128,
                reduce=reduce_trips(nparts))


def supported(N, H, W, Cin, Cout, k):
    """wc_conv_narrow64_supported, restated"""
    return (min(N, H, Cin, Cout) > 0 and W >= 2 and k in (1, 3) and k * k * Cin < 32 and Cout % 64 == 0 and N * H * W < 2 ** 31)


def split_supported(N, H, W, Cin, Cout, k):
    """wc_conv_fwd_narrow_split_supported, restated: not monotone in M, because tiles_per_wave jumps"""
    if not supported(N, H, W, Cin, Cout, k) or N * H * W * Cin >= 2 ** 31:
        return False
    g = plan(N, H, W, Cin, Cout, k)['grid']
    return g[0] * g[1] <= SPLIT_BLOCKS


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
class Row:
    """One layer shape: x (N, H, W, Cin) NHWC, w (Cout, Cin, k, k).  The class literals: nrow = k*k*Cin (the bias row's index), inst (the
    forward's KS), ntiles, tpw (tiles per wave), grid (workgroups, 64-channel columns), ppw (pixels per wave of the weight gradient),
    nparts, ngrp (128-channel groups), reduce (unrolled, tail trips).  fmt: the weight's memory format; bias: present?; split: does the
    split variant take the shape (gate rows only)."""

    def __init__(self, name, shape, Cin, Cout, k, nrow, inst, ntiles, tpw, grid, ppw, nparts, ngrp, reduce, fmt='channels_last', bias=True,
                 tags=(), split=None):
        self.name, self.shape, self.Cin, self.Cout, self.k = name, shape, Cin, Cout, k
        self.nrow, self.inst, self.ntiles, self.tpw, self.grid = nrow, inst, ntiles, tpw, grid
        self.ppw, self.nparts, self.ngrp, self.reduce = ppw, nparts, ngrp, reduce
        self.fmt, self.bias, self.tags, self.split = fmt, bias, tags, split

    @property
    def M(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def geom(self):
        return self.shape + (self.Cin, self.Cout, self.k)

    def literals(self):
        return {n: getattr(self, n) for n in ('nrow', 'inst', 'ntiles', 'tpw', 'grid', 'ppw', 'nparts', 'ngrp', 'reduce')}

    def label(self):
        return (f"<{self.inst}> nrow {self.nrow} tiles {self.ntiles} tpw {self.tpw} grid {self.grid[0]}x{self.grid[1]} ppw {self.ppw} "
                f"parts {self.nparts} grp {self.ngrp} reduce {self.reduce[0]}+{self.reduce[1]}")

    def __repr__(self):
        return self.name


ROWS = [
    # every k-step class and both sides of every gate (nrow 3|4, 9|10, 19|20, 27|28), the full table (nrow 31: the bias row is row 31),
    # the bias row in the last tap's k-step (odd nrow) and in a k-step of its own (even nrow): M = 70, two full tiles and a partial one
    Row('k1-c1', (2, 5, 7), 1, 64, 1, nrow=1, inst=2, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c2', (2, 5, 7), 2, 64, 1, nrow=2, inst=2, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c3', (2, 5, 7), 3, 64, 1, nrow=3, inst=2, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c4', (2, 5, 7), 4, 64, 1, nrow=4, inst=5, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c9', (2, 5, 7), 9, 64, 1, nrow=9, inst=5, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c10', (2, 5, 7), 10, 64, 1, nrow=10, inst=10, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c19', (2, 5, 7), 19, 64, 1, nrow=19, inst=10, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c20', (2, 5, 7), 20, 64, 1, nrow=20, inst=14, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c27', (2, 5, 7), 27, 64, 1, nrow=27, inst=14, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c28', (2, 5, 7), 28, 64, 1, nrow=28, inst=16, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k1-c31', (2, 5, 7), 31, 64, 1, nrow=31, inst=16, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k3-c1', (2, 5, 7), 1, 64, 3, nrow=9, inst=5, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k3-c2', (2, 5, 7), 2, 64, 3, nrow=18, inst=10, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    Row('k3-c3', (2, 5, 7), 3, 64, 3, nrow=27, inst=14, ntiles=3, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('kstep',)),
    # the channel groups: one, one and a half (the last group's upper half has no channels) and two groups of 128
    Row('k3-c3-o128', (2, 5, 7), 3, 128, 3, nrow=27, inst=14, ntiles=3, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('group',)),
    Row('k1-c31-o128', (2, 5, 7), 31, 128, 1, nrow=31, inst=16, ntiles=3, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('group',)),
    Row('k3-c3-o192', (2, 5, 7), 3, 192, 3, nrow=27, inst=14, ntiles=3, tpw=1, grid=(1, 3), ppw=16, nparts=1, ngrp=2, reduce=(0, 1), tags=('group', 'o192')),
    Row('k1-c31-o192', (2, 5, 7), 31, 192, 1, nrow=31, inst=16, ntiles=3, tpw=1, grid=(1, 3), ppw=16, nparts=1, ngrp=2, reduce=(0, 1), tags=('group', 'o192')),
    Row('k3-c3-o256', (2, 5, 7), 3, 256, 3, nrow=27, inst=14, ntiles=3, tpw=1, grid=(1, 4), ppw=16, nparts=1, ngrp=2, reduce=(0, 1), tags=('group',)),
    Row('k1-c31-o256', (2, 5, 7), 31, 256, 1, nrow=31, inst=16, ntiles=3, tpw=1, grid=(1, 4), ppw=16, nparts=1, ngrp=2, reduce=(0, 1), tags=('group',)),
    # the pixel edges.  M2: the smallest accepted shape, three idle waves; M31: one partial tile; M33 / M129: M = +1 (mod 32), odd M (the
    # second lane half's pixel is past the range's end); nparts 1, 2, 8 | 9, 120 | 121 (the reduce kernel's unrolled loop is entered),
    # 128 | 129, 256; M32800: ntiles 1025, two tiles per wave, the ppw = 16 floor lifted
    Row('M2', (1, 1, 2), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('pixel', 'partial')),
    Row('M31', (1, 1, 31), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('pixel', 'partial')),
    Row('M33', (1, 3, 11), 3, 64, 3, nrow=27, inst=14, ntiles=2, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('pixel', 'partial')),
    Row('M128', (2, 8, 8), 3, 64, 3, nrow=27, inst=14, ntiles=4, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('pixel',)),
    Row('M129', (1, 3, 43), 3, 64, 3, nrow=27, inst=14, ntiles=5, tpw=1, grid=(2, 1), ppw=16, nparts=2, ngrp=1, reduce=(0, 2), tags=('pixel', 'partial')),
    Row('M1024', (1, 32, 32), 3, 64, 3, nrow=27, inst=14, ntiles=32, tpw=1, grid=(8, 1), ppw=16, nparts=8, ngrp=1, reduce=(0, 8), tags=('pixel',)),
    Row('M1152', (2, 24, 24), 3, 64, 3, nrow=27, inst=14, ntiles=36, tpw=1, grid=(9, 1), ppw=16, nparts=9, ngrp=1, reduce=(0, 9), tags=('pixel',)),
    Row('M15360', (1, 120, 128), 3, 64, 3, nrow=27, inst=14, ntiles=480, tpw=1, grid=(120, 1), ppw=16, nparts=120, ngrp=1, reduce=(0, 120), tags=('pixel',)),
    Row('M15488', (1, 121, 128), 3, 64, 3, nrow=27, inst=14, ntiles=484, tpw=1, grid=(121, 1), ppw=16, nparts=121, ngrp=1, reduce=(1, 105), tags=('pixel',)),
    Row('M16384', (4, 64, 64), 3, 64, 3, nrow=27, inst=14, ntiles=512, tpw=1, grid=(128, 1), ppw=16, nparts=128, ngrp=1, reduce=(8, 0), tags=('pixel',)),
    Row('M16512', (1, 129, 128), 3, 64, 3, nrow=27, inst=14, ntiles=516, tpw=1, grid=(129, 1), ppw=16, nparts=129, ngrp=1, reduce=(8, 1), tags=('pixel',)),
    Row('M32768', (8, 64, 64), 3, 64, 3, nrow=27, inst=14, ntiles=1024, tpw=1, grid=(256, 1), ppw=16, nparts=256, ngrp=1, reduce=(16, 0), tags=('pixel',)),
    Row('M32800', (1, 164, 200), 3, 64, 3, nrow=27, inst=14, ntiles=1025, tpw=2, grid=(129, 1), ppw=18, nparts=228, ngrp=1, reduce=(8, 100), tags=('pixel',)),
    Row('M33-o192', (1, 3, 11), 3, 192, 3, nrow=27, inst=14, ntiles=2, tpw=1, grid=(1, 3), ppw=16, nparts=1, ngrp=2, reduce=(0, 1), tags=('pixel', 'o192')),
    Row('M16385-o192', (5, 29, 113), 3, 192, 3, nrow=27, inst=14, ntiles=513, tpw=1, grid=(129, 3), ppw=16, nparts=129, ngrp=2, reduce=(8, 1), tags=('pixel', 'o192')),
    # other shapes: H != W, W no power of two, H = 1; the weight in both memory formats; without a bias (1x1, 128 outputs)
    Row('3x6x10', (3, 6, 10), 3, 64, 3, nrow=27, inst=14, ntiles=6, tpw=1, grid=(2, 1), ppw=16, nparts=2, ngrp=1, reduce=(0, 2), tags=('shape',)),
    Row('3x6x10-contiguous', (3, 6, 10), 3, 64, 3, nrow=27, inst=14, ntiles=6, tpw=1, grid=(2, 1), ppw=16, nparts=2, ngrp=1, reduce=(0, 2), fmt='contiguous', tags=('shape',)),
    Row('3x6x10-nobias', (3, 6, 10), 3, 128, 1, nrow=3, inst=2, ntiles=6, tpw=1, grid=(2, 2), ppw=16, nparts=2, ngrp=1, reduce=(0, 2), bias=False, tags=('shape',)),
    Row('2x7x7', (2, 7, 7), 3, 64, 3, nrow=27, inst=14, ntiles=4, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('shape',)),
    Row('2x7x7-contiguous', (2, 7, 7), 3, 64, 3, nrow=27, inst=14, ntiles=4, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), fmt='contiguous', tags=('shape',)),
    Row('2x7x7-nobias', (2, 7, 7), 3, 128, 1, nrow=3, inst=2, ntiles=4, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), bias=False, tags=('shape',)),
    Row('2x14x28', (2, 14, 28), 3, 64, 3, nrow=27, inst=14, ntiles=25, tpw=1, grid=(7, 1), ppw=16, nparts=7, ngrp=1, reduce=(0, 7), tags=('shape',)),
    Row('2x14x28-contiguous', (2, 14, 28), 3, 64, 3, nrow=27, inst=14, ntiles=25, tpw=1, grid=(7, 1), ppw=16, nparts=7, ngrp=1, reduce=(0, 7), fmt='contiguous', tags=('shape',)),
    Row('2x14x28-nobias', (2, 14, 28), 3, 128, 1, nrow=3, inst=2, ntiles=25, tpw=1, grid=(7, 2), ppw=16, nparts=7, ngrp=1, reduce=(0, 7), bias=False, tags=('shape',)),
    Row('4x2x3', (4, 2, 3), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('shape',)),
    Row('4x2x3-contiguous', (4, 2, 3), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), fmt='contiguous', tags=('shape',)),
    Row('4x2x3-nobias', (4, 2, 3), 3, 128, 1, nrow=3, inst=2, ntiles=1, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), bias=False, tags=('shape',)),
    Row('3x1x9', (3, 1, 9), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), tags=('shape',)),
    Row('3x1x9-contiguous', (3, 1, 9), 3, 64, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 1), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), fmt='contiguous', tags=('shape',)),
    Row('3x1x9-nobias', (3, 1, 9), 3, 128, 1, nrow=3, inst=2, ntiles=1, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1), bias=False, tags=('shape',)),
]

# The mirrored forward and the exchanged weight gradient of a layer F -> Cout in (1, 3) (the generator's last layer): in the kernels' terms
# Cin := the layer's Cout and Cout := F.  The mirrored forward takes F in 64s, the exchanged gradient's entry (wc_conv_wrw_narrow_f32) in 128s.
MIRROR_ROWS = [
    Row('3x6x10-c3-F64', (3, 6, 10), 3, 64, 3, nrow=27, inst=14, ntiles=6, tpw=1, grid=(2, 1), ppw=16, nparts=2, ngrp=1, reduce=(0, 2)),
    Row('2x7x7-c1-F128', (2, 7, 7), 1, 128, 3, nrow=9, inst=5, ntiles=4, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1)),
    Row('2x14x28-c3-F192', (2, 14, 28), 3, 192, 3, nrow=27, inst=14, ntiles=25, tpw=1, grid=(7, 3), ppw=16, nparts=7, ngrp=2, reduce=(0, 7)),
    Row('4x2x3-c1-F256', (4, 2, 3), 1, 256, 3, nrow=9, inst=5, ntiles=1, tpw=1, grid=(1, 4), ppw=16, nparts=1, ngrp=2, reduce=(0, 1)),
    Row('1x1x31-c3-F128', (1, 1, 31), 3, 128, 3, nrow=27, inst=14, ntiles=1, tpw=1, grid=(1, 2), ppw=16, nparts=1, ngrp=1, reduce=(0, 1)),
    Row('3x6x10-c3-F256', (3, 6, 10), 3, 256, 3, nrow=27, inst=14, ntiles=6, tpw=1, grid=(2, 4), ppw=16, nparts=2, ngrp=2, reduce=(0, 2)),
]

# The split variant's gate, grid <= 512 workgroups: at 128 outputs every M passes (ntiles 1024: 256 x 2 = 512; ntiles 1025: two tiles per
# wave, 129 x 2); at 192 outputs M = 21760 is the largest accepted with one tile per wave (170 x 3 = 510; 171 x 3 = 513), everything up
# to ntiles 1024 is declined, and two tiles per wave are accepted again up to M = 43520.
GATE_ROWS = [
    Row('M32768-o128', (8, 64, 64), 3, 128, 3, nrow=27, inst=14, ntiles=1024, tpw=1, grid=(256, 2), ppw=16, nparts=256, ngrp=1, reduce=(16, 0), split=True),
    Row('M32769-o128', (9, 11, 331), 3, 128, 3, nrow=27, inst=14, ntiles=1025, tpw=2, grid=(129, 2), ppw=18, nparts=228, ngrp=1, reduce=(8, 100), split=True),
    Row('M21760-o192', (1, 136, 160), 3, 192, 3, nrow=27, inst=14, ntiles=680, tpw=1, grid=(170, 3), ppw=16, nparts=170, ngrp=2, reduce=(8, 42), split=True),
    Row('M21761-o192', (1, 47, 463), 3, 192, 3, nrow=27, inst=14, ntiles=681, tpw=1, grid=(171, 3), ppw=16, nparts=171, ngrp=2, reduce=(8, 43), split=False),
    Row('M32768-o192', (8, 64, 64), 3, 192, 3, nrow=27, inst=14, ntiles=1024, tpw=1, grid=(256, 3), ppw=16, nparts=256, ngrp=2, reduce=(16, 0), split=False),
    Row('M32769-o192', (9, 11, 331), 3, 192, 3, nrow=27, inst=14, ntiles=1025, tpw=2, grid=(129, 3), ppw=18, nparts=228, ngrp=2, reduce=(8, 100), split=True),
    Row('M43520-o192', (2, 136, 160), 3, 192, 3, nrow=27, inst=14, ntiles=1360, tpw=2, grid=(170, 3), ppw=22, nparts=248, ngrp=2, reduce=(8, 120), split=True),
    Row('M43521-o192', (3, 89, 163), 3, 192, 3, nrow=27, inst=14, ntiles=1361, tpw=2, grid=(171, 3), ppw=22, nparts=248, ngrp=2, reduce=(8, 120), split=False),
]

# declined by every narrow predicate: a one-pixel-wide image (the multiply-shift division wants divisors >= 2)
W1_GEOMS = [(2, 5, 1, 3, 64, 3), (2, 5, 1, 3, 128, 3), (1, 1, 1, 3, 128, 1), (128, 32, 1, 1, 128, 3), (4, 1, 1, 31, 256, 1)]

ALL_ROWS = ROWS + MIRROR_ROWS + GATE_ROWS
SMALL_ROWS = [r for r in ROWS if r.M <= 1152]           # the rows a CPU float64 convolution with autograd takes in milliseconds


def tagged(tag, rows=None):
    return [r for r in (ROWS if rows is None else rows) if tag in r.tags]


def by_name(name):
    return next(r for r in ALL_ROWS if r.name == name)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(row):
    """float32 x (N, H, W, Cin), w (Cout, Cin, k, k), b (Cout,) | None, gy (N, H, W, Cout), h (gy's shape: a ReLU's pre-activations with
    +0, -0 and NaN among them).  The bias is 0.5-sigma: a dropped bias row is far above the bounds."""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    N, H, W = row.shape
    x = (rng.standard_normal((N, H, W, row.Cin)) * 0.7 + 0.1).astype(np.float32)
    w = (rng.standard_normal((row.Cout, row.Cin, row.k, row.k)) / np.sqrt(row.nrow)).astype(np.float32)
    b = (rng.standard_normal(row.Cout) * 0.5).astype(np.float32) if row.bias else None
    gy = rng.standard_normal((N, H, W, row.Cout)).astype(np.float32)
    h = rng.standard_normal((N, H, W, row.Cout)).astype(np.float32)
    flat = h.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = np.nan
    return x, w, b, gy, h


# ---- float64 direct sums -----------------------------------------------------------------------------------------------------------
def patches(x, k):
    """A[p][m] of the kernels: p = (n, y, x) row-major, m = tap * C + c with tap = r * k + s reading pixel (y + r - k/2, x + s - k/2)
    (zero outside the image); column k*k*C is the constant 1 (the bias row)."""
    x = np.asarray(x, np.float64)
    N, H, W, C = x.shape
    A = np.zeros((N, H, W, k * k * C + 1))
    for r in range(k):
        for s in range(k):
            dy, dx = r - k // 2, s - k // 2
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                A[:, y0:y1, x0:x1, (r * k + s) * C:(r * k + s + 1) * C] = x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx, :]
    A[..., -1] = 1.0
    return A.reshape(N * H * W, k * k * C + 1)


def weight_rows(w, b=None, mirrored=False):
    """Wm[m][o] = w[o][c][r][s] and row k*k*C = b (0 without one).  mirrored: w is (C, O, k, k) of the transposed map, its taps read
    back to front: Wm[m][o] = w[c][o][k-1-r][k-1-s]."""
    w = np.asarray(w, np.float64)
    if mirrored:
        w = w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    O, C, k, _ = w.shape
    Wm = np.zeros((k * k * C + 1, O))
    Wm[:-1] = w.transpose(2, 3, 1, 0).reshape(k * k * C, O)
    if b is not None:
        Wm[-1] = np.asarray(b, np.float64)
    return Wm


def forward(x, w, b=None, relu=False, mirrored=False):
    k = w.shape[2]
    y = patches(x, k) @ weight_rows(w, b, mirrored)
    if relu:
        y = np.maximum(y, 0.0)
    return y.reshape(x.shape[:3] + (y.shape[1],))


def mirrored_forward(gy, w):
    """the data gradient of the 'same' convolution x (.., F) -> y (.., C) with w (C, F, k, k), from gy (.., C)"""
    return forward(gy, w, None, mirrored=True)


def product_rows(x, gy, k, pixels=None):
    """D[m][o] = sum_p A[p][m] gy[p][o] over all pixels (or the index array `pixels`)"""
    A = patches(x, k)
    G = np.asarray(gy, np.float64).reshape(A.shape[0], -1)
    if pixels is not None:
        A, G = A[pixels], G[pixels]
    return A.T @ G


def gradients_of(D, C, k):
    """-> dW (O, C, k, k), db (O,) from the product's rows"""
    O = D.shape[1]
    return D[:-1].reshape(k, k, C, O).transpose(3, 2, 0, 1).copy(), D[-1].copy()


def gradients(x, gy, k, mask=None):
    """dW, db of the 'same' convolution from its output gradient; mask: gy is read through threshold_backward(gy, mask, 0) --
    zero where mask <= 0, the gradient where mask > 0 or mask is NaN"""
    g = np.asarray(gy, np.float64)
    if mask is not None:
        g = np.where(np.asarray(mask) <= 0, 0.0, g)
    return gradients_of(product_rows(x, g, k), x.shape[3], k)


def exchanged_gradient(x, gy, k):
    """dW (C, F, k, k) of the layer x (.., F) -> y (.., C) as the kernel computes it: the narrow-input gradient of a convolution that
    reads gy and whose output gradient is x, the taps mirrored"""
    dwt, _ = gradients_of(product_rows(gy, x, k), gy.shape[3], k)       # (F, C, k, k)
    return dwt.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1].copy()


@lru_cache(maxsize=None)
def reference(name):
    """float64 (y, y with ReLU, dW, db, masked dW, masked db) of a row of ROWS or GATE_ROWS, computed once"""
    row = by_name(name)
    x, w, b, gy, h = inputs(row)
    dw, db = gradients(x, gy, row.k)
    mdw, mdb = gradients(x, gy, row.k, mask=h)
    out = dict(y=forward(x, w, b), relu=forward(x, w, b, relu=True), dw=dw, db=db, mdw=mdw, mdb=mdb)
    for v in out.values():
        v.setflags(write=False)
    return out


def mirror_inputs(row):
    """the layer F -> C of a row of MIRROR_ROWS: x (N, H, W, F), w (C, F, 3, 3), gy (N, H, W, C), float32"""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    N, H, W = row.shape
    C, F = row.Cin, row.Cout
    x = (rng.standard_normal((N, H, W, F)) * 0.8).astype(np.float32)
    w = (rng.standard_normal((C, F, row.k, row.k)) / np.sqrt(F * row.k * row.k)).astype(np.float32)
    gy = rng.standard_normal((N, H, W, C)).astype(np.float32)
    return x, w, gy


@lru_cache(maxsize=None)
def mirror_reference(name):
    row = by_name(name)
    x, w, gy = mirror_inputs(row)
    out = dict(dx=mirrored_forward(gy, w), dw=exchanged_gradient(x, gy, row.k))
    for v in out.values():
        v.setflags(write=False)
    return out


def rel(a, r):
    """max |a - r| over max |r|"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float(np.abs(a - r).max() / np.abs(r).max())
