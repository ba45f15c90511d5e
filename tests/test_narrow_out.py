"""CPU tests of the narrow-output convolution's host side (csrc/wc_conv.hip wc_conv_narrow_out_supported / wc_conv_narrow_out_f32) and of
its float64 reference (tests/narrow_out_reference.py): which shapes the predicate takes, the codes the entry returns without a device,
the reference against torch's float64 autograd, and that the reference tells the kernel's possible faults apart on the GPU rows.
No kernel is launched (the library loads without a device).  DESIGN.md section 4.23."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import narrow_out_reference as R

WC_ERR_NULL, WC_ERR_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from wc_gan_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------
def test_every_recipe_grid_is_taken(lib):
    for hw in R.RECIPE_GRIDS:
        for cw in R.RECIPE_WIDTHS:
            for cn in (3, 1):
                for k in (3, 1):
                    for n in (1, 64, 128):
                        assert lib.wc_conv_narrow_out_supported(n, hw, hw, cw, cn, k) == 1, (n, hw, cw, cn, k)


def test_every_row_is_taken_and_the_widest_row_is_the_widest(lib):
    from wc_gan_amd import conv as C
    for r in R.ROWS:
        assert lib.wc_conv_narrow_out_supported(r.N, r.H, r.W, r.Cw, r.Cn, r.k) == 1, r
        assert C.narrow_out_supported((r.N, r.H, r.W, r.Cw), (r.Cw, r.Cn, r.k, r.k))
        assert C.narrow_out_supported((r.N, r.H, r.W, r.Cw), (r.Cn, r.Cw, r.k, r.k), forward=True)
    w = R.WIDEST
    assert lib.wc_conv_narrow_out_supported(w.N, w.H, w.W + 1, w.Cw, w.Cn, w.k) == 0        # the LDS band: three rows of Z no longer fit
    assert lib.wc_conv_narrow_out_supported(w.N, w.H, 4 * w.W, w.Cw, w.Cn, 1) == 1          # (no halo at 1x1: one row)


@pytest.mark.parametrize("shape", [(2, 4, 1, 64, 3, 3),        # W = 1: the multiply-shift division
                                   (2, 4, 4, 64, 3, 2),        # ksize = 2
                                   (2, 4, 4, 64, 4, 3),        # ksize^2 * Cn = 36
                                   (2, 4, 4, 64, 32, 1),       # ksize^2 * Cn = 32
                                   (2, 4, 4, 48, 3, 3),        # Cw = 48
                                   (2, 4, 4, 0, 3, 3), (0, 4, 4, 64, 3, 3), (2, 0, 4, 64, 3, 3), (2, 4, 4, 64, 0, 3),
                                   (1 << 11, 1 << 10, 1 << 10, 64, 3, 3),      # 2^31 points
                                   (1, 4, 4, 1024, 1, 1)])     # the weight alone fills the LDS
def test_what_the_predicate_declines(lib, shape):
    assert lib.wc_conv_narrow_out_supported(*shape) == 0
    # the entry answers WC_ERR_SHAPE in front of any launch (non-null pointers it never follows)
    g, w, out = (torch.zeros(4) for _ in range(3))
    N, H, W, cw, cn, k = shape
    code = lib.wc_conv_narrow_out_f32(g.data_ptr(), None, w.data_ptr(), 1, 1, 1, 1, N, H, W, cw, cn, k, out.data_ptr(), None)
    assert code == WC_ERR_SHAPE


def test_null_pointers_return_their_code_without_a_device(lib):
    t = torch.zeros(4)
    p = t.data_ptr()
    args = (1, 1, 1, 1, 2, 4, 4, 64, 3, 3)
    assert lib.wc_conv_narrow_out_f32(None, None, p, *args, p, None) == WC_ERR_NULL
    assert lib.wc_conv_narrow_out_f32(p, None, None, *args, p, None) == WC_ERR_NULL
    assert lib.wc_conv_narrow_out_f32(p, None, p, *args, None, None) == WC_ERR_NULL
    assert lib.wc_abi_version() == 8


def test_the_python_predicate_checks_the_channel_axes(lib):
    from wc_gan_amd import conv as C
    assert C.narrow_out_supported((2, 4, 4, 64), (64, 3, 3, 3)) and not C.narrow_out_supported((2, 4, 4, 64), (3, 64, 3, 3))
    assert C.narrow_out_supported((2, 4, 4, 64), (3, 64, 3, 3), forward=True)
    assert not C.narrow_out_supported((2, 4, 4, 128), (64, 3, 3, 3)) and not C.narrow_out_supported((2, 4, 4, 64), (64, 3, 3, 1))


# ---- the reference against torch's float64 autograd ------------------------------------------------------------------------------------
SMALL = [r for r in R.ROWS if r.N * r.H * r.W <= 4096]


@pytest.mark.parametrize("name", [r.name for r in SMALL])
def test_reference_matches_torch_float64(name):
    row = R.by_name(name)
    g, h, w, v = R.inputs(row)
    ref = R.reference(name)
    g64, h64 = torch.from_numpy(g).double().permute(0, 3, 1, 2), torch.from_numpy(h).double().permute(0, 3, 1, 2)
    gm64 = torch.ops.aten.threshold_backward(g64, h64, 0)
    assert bool((gm64 == 0).any()) and bool((torch.from_numpy(h) == 0).any())
    x = torch.zeros(row.N, row.Cn, row.H, row.W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, torch.from_numpy(w).double(), padding=row.k // 2)
    for key, go in (('dx', g64), ('dx_masked', gm64)):
        dx = torch.autograd.grad(y, x, go, retain_graph=True)[0].permute(0, 2, 3, 1).numpy()
        assert R.rel(dx, ref[key]) < 1e-12, key
    for key, gi in (('y', g64), ('y_masked', gm64)):
        out = F.conv2d(gi, torch.from_numpy(v).double(), padding=row.k // 2).permute(0, 2, 3, 1).numpy()
        assert R.rel(out, ref[key]) < 1e-12, key


def test_negative_zero_in_the_mask_masks():
    g = np.ones((1, 2, 2, 32), dtype=np.float32)
    h = np.full_like(g, -0.0)
    h[0, 0, 0, :] = 1.0
    w = np.ones((32, 1, 1, 1), dtype=np.float32)
    out = R.narrow_out(g, w, h)
    assert out[0, 0, 0, 0] == 32.0 and float(np.abs(out).sum()) == 32.0


# ---- the reference tells the faults apart ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault,name,band", [('halo', '3x5x7-64-3-k3', 2), ('halo', '1x3x720-32-1-k3', 1), ('halo', '4x64x64-64-3-k3', 16),
                                             ('unmirrored', '3x5x7-64-3-k3', 0), ('unmirrored', '2x1x2-32-1-k3', 0),
                                             ('mask_after', '3x5x7-64-3-k3', 0), ('mask_after', '2x6x8-64-3-k1', 0),
                                             ('partial', '3x5x7-64-3-k3', 0), ('partial', '2x1x2-32-1-k3', 0)])
def test_a_faulty_kernel_is_far_outside_the_bound(fault, name, band):
    row = R.by_name(name)
    g, h, w, _ = R.inputs(row)
    masked = fault == 'mask_after'
    ref = R.reference(name)['dx_masked' if masked else 'dx']
    assert R.rel(R.faulty(g, w, h if masked else None, fault, band), ref) > 1e-2
