"""The narrow-output convolution (csrc/wc_conv.hip conv_narrow_out_kernel through wc_conv_narrow_out_f32 / conv.narrow_out_conv) against
the NumPy float64 direct sums of tests/narrow_out_reference.py: every row plain and masked (the mask holds exact zeros and -0.0), in both
weight formats and both orientations (the data gradient of an image layer; the forward of a layer with few outputs), the same bits on
a second call, three rows on poisoned guard-banded buffers, a declined shape that writes nothing.  Bound: 1e-5 of the tensor's maximum
(narrow_out_reference.BOUND, tests/test_narrow_edges_gpu.py's for the narrow kernels' data gradient); torch's fp32 convolution_backward
of the same inputs is measured beside it.

    PYTHONPATH=. python tests/test_narrow_out_gpu.py          # the table of profiles/narrow_out_parity.txt"""
import numpy as np
import pytest
import torch

import narrow_out_reference as R
from _poison import run_patterns, same_bits

pytestmark = pytest.mark.gpu

WC_ERR_SHAPE = -2
FORMATS = ('contiguous', 'channels_last')
KEYS = [(o, m) for o in ('dx', 'y') for m in (False, True)]


def _dev(a, fmt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else t


def _key(orient, masked):
    return orient + ('_masked' if masked else '')


def _measure(row, fmt):
    """-> {key: error of the kernel against float64}, {key: the same of torch's fp32 convolution}; asserts the same bits on a second call"""
    from wc_gan_amd import conv as C
    g, h, w, v = R.inputs(row)
    ref = R.reference(row.name)
    gd, hd, wd, vd = _dev(g), _dev(h), _dev(w, fmt), _dev(v, fmt)
    assert C.narrow_out_supported(tuple(gd.shape), tuple(wd.shape)) and C.narrow_out_supported(tuple(gd.shape), tuple(vd.shape), forward=True)
    hip, t32 = {}, {}
    gm = torch.ops.aten.threshold_backward(gd, hd, 0)
    x = torch.zeros(row.N, row.Cn, row.H, row.W, device='cuda')
    pad = [row.k // 2, row.k // 2]
    for orient, masked in KEYS:
        key = _key(orient, masked)
        weight = wd if orient == 'dx' else vd
        out = C.narrow_out_conv(gd, weight, mask=hd if masked else None, forward=orient == 'y')
        assert out.shape == (row.N, row.H, row.W, row.Cn) and out.is_contiguous()
        assert same_bits(out, C.narrow_out_conv(gd, weight, mask=hd if masked else None, forward=orient == 'y')), key
        hip[key] = R.rel(out.cpu().numpy(), ref[key])
        gi = (gm if masked else gd).permute(0, 3, 1, 2)
        if orient == 'dx':
            o32 = torch.ops.aten.convolution_backward(gi, x, weight, None, [1, 1], pad, [1, 1], False, [0, 0], 1, [True, False, False])[0]
        else:
            o32 = torch.nn.functional.conv2d(gi, weight, padding=row.k // 2)
        t32[key] = R.rel(o32.permute(0, 2, 3, 1).cpu().numpy(), ref[key])
    return hip, t32


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", [r.name for r in R.ROWS])
def test_a_row_matches_float64_plain_and_masked_in_both_orientations(name, fmt):
    row = R.by_name(name)
    hip, t32 = _measure(row, fmt)
    print("narrow out", name, fmt, "hip", hip, "torch fp32", t32)
    assert all(e < R.BOUND for e in hip.values()), (hip, t32)


def test_the_mask_is_threshold_backwards_predicate():
    """-0.0, 0.0 and negative pre-activations mask; a NaN pre-activation lets the gradient through, as torch's threshold_backward does"""
    from wc_gan_amd import conv as C
    g = torch.ones(1, 2, 2, 32, device='cuda')
    h = torch.full_like(g, -0.0)
    h[0, 0, 1, :] = 0.0
    h[0, 1, 0, :] = -1.0
    h[0, 1, 1, :] = float('nan')
    w = torch.ones(32, 1, 1, 1, device='cuda')
    out = C.narrow_out_conv(g, w, mask=h)
    want = torch.ops.aten.threshold_backward(g, h, 0).sum(-1, keepdim=True)
    assert torch.equal(out, want) and out.flatten().tolist() == [0.0, 0.0, 0.0, 32.0]


@pytest.mark.parametrize("name", R.POISON_ROWS)
def test_on_poisoned_guarded_buffers(name):
    """Guard bands around g, the mask, the weights and the outputs; the same bits whatever the fresh buffers held -- the clamped loads of a
    partial tile and the idle waves of a short band leave nothing."""
    from wc_gan_amd import conv as C
    row = R.by_name(name)
    g, h, w, v = R.inputs(row)
    ref = R.reference(name)

    def call(P):
        gd, hd, wd, vd = (P.guarded(a) for a in (g, h, w, v))
        return dict(dx=C.narrow_out_conv(gd, wd), dx_masked=C.narrow_out_conv(gd, wd, mask=hd),
                    y=C.narrow_out_conv(gd, vd, forward=True), y_masked=C.narrow_out_conv(gd, vd, mask=hd, forward=True))
    for o in run_patterns(call).values():
        for key, val in o.items():
            assert R.rel(val.numpy(), ref[key]) < R.BOUND, key


@pytest.mark.parametrize("shape", [(1, 3, R.WIDEST.W + 1, 32, 1, 3), (2, 4, 4, 48, 3, 3), (2, 4, 4, 64, 4, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_a_declined_shape_writes_nothing(shape):
    from wc_gan_amd import _lib, conv as C
    from wc_gan_amd.ops import _ptr, _stream
    N, H, W, cw, cn, k = shape
    assert not C.narrow_out_supported((N, H, W, cw), (cw, cn, k, k))
    g, h, w = torch.randn(N, H, W, cw, device='cuda'), torch.randn(N, H, W, cw, device='cuda'), torch.randn(cw, cn, k, k, device='cuda')
    out = torch.empty(N, H, W, cn, device='cuda')
    out.view(torch.uint8).fill_(0x5A)
    for mask in (None, h):
        code = _lib.load().wc_conv_narrow_out_f32(_ptr(g), _ptr(mask), _ptr(w), *w.stride(), N, H, W, cw, cn, k, _ptr(out), _stream())
        assert code == WC_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == 0x5A).all())
    with pytest.raises(_lib.WcHipError):
        C.narrow_out_conv(g, w)


if __name__ == '__main__':
    keys = [_key(o, m) for o, m in KEYS]
    print(f"{'row':<20}{'format':<16}{'route':<12}" + ''.join(f"{k:>12}" for k in keys))
    worst = dict.fromkeys(keys, 0.0)
    for row in R.ROWS:
        for fmt in FORMATS:
            hip, t32 = _measure(row, fmt)
            for route, e in (('hip', hip), ('torch fp32', t32)):
                print(f"{row.name:<20}{fmt:<16}{route:<12}" + ''.join(f"{e[k]:>12.2e}" for k in keys))
            worst = {k: max(worst[k], hip[k]) for k in keys}
    print(f"{'maximum':<20}{'':<16}{'hip':<12}" + ''.join(f"{worst[k]:>12.2e}" for k in keys))
    print(f"bound {R.BOUND:.0e} (max |error| / max |reference|)")
