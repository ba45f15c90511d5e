"""Every branch of the block convolutions' host dispatch (csrc/wc_conv.hip: wc_conv_f16x3, conv_ksplit, wrw_splits, the narrow kernels'
k-step table) at the smallest shape that reaches it, against torch's float64 convolution of the same map: forward, data gradient,
weight gradient and bias gradient.  Inputs, reference and tolerances are tests/test_conv_gpu.py's.

The instantiation each row is there for was worked out from the dispatch rules
    ksplit = 1 unless (M/128) * nphase * (Cout / (256 | 128)) <= 96: then ceil(256 / that), at most 8 and at most iters / 4
    <4, NB> (the 256-point tile) when ksplit == 1, M % 256 == 0 and (M/256) * nphase * (Cout / (256 | 128)) >= 256
and, for the rows that name one, is read back from a profiled call.

`PYTHONPATH=. python tests/test_conv_dispatch_gpu.py` prints the measured error of every row (profiles/conv_dispatch_parity.txt)."""
import re

import pytest
import torch
import torch.nn.functional as F

from test_conv_gpu import TOL, _rel, _weights

# kind, N, H, W, Cin, Cout, k, contiguous-format weight, (forward, data-gradient) instantiation to see in a profile | None
CASES = [
    ('same', 64, 32, 32, 128, 128, 3, False, ('<4,2,false>', '<4,2,false>')),      # the smallest M that reaches <4,2> with one phase
    ('down3', 128, 24, 24, 128, 128, 3, False, ('<2,2,false>', '<4,2,false>')),    # STL-10 critic: phase data gradient, 144-point images
    ('up3', 128, 12, 12, 128, 128, 3, False, ('<4,2,false>', '<2,2,false>')),      # <4,2> on the phase geometry's forward
    ('up3', 128, 12, 12, 256, 256, 3, False, ('<4,4,false>', '<2,4,false>')),      # <4,4> with tiles that straddle images
    ('same', 32, 6, 10, 128, 128, 3, False, None),          # H != W, W no power of two, 15 tiles; k-split 8
    ('down3', 32, 12, 20, 128, 256, 3, False, None),        # non-square, strided; data-gradient k-split 5
    ('up3', 32, 6, 10, 256, 128, 3, False, None),           # non-square, phases; forward k-split 5
    ('same', 2, 16, 4, 128, 128, 3, False, None),           # the same M with H and W exchanged
    ('same', 2, 4, 16, 128, 128, 3, False, None),
    ('same', 2, 8, 8, 1024, 1024, 3, False, None),          # reduction length 9216; weight-gradient 256-tile, splits clamped to M/32 = 4
    ('same', 2, 8, 8, 1024, 1024, 1, False, None),
    ('down3', 2, 16, 16, 512, 1024, 3, False, None),        # the Tiny-ImageNet critic's widths
    ('down3', 2, 32, 32, 256, 512, 3, False, None),
    ('same', 2, 16, 16, 512, 1024, 3, False, None),
    ('same', 2, 8, 8, 128, 128, 3, True, None),             # contiguous-format weight: weight gradient with x_cols == false, k_axis = 1
]
_ID = lambda c: '-'.join(str(v) for v in c[:7]) + ('-contiguous' if c[7] else '')


def _ref3(x, w, b, kind):
    """Conv2D 'same' | Conv2D 3x3 -> AveragePooling2D | UpSampling2D -> Conv2D 3x3, in x's dtype on NHWC"""
    xn = x.permute(0, 3, 1, 2)
    if kind == 'up3':
        xn = F.interpolate(xn, scale_factor=2, mode='nearest')
    y = F.conv2d(xn, w.to(x.dtype), b.to(x.dtype), padding=w.shape[2] // 2)
    if kind == 'down3':
        y = F.avg_pool2d(y, 2)
    return y.permute(0, 2, 3, 1)


def _kernel_names(fn):
    """device kernel names of one profiled call of fn (spaces removed)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not names:           # (a profiler build that does not tag device events: every kernel's name still says "kernel")
        names = [e.name for e in prof.events() if "kernel" in e.name.lower() and not e.name.startswith(("aten::", "hip", "cuda"))]
    return [n.replace(' ', '').replace('(bool)0', 'false').replace('(bool)1', 'true') for n in names]


def _instantiations(names, kernel):
    return [m.group(1) for n in names for m in [re.search(kernel + r'(<[^>]*>)', n)] if m]


def _case(kind, N, H, W, ci, co, k, contiguous):
    """-> (errors against float64 of the HIP route, the same of torch's fp32 convolution, x, w, b, gy)"""
    from wc_gan_amd import conv as C
    torch.manual_seed(N + H + ci)
    x = (torch.randn(N, H, W, ci, device='cuda') * 1.7 + 0.3).requires_grad_(True)
    w = _weights('same', ci, co, k, channels_last=not contiguous).requires_grad_(True)
    b = (torch.randn(co, device='cuda') * 0.1).requires_grad_(True)
    assert C.supported(x, w, kind)
    assert w.stride(1) == (k * k if contiguous else 1)
    y = C.fast_conv(x, w, b, kind)
    gy = torch.randn_like(y)
    grads = torch.autograd.grad(y, (x, w, b), gy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, b))
    y64 = _ref3(x64, w64, b64, kind)
    assert y.shape == y64.shape
    ref = (y64,) + torch.autograd.grad(y64, (x64, w64, b64), gy.double())
    y32 = _ref3(x, w, b, kind)
    t32 = (y32,) + torch.autograd.grad(y32, (x, w, b), gy)
    keys = ('y', 'dx', 'dw', 'db')
    errs = {n: _rel(a, r) for n, a, r in zip(keys, (y,) + grads, ref)}
    torch_errs = {n: _rel(a, r) for n, a, r in zip(keys, t32, ref)}
    assert grads[1].stride() == w.stride()
    return errs, torch_errs, x, w, b, gy


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_each_dispatch_branch_matches_float64(case):
    """y, dx, dW and db of one row of CASES against float64; the rows that name instantiations also read them from a profiled forward and
    a profiled backward (the only conv_f16x3_kernel launch of each)."""
    kind, N, H, W, ci, co, k, contiguous, want = case
    errs, torch_errs, x, w, b, gy = _case(kind, N, H, W, ci, co, k, contiguous)
    print("conv dispatch", _ID(case), "hip", errs, "torch fp32", torch_errs)
    assert errs['y'] < TOL and errs['dx'] < TOL and errs['db'] < TOL, errs
    assert errs['dw'] < 2e-5, errs
    if want is None:
        return
    from wc_gan_amd import conv as C
    fwd = _kernel_names(lambda: C.fast_conv(x, w, b, kind))
    y = C.fast_conv(x, w, b, kind)
    bwd = _kernel_names(lambda: torch.autograd.grad(y, (x, w, b), gy))
    if not fwd or not bwd:
        pytest.skip("this profiler build reports no device kernel names: the instantiation was not checked (the parity assertions ran)")
    assert _instantiations(fwd, 'conv_f16x3_kernel') == [want[0]], fwd
    assert _instantiations(bwd, 'conv_f16x3_kernel') == [want[1]], bwd


def _narrow_case():
    from wc_gan_amd import conv as C
    torch.manual_seed(11)
    shape, cout, k = (4, 8, 8, 30), 128, 1
    x = (torch.randn(*shape, device='cuda') * 0.7 + 0.1).requires_grad_(True)
    out = []
    for fmt in (torch.channels_last, torch.contiguous_format):
        w = (torch.randn(cout, shape[3], k, k, device='cuda') / (shape[3] * k * k) ** 0.5).contiguous(memory_format=fmt).requires_grad_(True)
        b = (torch.randn(cout, device='cuda') * 0.1).requires_grad_(True)
        assert C.narrow_wrw_supported(x, w) and not C.supported(x, w, 'same')
        y = C.narrow_in_conv(x, w, b)
        gy = torch.randn_like(y)
        dx, dw, db = torch.autograd.grad(y, (x, w, b), gy)
        dw2, = torch.autograd.grad(C.narrow_in_conv(x, w, b), (w,), gy)
        y64 = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=k // 2).permute(0, 2, 3, 1)
        dx64, dw64, db64 = torch.autograd.grad(y64, (x, w, b), gy.double())
        assert dw.stride() == w.stride() and torch.equal(dw, dw2)
        out.append((dict(y=_rel(y, y64), dx=_rel(dx, dx64), dw=_rel(dw, dw64), db=_rel(db, db64)), x, w, b))
    return out


@pytest.mark.gpu
def test_narrow_forward_at_its_widest_k_step_table():
    """k = 1 with 30 input channels: 16 k-step pairs (30 rows + the bias row), conv_fwd_narrow_kernel<16>; nrow = 30 in the one-pass
    weight gradient.  Bounds: test_narrow_input_weight_gradient_against_float64's."""
    from wc_gan_amd import conv as C
    for errs, x, w, b in _narrow_case():
        print("conv dispatch narrow 4-8-8-30-128-1", errs)
        assert errs['y'] < 1e-5 and errs['dx'] < 1e-5, errs
        assert errs['dw'] < 2e-6 and errs['db'] < 2e-6, errs
    names = _kernel_names(lambda: C.narrow_in_conv(x, w, b))
    if not names:
        pytest.skip("this profiler build reports no device kernel names: the instantiation was not checked (the parity assertions ran)")
    assert _instantiations(names, 'conv_fwd_narrow_kernel') == ['<16>'], names


if __name__ == '__main__':
    print(f"{'case':<44}{'route':<12}{'y':>10}{'dx':>10}{'dw':>10}{'db':>10}")
    for case in CASES:
        errs, torch_errs = _case(*case[:8])[:2]
        for route, e in (('hip', errs), ('torch fp32', torch_errs)):
            print(f"{_ID(case):<44}{route:<12}" + ''.join(f"{e[n]:>10.2e}" for n in ('y', 'dx', 'dw', 'db')))
    for fmt, (errs, *_rest) in zip(('channels_last', 'contiguous'), _narrow_case()):
        print(f"{'narrow 4-8-8-30-128-1 ' + fmt:<44}{'hip':<12}" + ''.join(f"{errs[n]:>10.2e}" for n in ('y', 'dx', 'dw', 'db')))
