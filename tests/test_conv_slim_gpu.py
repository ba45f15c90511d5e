"""The block convolutions at 64 and 32 channels (csrc/wc_conv.hip: conv_f16x3_slim_kernel's 128-point x 32-output tiles, conv_wrw_slim_kernel's
32 x 32 tiles, and the 64-wide tiles the kernels always had, reached through a layer marked slim_conv) against
torch's float64 convolution of the same map and its autograd, in both weight memory formats, on guard-banded memory, and through a cut-down
ImageNet-recipe generator against tests/generator_reference.py.  Reference, inputs and tolerances are tests/test_conv_gpu.py's and
tests/test_conv_dispatch_gpu.py's (imported): y, dx, db < TOL = 1e-5 and dW < 2 * TOL of the tensor's maximum; the network's bounds are
tests/test_generator_gpu.py's BOUNDS, on the ReLU signs the HIP network applied.  The row table is tests/test_conv_slim.py's.

`PYTHONPATH=. python tests/test_conv_slim_gpu.py` prints the measured error of every row (profiles/slim_conv_parity.txt)."""
import ctypes
import functools

import pytest
import torch

from test_conv_dispatch_gpu import _ref3
from test_conv_gpu import TOL, _ref, _rel, _weights
from test_conv_slim import ROW_ID, ROWS, _geoms, route_labels, slim_side

DW_TOL = 2 * TOL
FORMATS = ('channels_last', 'contiguous')


class _Site:
    """a layer object as conv.fast_conv_or_none sees it: marked, with room for the splits' records"""
    slim_conv = True


class _Plain:
    """the same layer without the mark"""


@functools.lru_cache(maxsize=None)
def _case(row):
    """inputs (fp32, on the GPU) and the float64 reference of a row, computed once: y, y of the ReLU'd input, and the gradients of both"""
    kind, N, H, W, ci, co, k = row
    torch.manual_seed(N + H + ci + co)
    x = torch.randn(N, H, W, ci, device='cuda') * 1.7 + 0.3
    w = _weights('same', ci, co, k, channels_last=False)
    b = torch.randn(co, device='cuda') * 0.1
    Ho, Wo = (2 * H, 2 * W) if kind == 'up3' else (H, W)
    gy = torch.randn(N, Ho, Wo, co, device='cuda')
    ref = {}
    for name, act in (('plain', lambda t: t), ('relu', torch.relu)):
        x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
        y64 = _ref3(act(x64), w64, b64, kind)
        ref[name] = (y64.detach(),) + torch.autograd.grad(y64, (x64, w64, b64), gy.double())
    return x, w, b, gy, ref


def _leaves(row, fmt):
    x, w, b, gy, ref = _case(row)
    wd = w.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else w.contiguous()
    return x.clone().requires_grad_(True), wd.clone().requires_grad_(True), b.clone().requires_grad_(True), gy, ref


def _row(row, fmt):
    """{name: error} of one row in one weight memory format: forward and the three gradients, without and with the ReLU in the split"""
    from wc_gan_amd import conv as C
    kind = row[0]
    errs = {}
    for name in ('plain', 'relu'):
        x, w, b, gy, ref = _leaves(row, fmt)
        if name == 'plain':
            y = C.fast_conv(x, w, b, kind, slim=True)
        else:
            y = C.fast_conv_or_none(x, w, b, kind, relu_input=True, site=_Site())
            assert y is not None
        grads = torch.autograd.grad(y, (x, w, b), gy)
        assert y.shape == ref[name][0].shape and grads[1].stride() == w.stride()
        for n, a, r in zip(('y', 'dx', 'dw', 'db'), (y,) + grads, ref[name]):
            errs[n if name == 'plain' else n + '_relu'] = _rel(a, r)
    return errs


def _assert_bounds(errs):
    for n, e in errs.items():
        assert e < (DW_TOL if n.startswith('dw') else TOL), (n, e, errs)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_each_row_matches_float64_in_both_weight_formats(row, fmt):
    """forward with and without the ReLU input, dx, dW and db; the 32-wide side lands on the weight gradient's rows in one memory format and
    on its columns in the other (x_cols in wrw_prepare)"""
    from wc_gan_amd import _lib, conv as C
    lib = _lib.load()
    x, w, b, gy, _ = _leaves(row, fmt)
    assert row[6] == 1 or (w.stride(1) == 1) == (fmt == 'channels_last')      # (a 1x1 weight has one dense layout)
    # the predicate and the launch agree (the 96 -> 96 row: taken, as three tiles of 32 outputs)
    gf, gd = _geoms(*row)
    assert all(lib.wc_conv_slim_supported(ctypes.addressof(g)) == 1 for g in (gf, gd))
    assert C.supported(x, w, row[0], slim=True) and not C.supported(x, w, row[0])
    errs = _row(row, fmt)
    print("slim conv", ROW_ID(row), fmt, {k: f"{v:.2e}" for k, v in errs.items()})
    _assert_bounds(errs)


@pytest.mark.gpu
def test_the_table_runs_both_epilogues_at_32_outputs():
    """labelled from wc_conv_workspace_bytes (0 = the direct epilogue, > 0 = the k-split's partial sums): the forward and the data gradient
    each run a 32-output geometry of either label"""
    from wc_gan_amd import _lib
    assert route_labels(_lib.load()) == {('forward', 'direct'), ('forward', 'ksplit'), ('dgrad', 'direct'), ('dgrad', 'ksplit')}


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_the_layer_entry_routes_a_marked_layer_only(row):
    from wc_gan_amd import conv as C
    x, w, b, gy, _ = _leaves(row, 'channels_last')
    assert C.fast_conv_or_none(x, w, b, row[0], site=_Plain()) is None
    assert C.fast_conv_or_none(x, w, b, row[0]) is None
    y = C.fast_conv_or_none(x, w, b, row[0], site=_Site())
    assert isinstance(y, torch.Tensor) and y.shape == gy.shape


def _twice(row):
    from wc_gan_amd import conv as C
    outs = []
    for _ in range(2):
        x, w, b, gy, _ = _leaves(row, 'channels_last')
        y = C.fast_conv(x, w, b, row[0], slim=True)
        outs.append((y.detach(),) + torch.autograd.grad(y, (x, w, b), gy))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("row", [ROWS[0], ROWS[3], ROWS[6], ROWS[8]], ids=ROW_ID)
def test_a_second_call_gives_the_same_bits(row):
    a, b = _twice(row)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


@pytest.mark.gpu
def test_a_marked_layer_runs_the_new_kernels_and_no_torch_convolution():
    from test_dcgan_gpu import _convolution_ops, _op_and_kernel_names
    row = ROWS[0]                                       # 32 -> 32, 3x3: every launch of the layer is a 32-wide one
    _twice(row)
    ops, kernels = _op_and_kernel_names(lambda: _twice(row))
    assert ops, "the profiler reported no operators"
    assert _convolution_ops(ops) == [], _convolution_ops(ops)
    if kernels:
        joined = ' '.join(kernels)
        assert 'miopen' not in joined.lower(), [k for k in kernels if 'miopen' in k.lower()]
        for name in ('conv_f16x3_slim_kernel', 'conv_wrw_slim_kernel', 'conv_ksplit_reduce_kernel', 'conv_wrw_reduce_kernel'):
            assert name in joined, name
        assert 'conv_f16x3_kernel' not in joined and 'conv_wrw_kernel' not in joined


# 32-output rows: a k-split forward and data gradient; the direct epilogue with a 64-output data gradient; the phase forward (strided
# stores) with a strided data gradient -- and the 96-wide row, whose last tile ends at the row's last channel
STRAY = [ROWS[0], ROWS[4], ROWS[6], ROWS[9]]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("row", STRAY, ids=ROW_ID)
def test_no_stray_writes_on_guard_banded_memory(row, fmt):
    """outputs, k-split partial sums, the weight gradient's partial sums, planes and weight images allocated inside poisoned guard bands
    (tests/_poison.py): the bands are intact behind forward and backward, the results do not depend on the fill, under the NaN fill no NaN
    is left in y, dx, dW or db -- a store sized for a 64-wide tile would show in each of the three -- and the values are the reference's"""
    from _poison import run_patterns
    from wc_gan_amd import conv as C
    kind = row[0]
    x, w, b, gy, ref = _case(row)
    x, w, b, gy = x.cpu(), w.cpu(), b.cpu(), gy.cpu()

    def run(P):
        xd = P.guarded(x).requires_grad_(True)
        wd = P.guarded(w)
        wd = (wd.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else wd).requires_grad_(True)
        bd = P.guarded(b).requires_grad_(True)
        p = C._plan(kind, xd, wd, False, True)
        assert p and p.ok
        y = C._FastConv.apply(xd, wd, bd, kind, p)
        return [y] + list(torch.autograd.grad(y, (xd, wd, bd), P.guarded(gy)))

    outs = run_patterns(run)
    for t in outs[0xFF]:
        assert not bool(torch.isnan(t).any())
    for t, r, tol in zip(outs[0xFF], ref['plain'], (TOL, TOL, DW_TOL, TOL)):
        assert _rel(t.cuda(), r) < tol


# ---- the network: a cut-down recipe generator against the float64 reference ---------------------------------------------------------------
NET_KW = dict(block_sizes=(128, 64, 32), resamples=('UP', 'UP', 'UP'), first_block_shape=(4, 4, 128), number_of_classes=1000,
              block_norm='d', block_after_norm='ufconv', filters_emb=32, last_norm='d', last_after_norm='uconv', gan_type='PROJECTIVE')
NET_BATCH = 32              # the first site has 32 * 16 = 512 = 4 C rows


def _net_module():
    import test_generator_gpu as TG
    from wc_gan_amd.generator import make_generator
    torch.manual_seed(7)
    G = make_generator(slim_conv=True, **NET_KW)
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith(('.bias', '.beta', '.gamma', '.kernel', '.class_matrix')):
                p.add_(0.05 * torch.randn_like(p))
    return G.cuda(), TG


def _net_inputs(seed):
    g = torch.Generator(device='cpu'); g.manual_seed(seed)
    z = torch.randn(NET_BATCH, 128, generator=g, dtype=torch.float64)
    cls = torch.randint(0, 1000, (NET_BATCH, 1), generator=g, dtype=torch.int32)
    w = torch.randn(NET_BATCH, 32, 32, 3, generator=g, dtype=torch.float64)
    return z.float().cuda(), cls.cuda(), w.cuda()


def _net_call(G, TG, z, cls, w, train):
    """one pass of the module (tests/test_generator_gpu.py's _hip_call without its recipes' route table) -> the errors against the reference
    given the signs this pass applied, and the (Cin, weight shape) of every convolution the block kernels took"""
    import generator_reference as R
    import wc_gan_amd.functional as WF
    from wc_gan_amd import conv as C
    state = {k: v.detach().clone() for k, v in G.state_dict().items()}
    G.train(train)
    for p in G.parameters():
        p.grad = None
    took, conv0 = [], C.fast_conv_or_none

    def conv(x, w_, *a, **k):
        y = conv0(x, w_, *a, **k)
        if y is not None:
            took.append((x.shape[-1], tuple(w_.shape)))
        return y
    probe, rec = TG._Probe(G, signs=not train), []
    with probe:
        C.fast_conv_or_none = conv              # (inside the probe's own wrapper: the generator calls through the module attribute)
        try:
            if train:
                WF.MASK_TAP = {'record': rec}
                try:
                    img = G(z, cls)
                finally:
                    WF.MASK_TAP = None
                (img * w.float()).sum().backward()
            else:
                with torch.no_grad():
                    img = G(z, cls)
        finally:
            C.fast_conv_or_none = conv0
    masks = [TG._unpack(m, s) for m, s in zip(rec, probe.shapes)] if train else probe.masks
    assert len(masks) == R.relu_count(NET_KW['block_sizes'])
    grads = {n: p.grad for n, p in G.named_parameters() if p.grad is not None} if train else None
    moving = TG._moving(G) if train else None
    kw = dict(NET_KW, **TG._site_kw(G))
    ref, ref_img, ref_grads = R.run(state, kw, z, cls, w if train else None, masks, training=train)
    TG._check_masks(masks, ref, 'slim network ' + ('train' if train else 'eval'))
    if train:
        assert set(grads) == set(n for n, _ in G.named_parameters())
    return R.errors(img.detach(), grads, moving, ref, ref_img, ref_grads), took


def _net_rows():
    G, TG = _net_module()
    rows = []
    z, cls, w = _net_inputs(21)
    rows.append(('train',) + _net_call(G, TG, z, cls, w, True))
    z, cls, w = _net_inputs(23)
    rows.append(('eval',) + _net_call(G, TG, z, cls, None, False))
    return rows, TG


@pytest.mark.gpu
def test_a_cut_down_recipe_generator_against_the_float64_reference():
    """blocks of 128, 64 and 32 filters from a (4, 4, 128) first block with the recipe's norms, 1000 classes and filters_emb 32, slim_conv
    on, at batch 32: image, every parameter gradient and the moving statistics of one training call, the image of one evaluation call"""
    rows, TG = _net_rows()
    bad = []
    for label, errs, took in rows:
        print("slim network", label, {k: f"{v:.2e}" for k, v in errs.items()})
        bad += [(label, k, v, TG.BOUNDS[k]) for k, v in errs.items() if not v < TG.BOUNDS[k]]
        # both narrow blocks' conv1, conv2 and shortcut took the block kernels
        for layer in ((128, (64, 128, 3, 3)), (64, (64, 64, 3, 3)), (128, (64, 128, 1, 1)),
                      (64, (32, 64, 3, 3)), (32, (32, 32, 3, 3)), (64, (32, 64, 1, 1))):
            assert layer in took, (label, layer, took)
    assert not bad, bad


if __name__ == '__main__':
    import os
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                              'slim_conv_parity.txt')
    from wc_gan_amd import _lib
    lib = _lib.load()
    names = ('y', 'dx', 'dw', 'db', 'y_relu', 'dx_relu', 'dw_relu', 'db_relu')
    lines = [f"{'row':<24}{'weight':<15}{'fwd / dgrad':<16}" + ''.join(f"{n:>10}" for n in names)]
    for row in ROWS:
        label = ' / '.join('k-split' if lib.wc_conv_workspace_bytes(ctypes.addressof(g)) else 'direct' for g in _geoms(*row))
        for fmt in FORMATS:
            errs = _row(row, fmt)
            _assert_bounds(errs)
            lines.append(f"{ROW_ID(row):<24}{fmt:<15}{label:<16}" + ''.join(f"{errs[n]:>10.2e}" for n in names))
    lines.append(f"bounds: y, dx, db {TOL:.0e}; dw {DW_TOL:.0e} of the tensor's maximum against torch's float64 convolution (tests/test_conv_gpu.py)")
    rows, TG = _net_rows()
    import generator_reference as R
    lines.append(f"{'cut-down generator (128, 64, 32), batch 32':<55}" + ''.join(f"{k:>10}" for k in R.KINDS))
    for label, errs, _ in rows:
        lines.append(f"{label:<55}" + ''.join(f"{errs[k]:>10.2e}" for k in R.KINDS))
    lines.append(f"{'bound (tests/test_generator_gpu.py BOUNDS)':<55}" + ''.join(f"{TG.BOUNDS[k]:>10.0e}" for k in R.KINDS))
    with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
