"""A critic marked slim_blocks on the GPU: its 64-wide layers through the marked layer entries against torch's
float64 convolution in both weight formats (tests/test_conv_slim_gpu.py's bounds: y, dx, db 1e-5, dW 2e-5 of the tensor's maximum; the
rows are tests/test_critic_slim.py's, which shows that they cover both epilogues and the F1 tail at 64 inputs), two cut-down critics as
networks against tests/critic_reference.py in the manner of tests/test_critic_gpu.py (forced masks with its MASK_BAND check; output, image
gradient and every parameter gradient; eval and two training calls), and the routes and bits: a marked pass runs no convolution of
torch's, an unmarked critic runs what it ran, a marked 128-wide critic has the unmarked one's bits.

BOUNDS: four times the worse of the HIP route and torch fp32 on the first run, rounded up to one digit, capped at 1e-4
(profiles/critic_slim_parity.txt; `PYTHONPATH=. python tests/test_critic_slim_gpu.py` prints that table)."""
import functools

import pytest
import torch

import test_critic_gpu as TC
from test_conv_dispatch_gpu import _ref3
from test_conv_gpu import TOL, _rel, _weights
from test_critic_slim import ROW_ID, ROWS
from test_dcgan_gpu import _convolution_ops, _op_and_kernel_names

pytestmark = pytest.mark.gpu

DW_TOL = 2 * TOL
FORMATS = ('channels_last', 'contiguous')


# ---- the layers ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(row):
    """inputs (fp32, on the GPU) and the float64 reference of a row, computed once: the layer as the critic calls it -- conv(relu(x)) for a
    3x3 layer (pooled for 'down3'), conv(x) for the 1x1 shortcut -- and its gradients"""
    kind, N, H, W, ci, co, k = row
    torch.manual_seed(N + H + ci + co + k)
    x = torch.randn(N, H, W, ci, device='cuda') * 1.7 + 0.3
    w = _weights('same', ci, co, k, channels_last=False)
    b = torch.randn(co, device='cuda') * 0.1
    Ho, Wo = (H // 2, W // 2) if kind == 'down3' else (H, W)
    gy = torch.randn(N, Ho, Wo, co, device='cuda')
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = _ref3(torch.relu(x64) if k == 3 else x64, w64, b64, kind)
    ref = (y64.detach(),) + torch.autograd.grad(y64, (x64, w64, b64), gy.double())
    return x, w, b, gy, ref


def _layer(row, fmt, on=True):
    from wc_gan_amd.generator import Conv2D
    kind, N, H, W, ci, co, k = row
    x, w, b, gy, ref = _case(row)
    layer = Conv2D(ci, co, (k, k), slim_blocks=on).cuda()
    with torch.no_grad():
        layer.conv.weight.data = (w.contiguous(memory_format=torch.channels_last) if fmt == 'channels_last' else w.contiguous()).clone()
        layer.conv.bias.copy_(b)
    return layer


def _run_layer(layer, row, x):
    kind, k = row[0], row[6]
    if kind == 'down3':
        return layer.forward_pooled(x, relu_input=True)
    return layer.forward_relu(x) if k == 3 else layer(x)


def _row(row, fmt):
    """{name: error} of one row in one weight format through the marked layer's entries; asserts that the block kernels took the call"""
    from wc_gan_amd import conv as C
    x, w, b, gy, ref = _case(row)
    layer = _layer(row, fmt)
    took, conv0 = [], C.fast_conv_or_none

    def conv(*a, **k):
        y = conv0(*a, **k)
        took.append(y is not None)
        return y
    C.fast_conv_or_none = conv
    try:
        xl = x.clone().requires_grad_(True)
        y = _run_layer(layer, row, xl)
    finally:
        C.fast_conv_or_none = conv0
    assert took == [True], took
    grads = torch.autograd.grad(y, (xl, layer.conv.weight, layer.conv.bias), gy)
    assert y.shape == ref[0].shape and grads[1].stride() == layer.conv.weight.stride()
    assert row[6] == 1 or (layer.conv.weight.stride(1) == 1) == (fmt == 'channels_last')
    return {n: _rel(a, r) for n, a, r in zip(('y', 'dx', 'dw', 'db'), (y,) + grads, ref)}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("row", ROWS, ids=ROW_ID)
def test_each_layer_row_matches_float64_in_both_weight_formats(row, fmt):
    errs = _row(row, fmt)
    print("critic slim layer", ROW_ID(row), fmt, {k: f"{v:.2e}" for k, v in errs.items()})
    for n, e in errs.items():
        assert e < (DW_TOL if n == 'dw' else TOL), (n, e, errs)


@pytest.mark.parametrize("row", [ROWS[0], ROWS[4]], ids=ROW_ID)
def test_an_unmarked_layer_keeps_its_route(row):
    from wc_gan_amd import conv as C
    x, w, b, gy, ref = _case(row)
    layer = _layer(row, 'channels_last', on=False)
    assert C.fast_conv_or_none(x, layer.conv.weight, layer.conv.bias, row[0], relu_input=True, site=layer) is None
    y = _run_layer(layer, row, x)
    assert _rel(y, ref[0]) < TOL


# ---- the networks -------------------------------------------------------------------------------------------------------------------------
NET_BATCH = 8
NETS = {
    'down-down-same': dict(input_image_shape=(16, 16, 3), block_sizes=(64, 128, 128), resamples=('DOWN', 'DOWN', 'SAME'), number_of_classes=10,
                           type='PROJECTIVE', spectral=True, sum_pool=True, conv_singular=False, slim_blocks=True),
    'down-same-64': dict(input_image_shape=(16, 16, 3), block_sizes=(64, 64), resamples=('DOWN', 'SAME'), number_of_classes=10,
                         type='PROJECTIVE', spectral=True, sum_pool=True, conv_singular=False, slim_blocks=True),
}
CEILING = 1e-4
# relative error = max |a - ref| / max |ref| per tensor, the worst tensor of a kind, over both networks (eval, training calls 1 and 2): the larger of
# the two routes, x 4, rounded up to one digit (profiles/critic_slim_parity.txt):
#   out     hip 3.88e-07  torch fp32 4.50e-07  -> 1.8e-06 -> 2e-06
#   dx      hip 4.94e-07  torch fp32 4.49e-07  -> 2.0e-06 -> 2e-06
#   conv_w  hip 4.79e-07  torch fp32 6.66e-07  -> 2.7e-06 -> 3e-06
#   bias    hip 3.32e-07  torch fp32 2.92e-07  -> 1.3e-06 -> 2e-06
#   head    hip 4.18e-07  torch fp32 4.06e-07  -> 1.7e-06 -> 2e-06
BOUNDS = dict(out=2e-6, dx=2e-6, conv_w=3e-6, bias=2e-6, head=2e-6)
assert all(b <= CEILING for b in BOUNDS.values())


def _count_nodes(fn):
    """-> (calls of conv.critic_first_block, of conv.critic_block) while fn runs"""
    from wc_gan_amd import conv as C
    seen = dict(first=0, block=0)
    first0, block0 = C.critic_first_block, C.critic_block

    def first(*a, **k):
        seen['first'] += 1
        return first0(*a, **k)

    def block(*a, **k):
        seen['block'] += 1
        return block0(*a, **k)
    C.critic_first_block, C.critic_block = first, block
    try:
        fn()
    finally:
        C.critic_first_block, C.critic_block = first0, block0
    return seen['first'], seen['block']


@pytest.mark.parametrize("net", list(NETS))
def test_cut_down_critic_in_eval_mode(net):
    errs, = TC._critic_errors(NETS[net], NET_BATCH, training=False)
    print("critic slim", net, "eval", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BOUNDS[k], (net, k, v, BOUNDS[k])


@pytest.mark.parametrize("net", list(NETS))
def test_cut_down_critic_in_two_training_calls(net):
    """the second call runs on history-scaled splits -- the first block's conv1 writes conv2's planes, block 1's conv1 finish writes its
    conv2's (F1 at 64 inputs) -- and an advanced (u, v); each call against its own reference"""
    for call, errs in enumerate(TC._critic_errors(NETS[net], NET_BATCH, training=True)):
        print("critic slim", net, "train call", call + 1, {k: f"{v:.2e}" for k, v in errs.items()})
        for k, v in errs.items():
            assert v < BOUNDS[k], (net, call, k, v, BOUNDS[k])


@pytest.mark.parametrize("net", list(NETS))
def test_every_block_of_a_marked_critic_runs_as_its_fused_node(net):
    kw = NETS[net]
    for on in (True, False):
        D = TC._module(dict(kw, slim_blocks=on), 'cuda').train()
        x, cls, weights = TC._inputs(kw, NET_BATCH, 'cuda', 3)
        first, block = _count_nodes(lambda: D(x, cls))
        if on:
            assert (first, block) == (1, len(kw['block_sizes']) - 1)
        else:       # the 64-wide blocks stay separate nodes; the 128 -> 128 SAME block of the first net is the fused node it always was
            assert (first, block) == (0, 1 if net == 'down-down-same' else 0)


# ---- routes and bits ----------------------------------------------------------------------------------------------------------------------
def _pass(D, x, cls, weights):
    for p in D.parameters():
        p.grad = None
    x.grad = None
    TC._loss(D(x, cls), weights).backward()


def _profiled(kw, narrow_out=True):
    from wc_gan_amd import conv as C
    D = TC._module(kw, 'cuda').train()
    x, cls, weights = TC._inputs(kw, NET_BATCH, 'cuda', 3)
    before = C.NARROW_OUT
    C.NARROW_OUT = narrow_out
    try:
        _pass(D, x, cls, weights)
        _pass(D, x, cls, weights)                       # (first calls measure and log: profile the steady state)
        return _op_and_kernel_names(lambda: _pass(D, x, cls, weights))
    finally:
        C.NARROW_OUT = before


def test_a_marked_pass_with_an_image_gradient_runs_no_torch_convolution_and_one_weight_batch():
    ops, kernels = _profiled(NETS['down-down-same'])
    assert ops, "the profiler reported no operators"
    assert _convolution_ops(ops) == [], _convolution_ops(ops)
    if kernels:
        joined = ' '.join(kernels)
        assert 'miopen' not in joined.lower(), [k for k in kernels if 'miopen' in k.lower()]
        assert len([k for k in kernels if 'conv_weights_batch_kernel' in k]) == 1, [k for k in kernels if 'weights' in k]
        assert not [k for k in kernels if 'conv_weights_kernel' in k or 'conv_weights_pair_kernel' in k]
        # conv1's masked gradient and the shortcut's plain one
        assert len([k for k in kernels if 'conv_narrow_out_kernel' in k]) == 2, kernels
        assert 'conv_fwd_narrow_split_kernel' in joined and 'conv_wrw_narrow_masked_kernel' in joined


def test_an_unmarked_critic_runs_what_it_ran():
    kw = dict(NETS['down-down-same'], slim_blocks=False)
    ops, kernels = _profiled(kw)
    ops_off, kernels_off = _profiled(kw, narrow_out=False)
    assert 'aten::convolution_backward' in ops and 'aten::convolution_backward' in ops_off
    assert not [k for k in kernels if 'conv_narrow_out_kernel' in k]
    assert sorted(kernels) == sorted(kernels_off)
    assert sorted(ops) == sorted(ops_off)


def _two_calls(kw, batch, narrow_out=True, launches=None):
    """two training calls of a fresh critic -> [(outputs, image gradient, parameter gradients)]; launches: a list that receives one entry
    per call of conv.narrow_out_conv"""
    from wc_gan_amd import conv as C
    D = TC._module(kw, 'cuda').train()
    before, conv0 = C.NARROW_OUT, C.narrow_out_conv

    def counted(*a, **k):
        if launches is not None:
            launches.append(k.get('mask') is not None)
        return conv0(*a, **k)
    C.NARROW_OUT, C.narrow_out_conv = narrow_out, counted
    try:
        outs = []
        for call in range(2):
            x, cls, weights = TC._inputs(kw, batch, 'cuda', 10 + call)
            out = D(x, cls)
            grads = torch.autograd.grad(TC._loss(out, weights), [x] + list(D.parameters()))
            outs.append(((out if isinstance(out, tuple) else (out,)), grads[0], grads[1:]))
        return outs
    finally:
        C.NARROW_OUT, C.narrow_out_conv = before, conv0


def test_a_marked_128_wide_critic_has_the_unmarked_ones_bits():
    """Outputs and every parameter gradient: the same bits marked, unmarked, and marked with NARROW_OUT off.  The image gradient is the
    one thing the mark changes at 128 channels: two launches of the narrow-output kernel (conv1's masked, the shortcut's plain) with the
    switch on, none with it off -- the route the unmarked critic takes.  That route's values are MIOpen's data gradient, which does not
    repeat its own bits between two runs of the UNMARKED critic (measured: 1e-7 of the tensor's maximum apart), so the three image gradients
    are held to each other at the layers' 1e-5, and the new kernel to its own bits on a second critic."""
    from wc_gan_amd.train import CONFIGS
    kw = CONFIGS['cifar10_uncond']['discriminator']
    n_plain, n_on, n_off = [], [], []
    plain = _two_calls(kw, 4, launches=n_plain)
    marked = _two_calls(dict(kw, slim_blocks=True), 4, launches=n_on)
    again = _two_calls(dict(kw, slim_blocks=True), 4)
    marked_off = _two_calls(dict(kw, slim_blocks=True), 4, narrow_out=False, launches=n_off)
    assert n_plain == [] and n_off == [] and sorted(n_on) == [False, False, True, True]
    for (o0, dx0, g0), (o1, dx1, g1), (o2, dx2, g2), (_, dx3, _) in zip(plain, marked, marked_off, again):
        for a, b, c in zip(o0 + tuple(g0), o1 + tuple(g1), o2 + tuple(g2)):
            assert torch.equal(a, b) and torch.equal(a, c)
        assert TC._rel(dx2, dx0.double()) < TOL and TC._rel(dx1, dx0.double()) < TOL
        assert torch.equal(dx1, dx3)


if __name__ == '__main__':
    kinds = ('out', 'dx', 'conv_w', 'bias', 'head')
    print(f"{'critic':<44}{'route':<12}" + ''.join(f"{k:>10}" for k in kinds), flush=True)
    worst = {route: dict.fromkeys(kinds, 0.0) for route in ('hip', 'torch fp32')}
    for name, kw in NETS.items():
        for training in (False, True):
            for route, fast in (('hip', True), ('torch fp32', False)):
                for call, errs in enumerate(TC._critic_errors(kw, NET_BATCH, training, fast)):
                    label = f"{name} {'train call ' + str(call + 1) if training else 'eval'}"
                    print(f"{label:<44}{route:<12}" + ''.join(f"{errs[k]:>10.2e}" for k in kinds), flush=True)
                    for k in kinds:
                        worst[route][k] = max(worst[route][k], errs[k])
    for route in worst:
        print(f"{'worst over the two critics':<44}{route:<12}" + ''.join(f"{worst[route][k]:>10.2e}" for k in kinds), flush=True)
    print(f"{'bound':<44}{'':<12}" + ''.join(f"{BOUNDS[k]:>10.0e}" for k in kinds), flush=True)
    print()
    print(f"{'layer row':<28}{'weight':<16}" + ''.join(f"{n:>10}" for n in ('y', 'dx', 'dw', 'db')))
    for row in ROWS:
        for fmt in FORMATS:
            errs = _row(row, fmt)
            print(f"{ROW_ID(row):<28}{fmt:<16}" + ''.join(f"{errs[n]:>10.2e}" for n in ('y', 'dx', 'dw', 'db')))
    print(f"bounds: y, dx, db {TOL:.0e}; dw {DW_TOL:.0e} of the tensor's maximum against torch's float64 convolution")
