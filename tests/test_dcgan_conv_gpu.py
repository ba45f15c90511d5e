"""The kernel pieces the DCGAN-SN recipes added to wc_gan_amd/conv.py (csrc/wc_conv.hip), against torch's float64 convolution of the same map
with the inputs, `_rel` and TOL of tests/test_conv_gpu.py (y, dx, db < 1e-5, dw < 2e-5: the project's bounds for these kernels):

  * layers with a 64-channel side on the block kernels: the 64-output tile <2, 1> of the forward / data-gradient kernel (with and without the
    shared tap loop) and the 64 x 64 tile <1, 1> of the weight gradient.  `conv.supported` takes such widths for kind 'down' only (the
    recipe's 64 -> 128 layer): every 'down' row goes through the layer entry; the kernels take every geometry with such a width, and the
    rows of the other kinds run them on the plan itself, which the layer entry refuses;
  * the narrow image layer 3 -> 64 at 3x3 (the critic's first layer);
  * the recipe's wide deconvolutions, 512 -> 512 and 512 -> 256 'up' and 256 -> 512 'down';
  * LeakyReLU inside the operand split.
"""
import pytest
import torch
import torch.nn.functional as F

from test_conv_gpu import TOL, _Site, _ref, _rel, _weights

SLOPE = 0.3

# kind, N, H, W, Cin, Cout, k
NARROW_TILE_CASES = [
    ('down', 2, 16, 16, 64, 128, 0),          # the virtual grid is exactly one 128-point tile; the data gradient: 4 phases with Cout = 64
    ('down', 8, 32, 32, 64, 128, 0),          # several tiles, images straddled; the data gradient's tap loop is shared (<2, 1, true>)
    ('down', 2, 16, 16, 128, 64, 0),          # the forward on the 64-output tile
    ('down', 2, 16, 16, 64, 64, 0),           # 64 both ways
    ('down', 2, 16, 16, 64, 192, 0),          # 192 = 128 + 64 outputs
    ('up', 2, 8, 8, 128, 64, 0),              # phases with Cout = 64 in the forward
    ('up', 2, 8, 8, 64, 128, 0),
    ('same', 4, 8, 8, 64, 64, 3),             # 64 both ways: shared tap loop forward and backward, one 64 x 64 weight-gradient tile per tap
    ('same', 16, 32, 32, 64, 64, 3),          # 128 tiles of 128 points: the 64-output tile without the shared tap loop
    ('same', 2, 8, 8, 64, 128, 1),            # 1x1: two iterations, no shared loop
    ('same', 2, 8, 8, 128, 64, 3),
    ('same', 1, 16, 16, 64, 192, 3),          # 192 = 128 + 64: three 64-output tiles; the weight gradient as 1 x 3 tiles of 64 x 64
    ('same', 2, 12, 16, 192, 64, 3),          # a grid that is no power of two
]


def _check_layer(kind, N, H, W, ci, co, k, bias=True):
    from wc_gan_amd import conv as C
    torch.manual_seed(N + H + ci)
    x = (torch.randn(N, H, W, ci, device='cuda') * 1.7 + 0.3).requires_grad_(True)
    w = _weights(kind, ci, co, k).requires_grad_(True)
    b = (torch.randn(co, device='cuda') * 0.1).requires_grad_(True) if bias else None
    narrow = bool(ci % 128 or co % 128)
    plan = C._Plan(kind, N, H, W, tuple(w.shape))
    assert plan.ok                                      # the kernels take the geometry, forward and data gradient
    assert C.supported(x, w, kind) == (kind == 'down' or not narrow)
    if kind == 'down' or not narrow:
        y = C.fast_conv(x, w, b, kind)
    else:                                               # a 64-wide side outside 'down': not a layer call, the kernels on the plan itself
        with pytest.raises(RuntimeError):
            C.fast_conv(x, w, b, kind)
        y = C._FastConv.apply(x, w, b, kind, plan)
    gy = torch.randn_like(y)
    leaves = (x, w) + ((b,) if bias else ())
    got = torch.autograd.grad(y, leaves, gy)
    y64 = _ref(x, w, b, kind)
    want = torch.autograd.grad(y64, leaves, gy.double())
    errs = dict(y=_rel(y, y64), dx=_rel(got[0], want[0]), dw=_rel(got[1], want[1]))
    if bias:
        errs['db'] = _rel(got[2], want[2])
    print(kind, (N, H, W, ci, co, k), {n: f"{v:.2e}" for n, v in errs.items()})
    assert y.shape == y64.shape
    assert errs['y'] < TOL and errs['dx'] < TOL and errs['dw'] < 2e-5 and errs.get('db', 0.0) < TOL, errs


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,H,W,ci,co,k", NARROW_TILE_CASES)
def test_layers_with_a_64_channel_side_match_float64(kind, N, H, W, ci, co, k):
    _check_layer(kind, N, H, W, ci, co, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,H,ci,co", [('down3', 8, 16, 64, 128), ('down3', 8, 16, 128, 64), ('up3', 8, 8, 64, 64), ('up3', 8, 8, 128, 64)])
def test_pooled_and_upsampled_3x3_layers_with_a_64_channel_side(kind, N, H, ci, co):
    """the 'down3' / 'up3' forms (the 4x4 kernels formed from the 3x3 weight inside the image, folded back in the weight gradient) on the
    64-wide tiles"""
    from wc_gan_amd import conv as C
    torch.manual_seed(N + H + ci)
    x = (torch.randn(N, H, H, ci, device='cuda') * 1.3 - 0.2).requires_grad_(True)
    w = _weights('same', ci, co, 3).requires_grad_(True)
    b = (torch.randn(co, device='cuda') * 0.1).requires_grad_(True)
    plan = C._Plan(kind, N, H, H, tuple(w.shape))
    assert plan.ok and not C.supported(x, w, kind)      # the kernels take it; the layer entry keeps 64-wide sides to kind 'down'
    y = C._FastConv.apply(x, w, b, kind, plan)
    xn = x.permute(0, 3, 1, 2).double()
    if kind == 'down3':
        y64 = F.avg_pool2d(F.conv2d(xn, w.double(), b.double(), padding=1), 2).permute(0, 2, 3, 1)
    else:
        y64 = F.conv2d(F.interpolate(xn, scale_factor=2, mode='nearest'), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    gy = torch.randn_like(y)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gy)
    dx64, dw64, db64 = torch.autograd.grad(y64, (x, w, b), gy.double())
    assert _rel(y, y64) < TOL and _rel(dx, dx64) < TOL and _rel(dw, dw64) < 2e-5 and _rel(db, db64) < TOL


@pytest.mark.gpu
def test_widths_that_are_no_multiple_of_64_stay_refused():
    """`supported` is exact: 32 and 96 channels on either side are not taken by the kernels (the data gradient would produce them), for
    no kind; and outside kind 'down' a 64-wide side is not taken by the layer entry"""
    from wc_gan_amd import conv as C
    for ci, co in ((32, 128), (128, 32), (96, 128), (128, 96), (64, 32)):
        x = torch.randn(8, 16, 16, ci, device='cuda')        # (2048 / 512 grid points: the widths are what is refused)
        assert not C.supported(x, _weights('same', ci, co, 3), 'same'), (ci, co)
        assert not C.supported(x, _weights('down', ci, co, 0), 'down'), (ci, co)
        assert not C._Plan('down', 8, 16, 16, (co, ci, 4, 4)).ok
    for kind, ci, co in (('same', 64, 64), ('same', 64, 128), ('up', 128, 64), ('up3', 64, 64), ('down3', 64, 128)):
        x = torch.randn(8, 16, 16, ci, device='cuda')
        assert not C.supported(x, _weights('same' if kind.endswith('3') else kind, ci, co, 3), kind), (kind, ci, co)
        assert not C.takes_planes(x.shape, _weights('same' if kind.endswith('3') else kind, ci, co, 3).shape, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,H,W,ci,co", [('up', 8, 4, 4, 512, 512), ('up', 8, 8, 8, 512, 256), ('down', 8, 8, 8, 256, 512)])
def test_the_recipes_wide_deconvolutions_match_float64(kind, N, H, W, ci, co):
    _check_layer(kind, N, H, W, ci, co, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", [(2, 16, 16), (8, 32, 32)])
@pytest.mark.parametrize("bias", [True, False])
def test_narrow_image_layer_to_64_channels(N, H, W, bias):
    """3 -> 64 at 3x3 through the narrow kernels (forward, weight and bias gradient on the fp32 matrix pipe): the upper half of the one
    128-channel group has no channels"""
    from wc_gan_amd import conv as C
    torch.manual_seed(N + H)
    x = torch.rand(N, H, W, 3, device='cuda') * 2 - 1
    w = _weights('same', 3, 64, 3).requires_grad_(True)
    b = (torch.randn(64, device='cuda') * 0.1).requires_grad_(True) if bias else None
    assert C.narrow_wrw_supported(x, w) and not C.supported(x, w, 'same')
    y = C.narrow_in_conv(x, w, b)
    gy = torch.randn_like(y)
    leaves = (w,) + ((b,) if bias else ())
    got = torch.autograd.grad(y, leaves, gy)
    y64 = _ref(x, w, b, 'same')
    want = torch.autograd.grad(y64, leaves, gy.double())
    assert y.shape == y64.shape == (N, H, W, 64)
    assert _rel(y, y64) < TOL and _rel(got[0], want[0]) < 2e-5
    if bias:
        assert _rel(got[1], want[1]) < TOL


def _leaky_inputs(kind, N, H, ci, co, seed):
    torch.manual_seed(seed)
    x = torch.randn(N, H, H, ci, device='cuda') * 1.7 - 0.4
    x[torch.rand_like(x) < 0.05] = 0.0                  # exact zeros: the gradient convention there is slope * g
    x.view(-1)[0] = -9.0                                # the largest magnitude is a NEGATIVE element: the scale must be the activated tensor's
    k = 0 if kind == 'down' else 3
    w = _weights(kind, ci, co, k)
    b = torch.randn(co, device='cuda') * 0.1
    assert bool((x == 0).any()) and bool((x > 0).any()) and bool((x < 0).any())
    return x, w, b


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,H,ci,co", [('same', 8, 16, 128, 128), ('down', 8, 16, 64, 128)])
def test_leaky_relu_in_the_split_equals_leaky_relu_then_the_layer(kind, N, H, ci, co):
    """conv(leaky(x)) as one call (the activation while x is split, its backward one launch over dx) against F.leaky_relu followed by the
    plain call: without a site history the planes are the same bits, so y and dW are equal, and dx differs by the rounding of the one
    multiplication by the slope on either side: two fp32 roundings (2 x 2^-24 relative) per element.  And both against float64."""
    from wc_gan_amd import conv as C
    x0, w0, b0 = _leaky_inputs(kind, N, H, ci, co, 21)
    x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
    y = C.fast_conv_or_none(x, w, b, kind, leaky_input=SLOPE)
    gy = torch.randn_like(y)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gy)
    x2, w2, b2 = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
    y2 = C.fast_conv_or_none(F.leaky_relu(x2, SLOPE), w2, b2, kind)
    dx2, dw2, db2 = torch.autograd.grad(y2, (x2, w2, b2), gy)
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert bool(((dx - dx2).abs() <= 2.0 ** -23 * dx2.abs()).all())
    x3, w3, b3 = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
    y64 = _ref(F.leaky_relu(x3.double(), SLOPE), w3, b3, kind)
    dx64, dw64, db64 = torch.autograd.grad(y64, (x3, w3, b3), gy.double())
    assert _rel(y, y64) < TOL and _rel(dx, dx64) < TOL and _rel(dw, dw64) < 2e-5 and _rel(db, db64) < TOL
    zero = x0 == 0
    assert bool(zero.any()) and _rel(dx[zero], dx64[zero]) < TOL          # x == 0 gets slope * g, torch's convention


@pytest.mark.gpu
@pytest.mark.parametrize("with_site", [False, True])
def test_slope_zero_is_the_relu_bit_for_bit(with_site):
    from wc_gan_amd import conv as C
    x0, w0, b0 = _leaky_inputs('same', 8, 16, 128, 128, 22)
    outs = []
    for mode in ('leaky', 'relu'):
        site = _Site() if with_site else None
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        res = []
        for call in range(2 if with_site else 1):           # with a site: the measuring call, then a history-scaled one
            kw = dict(leaky_input=0.0) if mode == 'leaky' else dict(relu_input=True)
            y = C.fast_conv_or_none(x * (1.0 + call), w, b, 'same', site=site, **kw)
            torch.manual_seed(5 + call)
            gy = torch.randn_like(y)
            res += [y, *torch.autograd.grad(y, (x, w, b), gy)]
        outs.append(res)
    for a, r in zip(*outs):
        assert torch.equal(a, r)
    planes_l, planes_r = C.split_planes(x0, leaky=0.0), C.split_planes(x0, relu=True)
    assert all(torch.equal(a, r) for a, r in zip((planes_l[0], planes_l[1], planes_l[2][:1]), (planes_r[0], planes_r[1], planes_r[2][:1])))


@pytest.mark.gpu
def test_history_scaled_leaky_split_gives_the_same_bits_eagerly_and_from_a_graph():
    """the pattern of test_conv_gpu's test for the plain split: three calls replayed from one hipGraph (twice) equal the same six calls made
    eagerly on a fresh site -- with the activation in the split and the column sums beside it"""
    from wc_gan_amd import conv as C
    torch.manual_seed(6)
    xs = [torch.randn(16, 16, 16, 128, device='cuda') * f - 0.2 * f for f in (1.0, 7.0, 0.05, 3.0, 3.0, 0.5, 11.0)]
    for x in xs:
        x[torch.rand_like(x) < 0.05] = 0.0
    eager_site, graph_site = _Site(), _Site()
    eager = [C.split_planes(x, site=eager_site, leaky=SLOPE, colsum=True) for x in xs]
    first = C.split_planes(xs[0], site=graph_site, leaky=SLOPE, colsum=True)          # the measuring call, eager on both sides
    buf = [torch.empty_like(xs[0]) for _ in range(3)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [C.split_planes(b, site=graph_site, leaky=SLOPE, colsum=True) for b in buf]
    assert torch.equal(first[0], eager[0][0])
    for rep in range(2):
        for b, x in zip(buf, xs[1 + 3 * rep: 4 + 3 * rep]):
            b.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            e = eager[1 + 3 * rep + k]
            assert torch.equal(o[0], e[0]) and torch.equal(o[1], e[1]) and torch.equal(o[2][:1], e[2][:1]) and torch.equal(o[3], e[3]), (rep, k)
    # what the planes hold is the activated tensor, to the split's 2^-20 of its maximum
    x = xs[6]
    back = (eager[6][0].double() + eager[6][1].double()) / float(eager[6][2][0])
    want = F.leaky_relu(x.double(), SLOPE)
    assert float((back - want).abs().max() / want.abs().max()) < 2.0 ** -20
    assert _rel(eager[6][3].sum(0), x.double().sum((0, 1, 2))) < TOL                  # the column sums are of x as given
