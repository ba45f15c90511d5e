"""Convolutions of the residual blocks either side of the WC sites on the split-fp16 MFMA path (csrc/wc_conv.hip).

`fast_conv(x, w, bias, kind)` on NHWC tensors:

    kind 'same'  Keras `Conv2D(k x k, padding='same')`, w (Cout, Cin, k, k)          generator.py:142-158
    kind 'down'  4x4 stride-2 padding-1 convolution, w (Cout, Cin, 4, 4)              (= Conv2D 3x3 -> AveragePooling2D, discriminator.py:41-54)
    kind 'up'    4x4 stride-2 padding-1 TRANSPOSED convolution, w (Cin, Cout, 4, 4)   (= UpSampling2D -> Conv2D 3x3, generator.py:144-151)
    kind 'down3' / 'up3'  the same two layers given the 3x3 weight (Cout, Cin, 3, 3) itself: the 4x4 kernels are sums of 3x3
                 taps, formed while the weight image is built and folded back in the weight gradient

Forward and the data gradient run on the HIP kernel (the data gradient of 'same' is a 'same', of 'down' an 'up' and of
'up' a 'down', with the channel roles swapped in the weight image), and so does the weight gradient (pixel-major tiles
read back through gfx950's transposing LDS read).  `relu_input` / `leaky_input` (fast_conv_or_none): the layer is conv(relu(x)) /
conv(leaky_relu(x, slope)) and the activation happens while x is split.  Channel widths: multiples of 128, of 64 for 'down' -- of 32 for
'same' and 'up3' in a layer built with slim_conv=True (`slim=` here), of 64 for 'same' and 'down3' in a critic
layer built with slim_blocks=True (`blocks=` here; section 4.23).  N*H*W of the virtual grid (the output's
for 'down' / 'down3', the input's otherwise): a multiple of 128, or -- for a layer built with ragged_conv=True (`ragged=` here) -- of 32:
the last 128-point tile is then partial.  No fallback inside: `supported(...)` tells the caller whether the
kernel takes a shape.
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F

from . import _lib, _state
from .ops import _ptr, _stream

_zero_lines = {}


def _zero_line(device):
    z = _zero_lines.get(device)
    if z is None:
        z = _zero_lines[device] = torch.zeros(64, dtype=torch.uint8, device=device)
    return z


def _plain(r, s):
    return [(r, s)], 1.0


def _pooled3(r, s):
    """4x4 stride-2 kernel of Conv2D 3x3 -> AveragePooling2D: tap (r, s) = 1/4 of the 3x3 taps (r - a, s - b), a, b in {0, 1}"""
    return [(r - a, s - b) for a in (0, 1) for b in (0, 1) if 0 <= r - a <= 2 and 0 <= s - b <= 2], 0.25


_UP_ROWS = ((2,), (1, 2), (0, 1), (0,))


def _upsampled3(r, s):
    """4x4 stride-2 transposed kernel of UpSampling2D -> Conv2D 3x3: rows [w2, w1 + w2, w0 + w1, w0] along each axis"""
    return [(r3, s3) for r3 in _UP_ROWS[r] for s3 in _UP_ROWS[s]], 1.0


def _set_sources(g, p, t, r, s, source):
    taps, coef = source(r, s)
    g.nsrc[p][t] = len(taps)
    for m, (r3, s3) in enumerate(taps):
        g.wr[p][t][m], g.ws[p][t][m] = r3, s3
    g.wcoef = coef


def _dense_geom(N, Hin, Win, Cin, Cout, k, stride, source=_plain):
    """taps (r, s) read input (y*stride + r - pad, x*stride + s - pad); pad = k//2 for 'same', 1 for the 4x4 stride-2 form"""
    pad = k // 2 if stride == 1 else 1
    g = _lib.ConvGeom()
    g.N, g.Hin, g.Win, g.Cin, g.Cout = N, Hin, Win, Cin, Cout
    g.H, g.W = Hin // stride, Win // stride
    g.Hout, g.Wout = g.H, g.W
    g.in_stride, g.out_stride, g.ntaps, g.nphase = stride, 1, k * k, 1
    for r in range(k):
        for s in range(k):
            t = r * k + s
            g.dy[0][t], g.dx[0][t] = r - pad, s - pad
            _set_sources(g, 0, t, r, s, source)
    return g


def _phase_geom(N, Hin, Win, Cin, Cout, source=_plain):
    """4x4 stride-2 padding-1 transposed convolution as four 2x2 sub-pixel convolutions: output (2y+py, 2x+px) reads
    input (y+dy, x+dx) through weight tap r = py + 1 - 2 dy"""
    g = _lib.ConvGeom()
    g.N, g.Hin, g.Win, g.Cin, g.Cout = N, Hin, Win, Cin, Cout
    g.H, g.W, g.Hout, g.Wout = Hin, Win, 2 * Hin, 2 * Win
    g.in_stride, g.out_stride, g.ntaps, g.nphase = 1, 2, 4, 4
    for py in range(2):
        for px in range(2):
            p = py * 2 + px
            g.off_y[p], g.off_x[p] = py, px
            t = 0
            for dy in ((-1, 0) if py == 0 else (0, 1)):
                for dx in ((-1, 0) if px == 0 else (0, 1)):
                    g.dy[p][t], g.dx[p][t] = dy, dx
                    _set_sources(g, p, t, py + 1 - 2 * dy, px + 1 - 2 * dx, source)
                    t += 1
    return g


def _supported(g):
    return bool(_lib.load().wc_conv_supported(ctypes.addressof(g)))


def _ragged(site):
    """Has the layer object opted in to a partial last tile (make_generator / make_discriminator(ragged_conv=True))?"""
    return bool(getattr(site, 'ragged_conv', False))


def _slim(site):
    """Has the layer object opted in to the 64- and 32-channel tiles (make_generator(slim_conv=True))?"""
    return bool(getattr(site, 'slim_conv', False))


def _blocks(site):
    """Has the layer object opted in to the critic's 64-wide block layers (make_discriminator(slim_blocks=True))?"""
    return bool(getattr(site, 'slim_blocks', False))


def supported(x, w, kind, ragged=False, slim=False, blocks=False):
    """Does the kernel take this call?  (channels multiples of 128 -- of 64 for kind 'down' --, N*H*W of the virtual grid a multiple of 128;
    ragged, the opt-in of a layer marked ragged_conv: a multiple of 32, the last tile partial -- wc_conv_ragged_supported;
    slim, the opt-in of a layer marked slim_conv: channels multiples of 32 on whole tiles -- wc_conv_slim_supported;
    blocks, the opt-in of a layer marked slim_blocks: the critic's kinds 'same' and 'down3' at widths that are multiples of 64)"""
    handed = getattr(x, '_wc_planes', None) is not None       # a K3 handle: the data is in the planes it carries
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (handed or x.is_contiguous()) and w.dtype == torch.float32):
        return False
    p = _plan(kind, x, w, ragged, slim, blocks)
    return bool(p) and p.ok


class _Plan:
    """Everything about a call that depends on the shapes only, built once: the two geometries, the weight axes, the
    support verdict and the workspace sizes (the per-call host work is what is left: a few allocations and launches)."""
    __slots__ = ('ok', 'fwd', 'bwd', 'fwd_ws', 'bwd_ws', 'wrw_ws', 'fwd_ptr', 'bwd_ptr', 'pair', 'res', 'tail', 'bwd_tail', 'local',
                 'bwd_local')

    def __init__(self, kind, N, H, W, wshape, ragged=False, slim=False):
        class _W:                                 # shape-only stand-in for the weight
            shape = wshape
        lib = _lib.load()
        (gf, kf, nf), (gb, kb, nb) = _geoms(kind, N, H, W, _W)
        self.fwd, self.bwd = (gf, kf, nf), (gb, kb, nb)
        self.fwd_ptr, self.bwd_ptr = ctypes.addressof(gf), ctypes.addressof(gb)
        # ragged: the layer opted in to a partial last tile (N*H*W a multiple of 32); without it the answer is the one it always was
        takes = lib.wc_conv_ragged_supported if ragged else lib.wc_conv_supported
        self.ok = bool(takes(self.fwd_ptr)) and bool(takes(self.bwd_ptr))
        # slim: the layer opted in to channel widths that are multiples of 32, on whole tiles.  A layer marked
        # both ways is taken where either set takes both geometries: a slim width on a partial last tile is in neither
        if slim and not self.ok:
            self.ok = bool(lib.wc_conv_slim_supported(self.fwd_ptr)) and bool(lib.wc_conv_slim_supported(self.bwd_ptr))
        self.fwd_ws = lib.wc_conv_workspace_bytes(self.fwd_ptr) if self.ok else 0
        self.bwd_ws = lib.wc_conv_workspace_bytes(self.bwd_ptr) if self.ok else 0
        self.wrw_ws = lib.wc_conv_wrw_workspace_bytes(self.fwd_ptr) if self.ok else 0
        # data gradient and weight gradient in one grid (wc_conv_bwd_pair_f16x3): the critic's 128-channel layers
        self.pair = self.ok and bool(lib.wc_conv_bwd_pair_supported(self.bwd_ptr, self.fwd_ptr))
        # a residual operand in the forward's finish (wc_conv_res_f16x3): the layers whose tap loop is shared over workgroups
        self.res = self.ok and bool(lib.wc_conv_res_supported(self.fwd_ptr))
        # a finish launch that can go on to its follower's work (wc_conv_tail_f16x3): the forward's, the data gradient's
        self.tail = self.ok and bool(lib.wc_conv_tail_supported(self.fwd_ptr))
        self.bwd_tail = self.ok and bool(lib.wc_conv_tail_supported(self.bwd_ptr))
        # the k-split's shares summed inside the workgroup (wc_conv_local_f16x3): one launch where run / run_tail issued two (LOCAL_KSPLIT)
        self.local = self.ok and bool(lib.wc_conv_local_supported(self.fwd_ptr))
        self.bwd_local = self.ok and bool(lib.wc_conv_local_supported(self.bwd_ptr))


_plans = {}


def _plan(kind, x, w, ragged=False, slim=False, blocks=False):
    # (an unmarked layer's key is the four-field one it always was; the slim mark adds a field, the slim_blocks mark a further one)
    key = (kind, tuple(x.shape), tuple(w.shape), bool(ragged)) + ((True,) if slim else ()) + (('blocks',) if blocks else ())
    p = _plans.get(key)
    if p is None:
        N, H, W, C = x.shape
        good = (kind == 'same' and w.shape[1] == C and w.shape[2] == w.shape[3] and w.shape[2] in (1, 3)) or \
               (kind == 'down' and w.shape[1] == C and tuple(w.shape[2:]) == (4, 4) and H % 2 == 0 and W % 2 == 0) or \
               (kind == 'down3' and w.shape[1] == C and tuple(w.shape[2:]) == (3, 3) and H % 2 == 0 and W % 2 == 0) or \
               (kind == 'up3' and w.shape[1] == C and tuple(w.shape[2:]) == (3, 3)) or \
               (kind == 'up' and w.shape[0] == C and tuple(w.shape[2:]) == (4, 4))
        if kind not in ('same', 'down', 'up', 'down3', 'up3'):
            raise ValueError(kind)
        # A width that is 64 beyond a multiple of 128 (the kernels' 64-wide tiles): the layer entry takes it for the plain 4x4 stride-2
        # convolution only -- the DC critic's 64 -> 128 layer.  The kernels take every geometry with such a width (_Plan.ok says so, and
        # tests/test_dcgan_conv_gpu.py runs them); the 64-wide ResNet blocks of toy configurations stay on their other path, as before.
        # A layer marked slim_conv drops this rule for the generator's kinds: its 64-wide layers reach the kernels they always had, its
        # 32-wide ones the 32-output and 32 x 32 tiles (wc_conv_slim_supported answers for both geometries).
        # A layer marked slim_blocks (make_discriminator(slim_blocks=True)) drops it for the critic's kinds where
        # every width is a multiple of 64: the verdict is wc_conv_supported's (wc_conv_ragged_supported's with ragged), as for any layer.
        wide64 = not (C % 64 or w.shape[0] % 64 or w.shape[1] % 64)
        if good and kind != 'down' and (C % 128 or w.shape[0] % 128 or w.shape[1] % 128) and not (slim and kind in ('same', 'up3')) \
                and not (blocks and kind in ('same', 'down3') and wide64):
            good = False
        p = _plans[key] = _Plan(kind, N, H, W, tuple(w.shape), bool(ragged), bool(slim)) if good else False
    return p


def _colsum_ok(C):
    return C % 4 == 0 and 256 % (C // 4) == 0


# The split's scale from the call before at the same call site (wc_conv_split_hist_f32: one launch instead of absmax + split; nothing clamps,
# an element that does not fit goes inf = loud).  Training-mode layers only: an eval-mode pass measures every tensor, so that the images of a
# loaded checkpoint do not depend on what the process ran before.  WC_SPLIT_HIST=0: the measured maximum everywhere, two launches (rounds 1-4).
SPLIT_HIST = os.environ.get('WC_SPLIT_HIST', '1') != '0'
HIST_FLOATS = 4 * 512 + 16     # include/wc_hip.h WC_CONV_HIST_FLOATS
HIST_REDO = 4 * 512            # WC_CONV_HIST_REDO: uint32 count of the gated second passes a site has taken


# The gated second pass of the history-scaled split (include/wc_hip.h, wc_conv_split_hist_f32): WC_SPLIT_HIST_REDO = 1 (default) for the
# output gradients only (role 'g', and the gradient penalty's 't' and 'd'), 2 for every split, 0 for none.  (Every split of the step: +0.56 ms of 18 -- what the history saves.)
_REDO_MODE = os.environ.get('WC_SPLIT_HIST_REDO', '1')


def _guarded(role):
    # 't' / 'd': the tangents and adjoints of the gradient penalty (penalty.py) scale with | ||grad D|| - 1 |: orders of magnitude between calls
    return _REDO_MODE == '2' or (_REDO_MODE != '0' and role in ('g', 't', 'd'))


def _site_hist(site, role, device):
    """[record (HIST_FLOATS floats on the device: two arrays of per-workgroup (maximum, tag) pairs), seeded?] of a call site:
    `site` is the layer object that owns the convolution (state lives in its __dict__, not in a parameter or buffer: no checkpoint entry --
    a resumed run measures once), role 'x' (its input) or 'g' (its output gradient); the gradient penalty (penalty.py) keeps records of its own
    at the same sites -- 'p' (the primal input at the interpolates), 't' (the tangent), 'd' (the adjoint) -- so that 'x' and 'g' never see it.  None for a layer in eval mode, and while a hipGraph is
    being recorded for a site that has no record yet (no allocation into a graph's private pool; the trainers warm up eagerly first)."""
    if not getattr(site, 'training', True):
        return None
    book = site.__dict__.setdefault('_wc_split_hist', {})
    h = book.get(role)
    if h is not None and h[0].device != device:     # the layer moved to another device: a fresh record there (its first call measures)
        h = None
    if h is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        h = book[role] = [torch.zeros(HIST_FLOATS, dtype=torch.float32, device=device), False]
    return h


def split_planes(x, relu=False, colsum=False, site=None, role='x', leaky=None):
    """fp32 tensor -> (hi, lo, scale): fp16 planes of s*x and the device scalar s.  colsum: also the 512 partial rows of the
    column sums over the last axis (-> the bias gradient, finished by weight_gradient), returned as a 4th element.
    site (+ role): the layer object this tensor belongs to -- the scale then comes from the previous call of that site (one launch).
    leaky: a negative slope in [0, 1] -- the planes are of LeakyReLU(x) (x > 0 ? x : slope * x); slope 0 gives the bits of relu=True."""
    lib = _lib.load()
    if leaky is not None:
        if relu:
            raise ValueError("relu and leaky are two activations")
        return _split_planes_leaky(lib, x, float(leaky), colsum, site, role)
    both = torch.empty((2,) + tuple(x.shape), dtype=torch.float16, device=x.device)
    hi, lo = both[0], both[1]
    scale = torch.empty(1 + 512, dtype=torch.float32, device=x.device)    # [scale | per-workgroup maxima scratch]
    h = _site_hist(site, role, x.device) if (SPLIT_HIST and site is not None) else None
    if h is not None:
        C = x.shape[-1]
        part = torch.empty((512, C), dtype=torch.float32, device=x.device) if colsum else None
        _lib.check(lib.wc_conv_split_hist_f32(_ptr(x), x.numel(), 1 if relu else 0, _ptr(hi), _ptr(lo), _ptr(scale), _ptr(part), C if colsum else 0,
                                              _ptr(h[0]), (0 if h[1] else 1) | (0 if _guarded(role) else 2), _stream()), "wc_conv_split_hist_f32")
        h[1] = True
        return (hi, lo, scale, part) if colsum else (hi, lo, scale)
    if not colsum:
        _lib.check(lib.wc_conv_split_f32(_ptr(x), x.numel(), 1 if relu else 0, _ptr(hi), _ptr(lo), _ptr(scale),
                                         scale.data_ptr() + 4, _stream()), "wc_conv_split_f32")
        return hi, lo, scale
    C = x.shape[-1]
    part = torch.empty((512, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.wc_conv_split_colsum_f32(_ptr(x), x.numel(), 1 if relu else 0, _ptr(hi), _ptr(lo), _ptr(scale),
                                            scale.data_ptr() + 4, _ptr(part), C, _stream()), "wc_conv_split_colsum_f32")
    return hi, lo, scale, part


def _split_planes_leaky(lib, x, slope, colsum, site, role):
    both = torch.empty((2,) + tuple(x.shape), dtype=torch.float16, device=x.device)
    hi, lo = both[0], both[1]
    scale = torch.empty(1 + 512, dtype=torch.float32, device=x.device)
    C = x.shape[-1]
    part = torch.empty((512, C), dtype=torch.float32, device=x.device) if colsum else None
    h = _site_hist(site, role, x.device) if (SPLIT_HIST and site is not None) else None
    if h is not None:
        _lib.check(lib.wc_conv_split_hist_leaky_f32(_ptr(x), x.numel(), slope, _ptr(hi), _ptr(lo), _ptr(scale), _ptr(part), C if colsum else 0,
                                                    _ptr(h[0]), (0 if h[1] else 1) | (0 if _guarded(role) else 2), _stream()),
                   "wc_conv_split_hist_leaky_f32")
        h[1] = True
    else:
        _lib.check(lib.wc_conv_split_leaky_f32(_ptr(x), x.numel(), slope, _ptr(hi), _ptr(lo), _ptr(scale), scale.data_ptr() + 4,
                                               _ptr(part), C if colsum else 0, _stream()), "wc_conv_split_leaky_f32")
    return (hi, lo, scale, part) if colsum else (hi, lo, scale)


def split_planes_masked(t, a, slope=0.0, site=None, role='t', colsum=False):
    """(hi, lo, scale) of t * (a > 0 ? 1 : slope) -- a tangent behind a ReLU (slope 0) or LeakyReLU whose primal pre-activation was `a` --
    in the launches of split_planes and with its bits on the premultiplied tensor (wc_conv_split[_hist]_masked_f32, csrc/wc_gp.hip).
    site / role as in split_planes; roles 't' and 'g' take the gated second pass.  colsum: as in split_planes, the partial rows of the
    column sums of the masked values as a 4th element (the critic block's backward: t = conv2's data gradient, a = conv1's output)."""
    if not (t.is_contiguous() and a.is_contiguous() and t.shape == a.shape and t.dtype == a.dtype == torch.float32):
        raise ValueError("split_planes_masked: dense fp32 tensors of one shape")
    lib = _lib.load()
    both = torch.empty((2,) + tuple(t.shape), dtype=torch.float16, device=t.device)
    hi, lo = both[0], both[1]
    scale = torch.empty(1 + 512, dtype=torch.float32, device=t.device)
    C = t.shape[-1]
    part = torch.empty((512, C), dtype=torch.float32, device=t.device) if colsum else None
    h = _site_hist(site, role, t.device) if (SPLIT_HIST and site is not None) else None
    if h is not None:
        _lib.check(lib.wc_conv_split_hist_masked_f32(_ptr(t), _ptr(a), t.numel(), float(slope), _ptr(hi), _ptr(lo), _ptr(scale),
                                                     _ptr(part), C if colsum else 0, _ptr(h[0]),
                                                     (0 if h[1] else 1) | (0 if _guarded(role) else 2), _stream()),
                   "wc_conv_split_hist_masked_f32")
        h[1] = True
    else:
        _lib.check(lib.wc_conv_split_masked_f32(_ptr(t), _ptr(a), t.numel(), float(slope), _ptr(hi), _ptr(lo), _ptr(scale),
                                                scale.data_ptr() + 4, _ptr(part), C if colsum else 0, _stream()), "wc_conv_split_masked_f32")
    return (hi, lo, scale, part) if colsum else (hi, lo, scale)


def block_input_gradient(dx1, x, other, down):
    """(x > 0 ? dx1 : 0) + other, or + 0.25 * other[n, y/2, x/2, c] when `down` (other at half resolution: the gradient in front of the
    block's 2x2 average pooling) -- threshold_backward, avg_pool2d's backward and the add that joins a critic block's two branches in one
    launch and with their bits (wc_conv_block_dx_f32).  NHWC fp32."""
    N, H, W, C = dx1.shape
    want = (N, H // 2, W // 2, C) if down else (N, H, W, C)
    if not (dx1.is_contiguous() and x.is_contiguous() and other.is_contiguous() and x.shape == dx1.shape and tuple(other.shape) == want
            and dx1.dtype == x.dtype == other.dtype == torch.float32):
        raise ValueError("block_input_gradient: dense fp32 NHWC tensors, `other` of dx1's shape (at half resolution when down)")
    out = torch.empty_like(dx1)
    _lib.check(_lib.load().wc_conv_block_dx_f32(_ptr(dx1), _ptr(x), _ptr(other), N, H, W, C, 1 if down else 0, _ptr(out), _stream()),
               "wc_conv_block_dx_f32")
    return out


def leaky_backward_(dx, x, slope):
    """dx *= (x > 0 ? 1 : slope) in place, one launch (wc_conv_leaky_bwd_f32): the LeakyReLU of conv(leaky(x)) on the data gradient"""
    if not (dx.is_contiguous() and x.is_contiguous() and dx.shape == x.shape and dx.dtype == x.dtype == torch.float32):
        raise ValueError("leaky_backward_: dense fp32 tensors of one shape")
    _lib.check(_lib.load().wc_conv_leaky_bwd_f32(_ptr(dx), _ptr(x), dx.numel(), float(slope), _stream()), "wc_conv_leaky_bwd_f32")
    return dx


def _storage_extent(w):
    return 1 + sum((n - 1) * s for n, s in zip(w.shape, w.stride()))


def weight_image(w, geom, k_axis, n_axis, site=None):
    """Fragment image of a (dense) 4-d weight for a geometry; k_axis / n_axis = which axis is reduced / produced.
    site: the layer object whose own weight w is -- the image prepare_images() built for it in this pass is picked up (see there)."""
    if site is not None:
        got = _pick_up(site, w, ((geom, k_axis, n_axis),))
        if got is not None:
            return got
    lib = _lib.load()
    nbytes = lib.wc_conv_weights_bytes(ctypes.addressof(geom))
    img = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    scale = torch.empty(1 + 512, dtype=torch.float32, device=w.device)
    ext = _storage_extent(w)
    if ext != w.numel():
        raise ValueError("weight must be dense")
    known = getattr(w, '_wc_amax', None)        # floats whose maximum is max|w| (left by the spectral-norm op): no sweep here
    _lib.check(lib.wc_conv_weights_f32(_ptr(w), w.stride(k_axis), w.stride(n_axis), w.stride(2), w.stride(3), ext,
                                       ctypes.addressof(geom), _ptr(img), _ptr(scale), scale.data_ptr() + 4,
                                       _ptr(known), 0 if known is None else known.numel(), _stream()),
               "wc_conv_weights_f32")
    return img, scale


def weight_image_pair(w, fwd, bwd, site=None):
    """The forward and the data-gradient image of one weight in one launch; fwd / bwd = (geometry, k_axis, n_axis).  site: as in weight_image."""
    if site is not None:
        got = _pick_up(site, w, (fwd, bwd))
        if got is not None:
            return got
    lib = _lib.load()
    (ga, ka, na), (gb, kb, nb) = fwd, bwd
    img_a = torch.empty(lib.wc_conv_weights_bytes(ctypes.addressof(ga)), dtype=torch.uint8, device=w.device)
    img_b = torch.empty(lib.wc_conv_weights_bytes(ctypes.addressof(gb)), dtype=torch.uint8, device=w.device)
    scale = torch.empty(2 + 512, dtype=torch.float32, device=w.device)
    ext = _storage_extent(w)
    if ext != w.numel():
        raise ValueError("weight must be dense")
    known = getattr(w, '_wc_amax', None)
    _lib.check(lib.wc_conv_weights_pair_f32(_ptr(w), w.stride(2), w.stride(3), ext,
                                            w.stride(ka), w.stride(na), ctypes.addressof(ga), _ptr(img_a),
                                            w.stride(kb), w.stride(nb), ctypes.addressof(gb), _ptr(img_b),
                                            _ptr(scale), scale.data_ptr() + 8, _ptr(known), 0 if known is None else known.numel(),
                                            _stream()), "wc_conv_weights_pair_f32")
    return (img_a, scale[0:1]), (img_b, scale[1:2])


def _cached_image(w, key, geom, k_axis, n_axis):
    """The image is rebuilt on every call (two small launches).  It used to be cached on the weight tensor per
    `w._version` -- but fused optimizers (torch's fused Adam) and replayed hipGraphs update weights WITHOUT moving that
    counter, and a stale image is a silently wrong convolution; the reuse it bought (the generator's 7 weights, twice per
    step) was ~0.1 ms."""
    return weight_image(w, geom, k_axis, n_axis)


# ---- a pass's weight images in one launch -------------------------------------------------------------------------------------------------
# The images depend on the weights only, yet each was a launch of its own between its layer's split and its convolution, on a chain of
# dependent dispatches (8 per critic pass).  As spectral.prepare_spectral does for the normalised weights, a network builds them at
# the top of its pass: the first pass under a key (pass_key: what fixes which images a pass asks for) LOGS the requests that name their
# layer; later passes under that key build every logged image from the weights as they are THEN (build_images: one launch, plus one for
# the maxima of weights no spectral norm has measured) and leave them on the layers, which pick them up once.  Nothing outlives its pass:
# no per-version cache (see _cached_image), so fused Adam and replayed hipGraphs, which move weights without moving `_version`, cannot meet
# a stale image -- a replayed graph replays the build, in front of its layers, on the updated weights.  A layer takes a prepared image only
# if it was built from the very tensor object the layer holds, for the very geometry object it asks with; otherwise it builds its own as
# before, so a wrong or stale log costs launches and nothing else (and is dropped, to be logged again).  BATCH_IMAGES = False: every layer
# builds its own (tests and tools compare the two in one process).
# The critic prepares (discriminator.Discriminator.forward).  The generator does not: with its forward prepared the same way the step was
# 0.04-0.1 ms SLOWER than without (profiles/image_batch_step_ab.txt; the cause was not looked for -- its passes run beside the critic on
# a second stream, or put their shortcuts on one, so its per-layer launches are not on one chain as the critic's are).
BATCH_IMAGES = True
_recording = None           # (root, key, entries) while a pass without a log runs
_prepared = None            # [root, key, missed] while a pass with prepared images runs


def pass_key(root, x):
    return (tuple(x.shape), torch.is_grad_enabled(), bool(x.requires_grad), root.training,
            tuple(p.requires_grad for p in root.parameters()))


def _own_weight(site):
    """The weight tensor a layer will hand to its convolution in this pass, without taking it: the parameter itself, or what
    prepare_spectral left for the layer to pick up (None when nothing valid is waiting: the layer then normalises, and builds, on its own)."""
    conv = getattr(site, 'conv', None)
    if conv is None:
        return None
    if hasattr(conv, 'normalized_weight'):
        ready = getattr(conv, '_w_ready', None)
        if ready is None or ready[1] != conv.weight._version or ready[2] != conv.training:
            return None
        return ready[0]
    return conv.weight


def _same_geoms(a, b):
    return len(a) == len(b) and all(p[0] is q[0] and p[1] == q[1] and p[2] == q[2] for p, q in zip(a, b))


def build_images(requests):
    """requests: [(weight, ((geometry, k_axis, n_axis), ...one or two...))] -> per request a tuple of (image, scale) per geometry, with the
    bits of weight_image / weight_image_pair: wc_conv_weights_batch_f32 behind, where a weight's maximum is neither known nor taken inside
    its job, one wc_conv_absmax_batch_f32.  All images of the call share one allocation."""
    lib = _lib.load()
    dev = requests[0][0].device
    sizes = [[lib.wc_conv_weights_bytes(ctypes.addressof(g[0])) for g in geoms] for _, geoms in requests]
    njobs = sum(len(s) for s in sizes)
    images = torch.empty(sum(sum(s) for s in sizes), dtype=torch.uint8, device=dev)
    scales = torch.empty(njobs, dtype=torch.float32, device=dev)
    jobs = (_lib.ConvWeightsJob * njobs)()
    measure = []
    for w, _ in requests:
        ext = _storage_extent(w)
        if ext != w.numel():
            raise ValueError("weight must be dense")
        if getattr(w, '_wc_amax', None) is None and not (ext <= 32768 and ext % 4 == 0 and w.data_ptr() % 16 == 0):
            measure.append(w)
    partials = None
    if measure:
        partials = torch.empty(len(measure) * _lib.ABSMAX_FLOATS, dtype=torch.float32, device=dev)
        sweeps = (_lib.ConvAbsmaxJob * len(measure))()
        for i, w in enumerate(measure):
            sweeps[i].x, sweeps[i].n, sweeps[i].partial = w.data_ptr(), w.numel(), partials.data_ptr() + 4 * _lib.ABSMAX_FLOATS * i
        _lib.check(lib.wc_conv_absmax_batch_f32(ctypes.addressof(sweeps), len(measure), _stream()), "wc_conv_absmax_batch_f32")
    out, j, off, m = [], 0, 0, 0
    for (w, geoms), nbytes in zip(requests, sizes):
        known = getattr(w, '_wc_amax', None)
        if known is not None:
            amax, count = known.data_ptr(), known.numel()
        elif m < len(measure) and measure[m] is w:
            amax, count = partials.data_ptr() + 4 * _lib.ABSMAX_FLOATS * m, _lib.ABSMAX_FLOATS
            m += 1
        else:
            amax, count = None, 0
        res = []
        for i, ((g, k_axis, n_axis), nb) in enumerate(zip(geoms, nbytes)):
            job = jobs[j]
            job.w, job.n_elems, job.g = w.data_ptr(), w.numel(), ctypes.addressof(g)
            job.stride_k, job.stride_n, job.stride_r, job.stride_s = w.stride(k_axis), w.stride(n_axis), w.stride(2), w.stride(3)
            job.image, job.scale = images.data_ptr() + off, scales.data_ptr() + 4 * j
            job.amax, job.amax_count, job.pair_of = amax, count, (j - 1 if i else -1)
            res.append((images[off:off + nb], scales[j:j + 1]))
            j += 1
            off += nb
        out.append(tuple(res))
    _lib.check(lib.wc_conv_weights_batch_f32(ctypes.addressof(jobs), njobs, _stream()), "wc_conv_weights_batch_f32")
    return out


def _clear_images(root):
    for site in root.__dict__.get('_wc_image_sites', ()):
        site._wc_images = None
    root._wc_image_sites = ()


def prepare_images(root, key):
    """Call at the top of a network's forward (behind prepare_spectral), finish_images(root) when the pass ends.  See above."""
    global _recording, _prepared
    _clear_images(root)                         # (a pass that did not end)
    _recording = _prepared = None
    if not BATCH_IMAGES:
        return
    logs = root.__dict__.get('_wc_image_logs')
    if logs is None:
        logs = root._wc_image_logs = {}
    log = logs.get(key)
    if log is None:
        _recording = (root, key, [])
        return
    _prepared = [root, key, False]
    requests, sites = [], []
    for site, geoms in log:
        w = _own_weight(site)
        if w is not None and w.dtype == torch.float32 and w.dim() == 4:
            requests.append((w, geoms))
            sites.append(site)
    if not requests:
        return
    for site, (w, geoms), images in zip(sites, requests, build_images(requests)):
        if site.__dict__.get('_wc_images') is None:
            site._wc_images = []
        site._wc_images.append((w, geoms, images if len(geoms) > 1 else images[0]))
    root._wc_image_sites = tuple(sites)


def _pick_up(site, w, geoms):
    """The images prepared for this request, once; None: the layer builds its own (and the request is logged, or the log marked stale)."""
    recs = site.__dict__.get('_wc_images')
    if recs:
        for i, (rw, rgeoms, images) in enumerate(recs):
            if rw is w and _same_geoms(rgeoms, geoms):
                del recs[i]
                return images
    if _recording is not None:
        _recording[2].append((site, tuple(geoms)))
    elif _prepared is not None:
        _prepared[2] = True
    return None


def finish_images(root):
    global _recording, _prepared
    if _recording is not None and _recording[0] is root:
        root._wc_image_logs[_recording[1]] = _recording[2]
    elif _prepared is not None and _prepared[0] is root:
        # a request the log did not foresee, or a prepared image nobody took: log this key again on its next pass
        if _prepared[2] or any(site.__dict__.get('_wc_images') for site in root.__dict__.get('_wc_image_sites', ())):
            root._wc_image_logs.pop(_prepared[1], None)
    _recording = _prepared = None
    _clear_images(root)


# A k-split convolution whose shares fit one workgroup's waves (wc_conv_local_supported; _Plan.local / .bwd_local: the critic's 128-channel
# layers at 8x8, batch 128) runs as ONE launch that sums the shares in LDS and finishes them (csrc/wc_conv.hip conv_local_kernel; DESIGN.md
# section 4.5) instead of the convolution and a finish launch over 16 MiB of partial sums.  Same bits.  False: the two launches everywhere
# (tests, tools/local_ksplit_bench.py).
LOCAL_KSPLIT = True


def _local(lib, geom, tail=None):
    if not LOCAL_KSPLIT or (tail is not None and tail.c.kind == _lib.TAIL_MASKED and tail.c.colsum_partials):
        return False
    return bool(lib.wc_conv_local_supported(ctypes.addressof(geom)))


def run(planes, image, geom, bias=None, relu=False, nbytes=None, res=None):
    """res: a tensor of the output's shape added to the result in the convolution's finish (wc_conv_res_f16x3: the geometries
    wc_conv_res_supported takes, _Plan.res)"""
    hi, lo, xs = planes
    img, ws = image
    lib = _lib.load()
    y = torch.empty((geom.N, geom.Hout, geom.Wout, geom.Cout), dtype=torch.float32, device=hi.device)
    if _local(lib, geom):
        if res is not None and (relu or not (res.is_contiguous() and res.shape == y.shape and res.dtype == torch.float32 and res.device == y.device)):
            raise ValueError("run: the residual is a dense fp32 tensor of the output's shape (and there is no ReLU behind it)")
        _lib.check(lib.wc_conv_local_f16x3(_ptr(hi), _ptr(lo), _ptr(xs), _ptr(img), _ptr(ws), _ptr(bias) if bias is not None else None,
                                           _ptr(res) if res is not None else None, _ptr(_zero_line(hi.device)), ctypes.addressof(geom),
                                           1 if relu else 0, _ptr(y), None, _stream()), "wc_conv_local_f16x3")
        return y
    if nbytes is None:
        nbytes = lib.wc_conv_workspace_bytes(ctypes.addressof(geom))
    work = torch.empty(nbytes, dtype=torch.uint8, device=hi.device) if nbytes else None
    if res is not None:
        if relu or not (res.is_contiguous() and res.shape == y.shape and res.dtype == torch.float32 and res.device == y.device):
            raise ValueError("run: the residual is a dense fp32 tensor of the output's shape (and there is no ReLU behind it)")
        _lib.check(lib.wc_conv_res_f16x3(_ptr(hi), _ptr(lo), _ptr(xs), _ptr(img), _ptr(ws), _ptr(bias) if bias is not None else None,
                                         _ptr(res), _ptr(_zero_line(hi.device)), ctypes.addressof(geom), _ptr(y),
                                         _ptr(work), nbytes, _stream()), "wc_conv_res_f16x3")
        return y
    _lib.check(lib.wc_conv_f16x3(_ptr(hi), _ptr(lo), _ptr(xs), _ptr(img), _ptr(ws), _ptr(bias) if bias is not None else None,
                                 _ptr(_zero_line(hi.device)), ctypes.addressof(geom), 1 if relu else 0, _ptr(y),
                                 _ptr(work), nbytes, _stream()), "wc_conv_f16x3")
    return y


def _geoms(kind, N, H, W, w):
    """(forward geometry, weight axes (k, n)), (data-gradient geometry, axes) for x of shape (N, H, W, Cin)"""
    if kind == 'same':
        co, ci, k = w.shape[0], w.shape[1], w.shape[2]
        fwd = _dense_geom(N, H, W, ci, co, k, 1)
        bwd = _dense_geom(N, H, W, co, ci, k, 1)
        for t in range(k * k):                       # dx[y] = sum_r g[y + pad - r] w[r]
            bwd.dy[0][t], bwd.dx[0][t] = -bwd.dy[0][t], -bwd.dx[0][t]
        return (fwd, 1, 0), (bwd, 0, 1)
    if kind in ('down', 'down3'):                    # 'down3': the 3x3 weight itself, the pooled 4x4 kernel is formed in the image
        co, ci = w.shape[0], w.shape[1]
        src = _pooled3 if kind == 'down3' else _plain
        return (_dense_geom(N, H, W, ci, co, 4, 2, src), 1, 0), (_phase_geom(N, H // 2, W // 2, co, ci, src), 0, 1)
    if kind == 'up3':                                # the 3x3 weight (Cout, Cin, 3, 3) of UpSampling2D -> Conv2D
        co, ci = w.shape[0], w.shape[1]
        return (_phase_geom(N, H, W, ci, co, _upsampled3), 1, 0), (_dense_geom(N, 2 * H, 2 * W, co, ci, 4, 2, _upsampled3), 0, 1)
    ci, co = w.shape[0], w.shape[1]                  # 'up'
    return (_phase_geom(N, H, W, ci, co), 0, 1), (_dense_geom(N, 2 * H, 2 * W, co, ci, 4, 2), 1, 0)


def weight_gradient(x_planes, g_planes, geom, w, k_axis, n_axis, nbytes=None, colsum=None):
    """dW (in w's own layout) from the split planes of the layer input and of the output gradient; `geom` = the forward
    geometry.  colsum: the partial rows split_planes(gy, colsum=True) left -> returns (dW, db)."""
    lib = _lib.load()
    xh, xl, xs = x_planes
    gh, gl, gs = g_planes[:3]
    dw = torch.empty_like(w)
    if dw.stride() != w.stride():
        raise ValueError("weight must be dense")
    if nbytes is None:
        nbytes = lib.wc_conv_wrw_workspace_bytes(ctypes.addressof(geom))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    if colsum is not None:
        db = torch.empty(geom.Cout, dtype=torch.float32, device=w.device)
        _lib.check(lib.wc_conv_wrw_bias_f16x3(_ptr(xh), _ptr(xl), _ptr(xs), _ptr(gh), _ptr(gl), _ptr(gs), _ptr(_zero_line(w.device)),
                                              ctypes.addressof(geom), _ptr(dw), w.stride(k_axis), w.stride(n_axis), w.stride(2),
                                              w.stride(3), _ptr(colsum), _ptr(db), _ptr(ws), nbytes, _stream()),
                   "wc_conv_wrw_bias_f16x3")
        return dw, db
    _lib.check(lib.wc_conv_wrw_f16x3(_ptr(xh), _ptr(xl), _ptr(xs), _ptr(gh), _ptr(gl), _ptr(gs), _ptr(_zero_line(w.device)),
                                     ctypes.addressof(geom), _ptr(dw), w.stride(k_axis), w.stride(n_axis), w.stride(2),
                                     w.stride(3), _ptr(ws), nbytes, _stream()), "wc_conv_wrw_f16x3")
    return dw


def _reader_record(site, role, device):
    """The record of `site` for `role` when a convolution's finish may write that reader's planes itself (a *_TAIL entry): the history
    route on, the site in training mode, the record there and seeded -- else None, and the caller keeps the finish and the split as two
    launches (the first call of a site, eval mode, a capture that meets a site without a record).  Never creates a record."""
    if not (SPLIT_HIST and site is not None and getattr(site, 'training', True)):
        return None
    h = site.__dict__.get('_wc_split_hist', {}).get(role)
    if h is None or not h[1] or h[0].device != device:
        return None
    return h


class _Tail:
    """The operands of a finish's tail (include/wc_hip.h wc_conv_tail) with the tensors it writes: `planes` = (hi, lo, scale[, partial rows])
    of SPLIT / MASKED, `out` of DX.  Holds every tensor the struct points at for as long as it lives."""

    def __init__(self, kind, shape, device, record=None, role='x', res=None, mask=None, other=None, colsum=False):
        t = self.c = _lib.ConvTail()
        t.kind = kind
        self.keep = (res, mask, other, record)
        self.planes = self.out = None
        if kind == _lib.TAIL_DX:
            self.out = torch.empty(shape, dtype=torch.float32, device=device)
            t.mask, t.other, t.out = _ptr(mask), _ptr(other), _ptr(self.out)
            return
        both = torch.empty((2,) + tuple(shape), dtype=torch.float16, device=device)
        scale = torch.empty(1 + 512, dtype=torch.float32, device=device)      # (split_planes' layout: [scale | scratch])
        t.hi, t.lo, t.scale, t.hist = _ptr(both[0]), _ptr(both[1]), _ptr(scale), _ptr(record[0])
        t.redo = 1 if _guarded(role) else 0
        self.planes = (both[0], both[1], scale)
        if kind == _lib.TAIL_SPLIT:
            t.res = _ptr(res) if res is not None else None
            return
        t.mask = _ptr(mask)
        if colsum:
            part = torch.empty((512, shape[-1]), dtype=torch.float32, device=device)
            t.colsum_partials, t.C = _ptr(part), shape[-1]
            self.planes += (part,)


def _dense32(t, shape):
    return t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.dtype == torch.float32


def run_tail(planes, image, geom, tail, bias=None, nbytes=None):
    """run(planes, image, geom, bias) on a geometry _Plan.tail / .bwd_tail takes, its finish going on to `tail`'s work
    (wc_conv_tail_f16x3): -> the fp32 output (None for a DX tail: the value is never written); tail.planes / tail.out hold the rest."""
    hi, lo, xs = planes
    img, ws = image
    lib = _lib.load()
    y = None
    if tail.c.kind != _lib.TAIL_DX:
        y = torch.empty((geom.N, geom.Hout, geom.Wout, geom.Cout), dtype=torch.float32, device=hi.device)
    if _local(lib, geom, tail):
        _lib.check(lib.wc_conv_local_f16x3(_ptr(hi), _ptr(lo), _ptr(xs), _ptr(img), _ptr(ws), _ptr(bias) if bias is not None else None,
                                           None, _ptr(_zero_line(hi.device)), ctypes.addressof(geom), 0, _ptr(y),
                                           ctypes.addressof(tail.c), _stream()), "wc_conv_local_f16x3")
        return y
    if nbytes is None:
        nbytes = lib.wc_conv_workspace_bytes(ctypes.addressof(geom))
    work = torch.empty(nbytes, dtype=torch.uint8, device=hi.device) if nbytes else None
    _lib.check(lib.wc_conv_tail_f16x3(_ptr(hi), _ptr(lo), _ptr(xs), _ptr(img), _ptr(ws), _ptr(bias) if bias is not None else None,
                                      _ptr(_zero_line(hi.device)), ctypes.addressof(geom), _ptr(y), _ptr(work), nbytes,
                                      ctypes.addressof(tail.c), _stream()), "wc_conv_tail_f16x3")
    return y


def backward_pair(g_planes, image, x_planes, plan, w, colsum=None, tail=None):
    """run(g_planes, image, plan.bwd) and weight_gradient(x_planes, g_planes, plan.fwd, w, ...) of one layer in two launches
    (wc_conv_bwd_pair_f16x3; plan.pair says whether the library takes the layer): -> (dx, dW, db | None), the bits of the two calls.
    tail (plan.bwd_tail; a MASKED or DX _Tail): the data gradient's finish goes on to the tail's work (dx None behind a DX tail)."""
    lib = _lib.load()
    gh, gl, gs = g_planes[:3]
    xh, xl, xs = x_planes
    img, ws = image
    gf, kf, nf = plan.fwd
    gb = plan.bwd[0]
    dx = None
    if tail is None or tail.c.kind != _lib.TAIL_DX:
        dx = torch.empty((gb.N, gb.Hout, gb.Wout, gb.Cout), dtype=torch.float32, device=gh.device)
    dw = torch.empty_like(w)
    if dw.stride() != w.stride():
        raise ValueError("weight must be dense")
    work_dx = torch.empty(plan.bwd_ws, dtype=torch.uint8, device=gh.device) if plan.bwd_ws else None
    work_dw = torch.empty(plan.wrw_ws, dtype=torch.uint8, device=gh.device)
    db = torch.empty(gf.Cout, dtype=torch.float32, device=w.device) if colsum is not None else None
    zero = _zero_line(gh.device)
    if tail is not None:
        _lib.check(lib.wc_conv_bwd_pair_tail_f16x3(_ptr(gh), _ptr(gl), _ptr(gs), _ptr(img), _ptr(ws), _ptr(zero), plan.bwd_ptr, _ptr(dx),
                                                   _ptr(work_dx), plan.bwd_ws,
                                                   _ptr(xh), _ptr(xl), _ptr(xs), plan.fwd_ptr, _ptr(dw), w.stride(kf), w.stride(nf),
                                                   w.stride(2), w.stride(3), _ptr(colsum), _ptr(db), _ptr(work_dw), plan.wrw_ws,
                                                   ctypes.addressof(tail.c), _stream()), "wc_conv_bwd_pair_tail_f16x3")
        return dx, dw, db
    _lib.check(lib.wc_conv_bwd_pair_f16x3(_ptr(gh), _ptr(gl), _ptr(gs), _ptr(img), _ptr(ws), _ptr(zero), plan.bwd_ptr, _ptr(dx),
                                          _ptr(work_dx), plan.bwd_ws,
                                          _ptr(xh), _ptr(xl), _ptr(xs), plan.fwd_ptr, _ptr(dw), w.stride(kf), w.stride(nf), w.stride(2),
                                          w.stride(3), _ptr(colsum), _ptr(db), _ptr(work_dw), plan.wrw_ws, _stream()),
               "wc_conv_bwd_pair_f16x3")
    return dx, dw, db


def takes_planes(shape, wshape, kind, ragged=False):
    """Would fast_conv_or_none take an input of this NHWC shape as planes handed over by K3 (functional.whiten_color(planes=True))?
    Shapes only -- the caller asks before it runs the site.  ragged: the reading layer is marked ragged_conv (see supported)."""
    class _S:
        pass
    xs, ws = _S(), _S()
    xs.shape, ws.shape = tuple(shape), tuple(wshape)
    p = _plan(kind, xs, ws, ragged)
    return bool(p) and p.ok


class _FastConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, kind, plan, relu_input=False, handed=None, site=None, leaky=None, residual=None):
        gf, kf, nf = plan.fwd
        # handed: x is a K3 handle and these are its planes (already ReLU'd and split by K3's epilogue: no pass here)
        # relu_input: the layer is conv(relu(x)); the ReLU happens in the split
        # site: the layer object (generator.Conv2D) -- its splits take their scale from the site's previous call (split_planes)
        # leaky: the layer is conv(leaky_relu(x, leaky)); the activation happens in the split, as the ReLU does
        planes = handed if handed is not None else split_planes(x, relu=relu_input, site=site, role='x', leaky=leaky)
        ctx.site, ctx.leaky = site, leaky
        if ctx.needs_input_grad[0]:                 # the data gradient will want its image too: both in one launch
            img, ctx.bwd_image = weight_image_pair(w, plan.fwd, plan.bwd, site=site)
        else:
            img, ctx.bwd_image = weight_image(w, gf, kf, nf, site=site), None
        # residual: y = conv(x) + residual, in the convolution's finish where it has one that takes it (plan.res), else added here
        if residual is not None and plan.res and FUSED_RESIDUAL:
            y = run(planes, img, gf, bias, nbytes=plan.fwd_ws, res=residual.contiguous())
        else:
            y = run(planes, img, gf, bias, nbytes=plan.fwd_ws)
            if residual is not None:
                y = y + residual
        # the planes stand in for (relu of) x (same bytes) in the weight gradient; x itself only for the ReLU mask
        ctx.save_for_backward(w, *planes, *((x,) if (relu_input or leaky is not None) else ()))
        ctx.kind, ctx.has_bias, ctx.plan, ctx.relu_input = kind, bias is not None, plan, relu_input
        return y

    @staticmethod
    def backward(ctx, gy):
        w, xh, xl, xs = ctx.saved_tensors[:4]
        kind, plan = ctx.kind, ctx.plan
        gy = gy.contiguous()
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        fused_db = want_db and ctx.needs_input_grad[1] and _colsum_ok(gy.shape[-1])    # db rides on the split + the dW reduction
        g_planes = split_planes(gy, colsum=fused_db, site=ctx.site, role='g')
        dx = dw = db = None
        # both gradients wanted, the data gradient's image at hand, a layer the pair entry takes: one grid for the two
        paired = ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and ctx.bwd_image is not None and plan.pair
        if paired:
            dx, dw, pdb = backward_pair(g_planes, ctx.bwd_image, (xh, xl, xs), plan, w, colsum=g_planes[3] if fused_db else None)
            if fused_db:
                db = pdb
        if ctx.needs_input_grad[0]:
            if not paired:
                gb, kb, nb = plan.bwd
                image = ctx.bwd_image if ctx.bwd_image is not None else weight_image(w, gb, kb, nb)
                dx = run(g_planes[:3], image, gb, nbytes=plan.bwd_ws)
            if ctx.relu_input:
                dx = torch.ops.aten.threshold_backward(dx, ctx.saved_tensors[4], 0)
            elif ctx.leaky is not None:
                dx = leaky_backward_(dx, ctx.saved_tensors[4], ctx.leaky)
        if ctx.needs_input_grad[1] and not paired:
            gf, kf, nf = plan.fwd
            if fused_db:
                dw, db = weight_gradient((xh, xl, xs), g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws, colsum=g_planes[3])
            else:
                dw = weight_gradient((xh, xl, xs), g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws)
        if want_db and not fused_db:
            db = gy.sum((0, 1, 2))
        need = ctx.needs_input_grad
        return dx, dw, db, None, None, None, None, None, None, (gy if len(need) > 9 and need[9] else None)


_ones = {}


def _one(device):
    """the device scalar 1.0: the `x scale` of planes that carry their scales per channel (folded into the weight instead)"""
    t = _ones.get(device)
    if t is None:
        t = torch.ones(1, dtype=torch.float32, device=device)
        if not torch.cuda.is_current_stream_capturing():
            _ones[device] = t
    return t


class _SplitConv(torch.autograd.Function):
    """A 1x1 convolution (the block's shortcut, generator.py:142-146) whose input arrives as the pre-split planes of the residual add
    in front (ops.SplitTensor: x[c] = center[c] + (hi + lo)[c] / scale[c]): the kernel runs on the planes themselves with
    wf[o][c] = w[o][c] / scale[c] and bf = bias + <center, w[o]> (wc_fold_channel_scale_f32), so x is neither converted back to fp32
    nor split again (rounds 1-3: one pass for max |x| and one to split, per shortcut and step).  Backward: the data gradient with the
    weight itself; the weight gradient of wf on the same planes, unfolded (wc_unfold_channel_scale_f32)."""

    @staticmethod
    def forward(ctx, x, w, bias, plan, st, site=None):
        from . import ops
        ctx.site = site
        gf, kf, nf = plan.fwd
        wf, bf = ops.fold_channel_scale(w, bias, st.scale, st.center)
        img = weight_image(wf, gf, kf, nf)          # (the folded weight is made inside the pass: nothing to prepare)
        ctx.bwd_image = None
        if ctx.needs_input_grad[0]:
            gb, kb, nb = plan.bwd
            ctx.bwd_image = weight_image(w, gb, kb, nb, site=site)
        hi, lo = st.planes[0].view(st.shape), st.planes[1].view(st.shape)
        one = _one(hi.device)
        y = run((hi, lo, one), img, gf, bf, nbytes=plan.fwd_ws)
        ctx.save_for_backward(w, hi, lo, one, st.scale, st.center)
        ctx.plan, ctx.has_bias = plan, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import ops
        w, xh, xl, one, scale, center = ctx.saved_tensors
        plan = ctx.plan
        gy = gy.contiguous()
        need_w = ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        fused_db = need_w and _colsum_ok(gy.shape[-1])       # db rides on the split + the dW reduction (the unfolding needs it anyway)
        g_planes = split_planes(gy, colsum=fused_db, site=ctx.site, role='g')
        dx = dw = db = None
        paired = ctx.needs_input_grad[0] and need_w and ctx.bwd_image is not None and plan.pair
        if paired:
            dx, D, db = backward_pair(g_planes, ctx.bwd_image, (xh, xl, one), plan, w, colsum=g_planes[3] if fused_db else None)
            if not fused_db:
                db = gy.sum((0, 1, 2))
            dw = ops.unfold_channel_scale(D, db, scale, center)
        elif ctx.needs_input_grad[0]:
            gb, kb, nb = plan.bwd
            image = ctx.bwd_image if ctx.bwd_image is not None else weight_image(w, gb, kb, nb)
            dx = run(g_planes[:3], image, gb, nbytes=plan.bwd_ws)
        if need_w:
            if not paired:
                gf, kf, nf = plan.fwd
                if fused_db:
                    D, db = weight_gradient((xh, xl, one), g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws, colsum=g_planes[3])
                else:
                    D = weight_gradient((xh, xl, one), g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws)
                    db = gy.sum((0, 1, 2))
                dw = ops.unfold_channel_scale(D, db, scale, center)
        elif need_b:
            db = gy.sum((0, 1, 2))
        return dx, dw, (db if need_b else None), None, None, None


def split_conv(x, st, w, bias=None, site=None):
    """conv1x1(x) for a handle x whose data is the ops.SplitTensor st (see _SplitConv).  Raises when the kernel does not take the
    shape -- the producer asks takes_planes() before it writes planes."""
    p = _plan('same', x, w, _ragged(site))
    if not (p and p.ok and tuple(w.shape[2:]) == (1, 1) and w.dtype == torch.float32):
        raise _lib.WcHipError(f"split_conv: a pre-split handle reached a convolution without a planes path {tuple(x.shape)} x {tuple(w.shape)}")
    return _SplitConv.apply(x, w, bias, p, st, site)


def fast_conv_or_none(x, w, bias=None, kind='same', relu_input=False, site=None, leaky_input=None):
    """fast_conv when the kernel takes the call, else None (the caller's other path).  relu_input: conv(relu(x)).
    leaky_input: a negative slope -- conv(leaky_relu(x, slope)).
    site: the layer object that owns this convolution (split_planes keeps the splits' scale history there)."""
    if leaky_input is not None and relu_input:
        raise ValueError("relu_input and leaky_input are two activations")
    handed = getattr(x, '_wc_planes', None)
    ragged = _ragged(site)                          # a layer marked ragged_conv takes a partial last tile (see supported)
    slim = _slim(site)                              # a layer marked slim_conv takes widths that are multiples of 32 (see supported)
    blocks = _blocks(site)                          # a layer marked slim_blocks takes the critic's kinds at multiples of 64 (see supported)
    if not supported(x, w, kind, ragged, slim, blocks):
        if handed is not None:
            raise _lib.WcHipError(f"fast_conv: a K3 handle reached a convolution that cannot take planes {tuple(x.shape)} x {tuple(w.shape)} ({kind})")
        return None
    if handed is not None:
        if relu_input or leaky_input is not None:
            raise ValueError("a K3 handle is already ReLU'd")
        return _FastConv.apply(x, w, bias, kind, _plan(kind, x, w, ragged, slim, blocks), False, handed, site)
    return _FastConv.apply(x, w, bias, kind, _plan(kind, x, w, ragged, slim, blocks), relu_input, None, site,
                           None if leaky_input is None else float(leaky_input))


# The critic's first block reads images (Conv2D 3 -> 128 and the 1x1 shortcut 3 -> 128): the forward stays with MIOpen, the weight and bias
# gradients come from ONE pass over gy on the fp32 matrix pipe (wc_conv_wrw_narrow_f32; WC_NARROW_WRW=0: MIOpen's, rounds 1-4)
NARROW_WRW = os.environ.get('WC_NARROW_WRW', '1') != '0'


def narrow_wrw_supported(x, w):
    """x NHWC fp32 on the GPU, w (Cout, Cin, k, k) with k in (1, 3), k*k*Cin < 32, Cout a multiple of 64"""
    if not (NARROW_WRW and x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() == 4 and w.dim() == 4):
        return False
    k = w.shape[2]
    if w.shape[3] != k or k not in (1, 3) or w.shape[1] != x.shape[3]:
        return False
    N, H, W, C = x.shape
    return bool(_lib.load().wc_conv_narrow64_supported(N, H, W, C, w.shape[0], k))


def narrow_forward(x, w, bias=None, relu=False, mirrored=False, wide32=False):
    """wc_conv_fwd_narrow_f32: y = conv(x, w) + bias for NHWC x with a handful of channels, w (Cout, Cin, k, k) in any dense layout.
    mirrored: w is (Cin, Cout, k, k) of the TRANSPOSED map and its taps are read back to front -- y is then the data gradient of the
    convolution w belongs to (x = its output gradient).  wide32 (_NarrowLastConv only): wc_conv_fwd_narrow32_f32, the wide side in 32s."""
    lib = _lib.load()
    N, H, W, C = x.shape
    k = w.shape[2]
    if mirrored:
        O = w.shape[1]
        ptr = ctypes.c_void_p(w.data_ptr() + 4 * ((k - 1) * w.stride(2) + (k - 1) * w.stride(3)))
        strides = (w.stride(0), w.stride(1), -w.stride(2), -w.stride(3))
    else:
        O = w.shape[0]
        ptr = _ptr(w)
        strides = (w.stride(1), w.stride(0), w.stride(2), w.stride(3))
    y = torch.empty((N, H, W, O), dtype=torch.float32, device=x.device)
    xc = x if x.is_contiguous() else x.contiguous()
    if wide32:
        _lib.check(lib.wc_conv_fwd_narrow32_f32(_ptr(xc), ptr, *strides, _ptr(bias), N, H, W, C, O, k, 1 if relu else 0, _ptr(y), _stream()),
                   "wc_conv_fwd_narrow32_f32")
        return y
    _lib.check(lib.wc_conv_fwd_narrow_f32(_ptr(xc), ptr, *strides, _ptr(bias), N, H, W, C, O, k, 1 if relu else 0, _ptr(y), _stream()),
               "wc_conv_fwd_narrow_f32")
    return y


# The data gradient of the critic's image layers (3x3 conv1 and the 1x1 shortcut of the first block; wanted in the generator's update only) was
# MIOpen's, in front of it torch's threshold_backward over the critic's largest tensor.  A layer marked slim_blocks takes it on the fp32 matrix
# pipe instead (wc_conv_narrow_out_f32), the ReLU's mask applied as the gradient is read.  NARROW_OUT = False: the
# marked layers keep MIOpen's (tests and tools/imagenet_critic_step.py compare the two in one process); unmarked layers never ask.
NARROW_OUT = True


def narrow_out_supported(gshape, wshape, forward=False):
    """Does wc_conv_narrow_out_f32 take a wide NHWC tensor of this shape with this weight?  Shapes only: w (Cw, Cn, k, k), the layer whose
    data gradient is asked for -- (Cn, Cw, k, k) with forward=True, the layer with few outputs itself."""
    if len(gshape) != 4 or len(wshape) != 4 or wshape[2] != wshape[3]:
        return False
    cw, cn = (wshape[1], wshape[0]) if forward else (wshape[0], wshape[1])
    N, H, W, C = gshape
    return C == cw and bool(_lib.load().wc_conv_narrow_out_supported(N, H, W, cw, cn, wshape[2]))


def narrow_out_conv(g, w, mask=None, forward=False, bias=None):
    """wc_conv_narrow_out_f32: the 'same' convolution of the wide NHWC fp32 tensor g down to a handful of channels.  w (Cw, Cn, k, k), any
    dense layout: the DATA GRADIENT of the layer w belongs to, g its output gradient.  forward=True: w is (Cn, Cw, k, k) and the result
    that layer's output (its taps read back to front, the channel strides exchanged).  mask (g's shape): g is read through the backward
    of a ReLU whose pre-activation was `mask` -- the values of threshold_backward(g, mask, 0), which is never written.  bias (Cn floats):
    added to every output pixel in the same launch (wc_conv_narrow_out_bias_f32); without one, the entry and the bits it always had."""
    N, H, W, C = g.shape
    k = w.shape[2]
    if _storage_extent(w) != w.numel():
        raise ValueError("weight must be dense")
    if forward:
        cn = w.shape[0]
        ptr = ctypes.c_void_p(w.data_ptr() + 4 * ((k - 1) * w.stride(2) + (k - 1) * w.stride(3)))
        strides = (w.stride(1), w.stride(0), -w.stride(2), -w.stride(3))
    else:
        cn = w.shape[1]
        ptr = _ptr(w)
        strides = (w.stride(0), w.stride(1), w.stride(2), w.stride(3))
    gc = g if g.is_contiguous() else g.contiguous()
    if mask is not None:
        if not (mask.shape == g.shape and mask.dtype == torch.float32):
            raise ValueError("narrow_out_conv: the mask is an fp32 tensor of g's shape")
        mask = mask if mask.is_contiguous() else mask.contiguous()
    out = torch.empty((N, H, W, cn), dtype=torch.float32, device=g.device)
    if bias is not None:
        if not (bias.shape == (cn,) and bias.dtype == torch.float32 and bias.is_contiguous()):
            raise ValueError("narrow_out_conv: the bias is a dense fp32 vector, one value per output channel")
        _lib.check(_lib.load().wc_conv_narrow_out_bias_f32(_ptr(gc), _ptr(mask), ptr, *strides, _ptr(bias), N, H, W, C, cn, k, _ptr(out),
                                                           _stream()), "wc_conv_narrow_out_bias_f32")
        return out
    _lib.check(_lib.load().wc_conv_narrow_out_f32(_ptr(gc), _ptr(mask), ptr, *strides, N, H, W, C, cn, k, _ptr(out), _stream()),
               "wc_conv_narrow_out_f32")
    return out


def _narrow_out_route(site, gshape, wshape):
    """Does the data gradient of this image layer run on wc_conv_narrow_out_f32?  The layer marked slim_blocks, the switch on, the shape taken."""
    return NARROW_OUT and _blocks(site) and narrow_out_supported(tuple(gshape), tuple(wshape))


class _NarrowInConv(torch.autograd.Function):
    """'same' convolution of an image-like input (k*k*Cin < 32): forward and weight / bias gradient on the fp32 matrix pipe
    (wc_conv_fwd_narrow_f32, wc_conv_wrw_narrow_f32); the data gradient -- wanted in the generator update only -- by MIOpen, or for a
    layer marked slim_blocks (site) by wc_conv_narrow_out_f32."""

    @staticmethod
    def forward(ctx, x, w, bias, site=None):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.site = site
        return narrow_forward(x, w, bias)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        N, H, W, C = x.shape
        O, k = w.shape[0], w.shape[2]
        lib = _lib.load()
        dx = dw = db = None
        g = gy if gy.is_contiguous() else gy.contiguous()
        if ctx.needs_input_grad[0] and _narrow_out_route(ctx.site, g.shape, w.shape):
            dx = narrow_out_conv(g, w)
        elif ctx.needs_input_grad[0]:
            dx = torch.ops.aten.convolution_backward(g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w, None, [1, 1], [k // 2, k // 2], [1, 1],
                                                     False, [0, 0], 1, [True, False, False])[0].permute(0, 2, 3, 1)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_strided(w.shape, w.stride(), dtype=torch.float32, device=w.device)
            if _storage_extent(dw) != dw.numel():
                raise ValueError("weight must be dense")
            db = torch.empty(O, dtype=torch.float32, device=w.device) if ctx.has_bias else None
            nb = lib.wc_conv_wrw_narrow64_workspace_bytes(N, H, W, C, O, k)
            ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
            xc = x if x.is_contiguous() else x.contiguous()
            _lib.check(lib.wc_conv_wrw_narrow64_f32(_ptr(xc), _ptr(g), N, H, W, C, O, k, _ptr(dw), dw.stride(1), dw.stride(0), dw.stride(2),
                                                    dw.stride(3), _ptr(db), _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow64_f32")
        return dx, dw, db, None


def narrow_weight_gradient(x, gy, w):
    """dW (w's own strides) of the 'same' convolution of an image-like NHWC x (narrow_wrw_supported) from its fp32 output gradient: the
    launch of _NarrowInConv.backward without the bias gradient"""
    N, H, W, C = x.shape
    O, k = w.shape[0], w.shape[2]
    lib = _lib.load()
    dw = torch.empty_strided(w.shape, w.stride(), dtype=torch.float32, device=w.device)
    if _storage_extent(dw) != dw.numel():
        raise ValueError("weight must be dense")
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(N, H, W, C, O, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    xc = x if x.is_contiguous() else x.contiguous()
    g = gy if gy.is_contiguous() else gy.contiguous()
    _lib.check(lib.wc_conv_wrw_narrow64_f32(_ptr(xc), _ptr(g), N, H, W, C, O, k, _ptr(dw), dw.stride(1), dw.stride(0), dw.stride(2),
                                            dw.stride(3), None, _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow64_f32")
    return dw


def narrow_in_conv(x, w, bias=None, site=None):
    """y = conv(x, w) + bias for NHWC x with a handful of channels (narrow_wrw_supported).  site: the layer object -- one marked
    slim_blocks takes its data gradient on wc_conv_narrow_out_f32 (see NARROW_OUT)"""
    if _storage_extent(w) != w.numel():
        w = w.contiguous()
    return _NarrowInConv.apply(x, w, bias, site)


def narrow_out_weight_gradient(x, gy, w, wide32=False):
    """dW of a 3x3 'same' convolution with a handful of OUTPUT channels (the generator's last layer, 256 -> 3) by the same one-pass kernel with
    the operands' roles exchanged: dW[o][c][r][s] = sum_q gy[q - (r-1, s-1)][o] x[q][c] is the narrow-input gradient of a convolution that reads
    gy (3 channels) and whose output gradient is x (256 channels), with the taps mirrored -- written through negative tap strides.  x, gy NHWC.
    wide32 (_NarrowLastConv only): wc_conv_wrw_narrow32_f32, x's channels in 32s (and a 1x1 layer as well)."""
    lib = _lib.load()
    N, H, W, C = x.shape
    O, k = w.shape[0], w.shape[2]
    dw = torch.empty_strided(w.shape, w.stride(), dtype=torch.float32, device=w.device)
    if _storage_extent(dw) != dw.numel():
        raise ValueError("weight must be dense")
    last = dw.data_ptr() + 4 * ((k - 1) * dw.stride(2) + (k - 1) * dw.stride(3))        # tap (k-1, k-1): the mirrored (0, 0)
    if wide32:
        nb = lib.wc_conv_wrw_narrow32_workspace_bytes(N, H, W, O, C, k)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        _lib.check(lib.wc_conv_wrw_narrow32_f32(_ptr(gy), _ptr(x), N, H, W, O, C, k, ctypes.c_void_p(last), dw.stride(0), dw.stride(1),
                                                -dw.stride(2), -dw.stride(3), None, _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow32_f32")
        return dw
    nb = lib.wc_conv_wrw_narrow_workspace_bytes(N, H, W, O, C, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    _lib.check(lib.wc_conv_wrw_narrow_f32(_ptr(gy), _ptr(x), N, H, W, O, C, k, ctypes.c_void_p(last), dw.stride(0), dw.stride(1), -dw.stride(2),
                                          -dw.stride(3), None, _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow_f32")
    return dw


def narrow_out_wrw_supported(x, w):
    if not (NARROW_WRW and x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() == 4 and w.dim() == 4):
        return False
    k = w.shape[2]
    if w.shape[3] != k or k not in (1, 3) or w.shape[1] != x.shape[3]:
        return False
    N, H, W, C = x.shape
    return bool(_lib.load().wc_conv_wrw_narrow_supported(N, H, W, w.shape[0], C, k))


# The generator's last layer at a width the CIFAR route above does not take (the ImageNet recipe: 32 -> 3 at 128 x 128; DESIGN.md section
# 4.24).  A layer marked narrow_last (make_generator(narrow_last=True)) runs its forward on the narrow-output kernel with the taps mirrored
# and the bias inside (wc_conv_narrow_out_bias_f32), its weight gradient on the one-pass kernel with the operands exchanged
# (wc_conv_wrw_narrow32_f32) and its data gradient on the mirrored narrow forward (wc_conv_fwd_narrow32_f32): no GEMM + fold, no
# convolution_backward, no intermediate of nine times the output.
def narrow_last_supported(xshape, wshape):
    """Does _NarrowLastConv take an NHWC input of this shape with this weight?  Shapes only: w (Cn, Cw, k, k) with Cn <= 4, the forward
    on the narrow-output kernel (narrow_out_supported(forward=True)) and both gradients on the 32-wide narrow entries
    (wc_conv_narrow32_supported: one predicate for the exchanged weight gradient and the mirrored data gradient)."""
    if len(xshape) != 4 or len(wshape) != 4 or wshape[2] != wshape[3] or wshape[0] > 4:
        return False
    if not narrow_out_supported(tuple(xshape), tuple(wshape), forward=True):
        return False
    N, H, W, _ = xshape
    if N * H * W * wshape[0] >= 2 ** 31:                 # (the mirrored forward's 32-bit element offset; implied by Cn <= 4 only up to 2^29 pixels)
        return False
    return bool(_lib.load().wc_conv_narrow32_supported(N, H, W, wshape[0], wshape[1], wshape[2]))


class _NarrowLastConv(torch.autograd.Function):
    """'same' convolution (1x1 or 3x3) of a wide NHWC input down to a handful of channels (narrow_last_supported), every pass on the
    project's narrow kernels.  db = the column sums of the output gradient, the reduction _NarrowConv3x3 uses under sum_bias_grad."""

    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return narrow_out_conv(x, w, forward=True, bias=bias)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        g = gy if gy.is_contiguous() else gy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = narrow_forward(g, w, None, mirrored=True, wide32=True)
        if ctx.needs_input_grad[1]:
            dw = narrow_out_weight_gradient(x, g, w, wide32=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 1, 2))
        return dx, dw, db


def narrow_last_conv(x, w, bias=None):
    """y = conv(x, w) + bias for contiguous NHWC fp32 x on the GPU and a dense w (Cn, Cw, k, k): narrow_last_supported(x.shape, w.shape)"""
    return _NarrowLastConv.apply(x, w, bias)


def fast_conv(x, w, bias=None, kind='same', residual=None, ragged=False, slim=False):
    """NHWC convolution (see the module docstring) -- raises if the shape is not one the kernel takes.
    residual: a tensor of the output's shape; the result is conv(x) + residual with the bits of that sum, added in the convolution's
    finish where the tap loop is shared over workgroups (wc_conv_res_f16x3), by an elementwise add behind the other geometries.
    ragged: take a partial last tile; slim: take channel widths that are multiples of 32 (see supported)."""
    if not supported(x, w, kind, ragged, slim):
        raise _lib.WcHipError(f"fast_conv: unsupported call {tuple(x.shape)} x {tuple(w.shape)} ({kind})")
    if residual is None:
        return _FastConv.apply(x, w, bias, kind, _plan(kind, x, w, ragged, slim))
    return _FastConv.apply(x, w, bias, kind, _plan(kind, x, w, ragged, slim), False, None, None, None, residual)


# ---- the critic's residual block as one autograd node ------------------------------------------------------------------------------------
# discriminator.ResBlockDown behind the first block, without a norm: y = conv2(relu(conv1(relu(x)))) [pooled] + (shortcut(pool(x)) | x).
# As separate nodes the passes BETWEEN the convolutions were torch's: threshold_backward over conv2's data gradient (which conv1's
# backward then read again to split it), threshold_backward + avg_pool2d_backward + add for the block input's gradient, and the block's
# `h + s` over an output its convolution had just written.  Here the mask rides in the split (split_planes_masked), the input's gradient
# is one launch (block_input_gradient) and the add one operand of conv2's finish (run(res=...)).  The convolutions, their sites' records
# and roles, and the order of every sum are those of the separate nodes: same bits.  FUSED_BLOCK = False: the separate nodes (tests and
# tools/critic_glue_bench.py compare the two in one process); the three FUSED_* flags below switch one part each, for that tool.
FUSED_BLOCK = True
FUSED_MASKED_SPLIT = True       # (a) conv2's data gradient is masked while conv1's backward splits it
FUSED_RESIDUAL = True           # (b) h + s in conv2's finish
FUSED_BLOCK_DX = True           # (c) the block input's gradient in one launch


class _Shape:
    def __init__(self, shape):
        self.shape = tuple(shape)


def critic_block_plans(xshape, w1shape, w2shape, wsshape, down, ragged=False, blocks=False):
    """(plan of conv1, of conv2, of the shortcut | None) when the fused block takes these shapes, else None.  Shapes only: x NHWC,
    the weights (Cout, Cin, k, k), wsshape None for the identity shortcut, down = the block halves the grid; ragged: the block's layers
    are marked ragged_conv, blocks: slim_blocks (see supported)."""
    if len(xshape) != 4 or len(w1shape) != 4 or len(w2shape) != 4:
        return None
    N, H, W, C = xshape
    F1, F2 = w1shape[0], w2shape[0]
    if tuple(w1shape[1:]) != (C, 3, 3) or tuple(w2shape[1:]) != (F1, 3, 3):
        return None
    if down and (H % 2 or W % 2):
        return None
    if wsshape is None:
        if down or F2 != C:
            return None
    elif tuple(wsshape) != (F2, C, 1, 1):
        return None
    if not (_colsum_ok(F1) and _colsum_ok(F2)):          # the bias gradients ride on the splits: no masked fp32 tensor to sum
        return None
    out = (N, H // 2, W // 2) if down else (N, H, W)
    p1 = _plan('same', _Shape(xshape), _Shape(w1shape), ragged, False, blocks)
    p2 = _plan('down3' if down else 'same', _Shape((N, H, W, F1)), _Shape(w2shape), ragged, False, blocks)
    ps = _plan('same', _Shape(out + (C,)), _Shape(wsshape), ragged, False, blocks) if wsshape is not None else None
    if not (p1 and p1.ok and p2 and p2.ok and (wsshape is None or (ps and ps.ok))):
        return None
    return p1, p2, ps


def _images(w, plan, both, site=None):
    """(forward image, data-gradient image | None): _FastConv.forward's choice"""
    if both:
        return weight_image_pair(w, plan.fwd, plan.bwd, site=site)
    gf, kf, nf = plan.fwd
    return weight_image(w, gf, kf, nf, site=site), None


def _layer_gradients(g_planes, fused_db, x_planes, w, plan, bwd_image, need_dx, need_dw, tail=None):
    """The launches of _FastConv.backward behind the split of the output gradient -> (dx, dW, db | None); dx is the convolution's data
    gradient as it comes (no activation's backward).  tail (need_dx, plan.bwd_tail): the data gradient's finish does the tail's work too."""
    cs = g_planes[3] if fused_db else None
    if need_dx and need_dw and bwd_image is not None and plan.pair:
        return backward_pair(g_planes, bwd_image, x_planes, plan, w, colsum=cs, tail=tail)
    dx = dw = db = None
    if need_dx:
        gb, kb, nb = plan.bwd
        image = bwd_image if bwd_image is not None else weight_image(w, gb, kb, nb)
        if tail is not None:
            dx = run_tail(g_planes[:3], image, gb, tail, nbytes=plan.bwd_ws)
        else:
            dx = run(g_planes[:3], image, gb, nbytes=plan.bwd_ws)
    if need_dw:
        gf, kf, nf = plan.fwd
        if fused_db:
            dw, db = weight_gradient(x_planes, g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws, colsum=cs)
        else:
            dw = weight_gradient(x_planes, g_planes, gf, w, kf, nf, nbytes=plan.wrw_ws)
    return dx, dw, db


def _pool2(x):
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


# The k-split finishes of the block write what their next launch read back (csrc/wc_conv.hip conv_finish_tail_kernel; DESIGN.md section
# 4.5): F1 conv1's finish -> conv2's input planes, F2 conv2's finish (with the residual) -> the NEXT block's conv1 input planes, B1 conv2's
# data-gradient finish -> conv1's masked output-gradient planes (and the bias gradient's partial rows), B2 conv1's data-gradient finish ->
# the SAME block's input gradient; B1 and B2 where the caller asks for them (critic_block's backward_tails: the critic's pass).  Each where the plan says the convolution shares its tap loop (_Plan.tail / .bwd_tail) and the
# reader's record can be used (_reader_record); otherwise the two launches run as before.  Same bits either way.  FUSED_FINISH = False:
# the two-launch route everywhere; the four flags below switch one part each (tests, tools/finish_split_bench.py).
FUSED_FINISH = True
FUSED_FINISH_F1 = True
FUSED_FINISH_F2 = True
FUSED_FINISH_B1 = True
FUSED_FINISH_B2 = True


class _CriticBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, ws, bs, sites, plans, down, next_site=None, xh=None, xl=None, xs=None, backward_tails=False):
        conv1, conv2, shortcut = sites
        p1, p2, ps = plans
        need = ctx.needs_input_grad
        need_h = need[0] or need[1] or need[2]
        # xh, xl, xs: the planes of relu(x) for conv1, written by the block in front (its conv2's finish, F2) -- this block's first split
        x_pl = (xh, xl, xs) if xh is not None else split_planes(x, relu=True, site=conv1, role='x')
        img1, bimg1 = _images(w1, p1, need[0], conv1)
        rec = _reader_record(conv2, 'x', x.device) if (FUSED_FINISH and FUSED_FINISH_F1 and p1.tail) else None
        if rec is not None:
            t1 = _Tail(_lib.TAIL_SPLIT, (p1.fwd[0].N, p1.fwd[0].Hout, p1.fwd[0].Wout, p1.fwd[0].Cout), x.device, record=rec, role='x')
            h = run_tail(x_pl, img1, p1.fwd[0], t1, bias=b1, nbytes=p1.fwd_ws)
            h_pl = t1.planes
        else:
            h = run(x_pl, img1, p1.fwd[0], b1, nbytes=p1.fwd_ws)
            h_pl = split_planes(h, relu=True, site=conv2, role='x')
        img2, bimg2 = _images(w2, p2, need_h, conv2)
        s, s_pl, bimgs = x, (), None
        if ws is not None:
            s_pl = split_planes(_pool2(x) if down else x, site=shortcut, role='x')
            imgs, bimgs = _images(ws, ps, need[0], shortcut)
            s = run(s_pl, imgs, ps.fwd[0], bs, nbytes=ps.fwd_ws)
        n_pl = ()
        g2 = p2.fwd[0]
        rec = None
        if next_site is not None and FUSED_FINISH and FUSED_FINISH_F2 and FUSED_RESIDUAL and p2.tail and _dense32(s, (g2.N, g2.Hout, g2.Wout, g2.Cout)):
            rec = _reader_record(next_site, 'x', x.device)
        if rec is not None:
            t2 = _Tail(_lib.TAIL_SPLIT, (g2.N, g2.Hout, g2.Wout, g2.Cout), x.device, record=rec, role='x', res=s)
            y = run_tail(h_pl, img2, g2, t2, bias=b2, nbytes=p2.fwd_ws)
            n_pl = t2.planes
        elif p2.res and FUSED_RESIDUAL:
            y = run(h_pl, img2, g2, b2, nbytes=p2.fwd_ws, res=s)
        else:
            y = run(h_pl, img2, g2, b2, nbytes=p2.fwd_ws) + s
        ctx.save_for_backward(x, h, w1, w2, *x_pl, *h_pl, *s_pl, *((ws,) if ws is not None else ()))
        ctx.sites, ctx.plans, ctx.down = sites, plans, down
        ctx.backward_tails = bool(backward_tails)
        ctx.images = (bimg1, bimg2, bimgs)
        ctx.has_bias = (b1 is not None, b2 is not None, bs is not None)
        # h leaves only for whoever watches the block's second norm site: no gradient, and none made up for it in backward
        # (autograd would otherwise hand backward a zero-filled tensor of h's shape: a pass over memory per block); the planes for the
        # next block likewise
        ctx.mark_non_differentiable(h, *n_pl)
        ctx.set_materialize_grads(False)
        return (y, h) + tuple(n_pl)

    @staticmethod
    def backward(ctx, g, _gh, *_gp):
        saved = ctx.saved_tensors
        x, h, w1, w2 = saved[:4]
        x_pl, h_pl = saved[4:7], saved[7:10]
        conv1, conv2, shortcut = ctx.sites
        p1, p2, ps = ctx.plans
        bimg1, bimg2, bimgs = ctx.images
        need = ctx.needs_input_grad
        need_h = need[0] or need[1] or need[2]
        if g is None:               # (gradients are not materialised: nothing reached y)
            return (None,) * 15
        g = g.contiguous()
        dx = dw1 = db1 = dw2 = db2 = dws = dbs = dx1 = None

        def bias_rides(has, need_b, need_w, C):
            return has and need_b and need_w and _colsum_ok(C)

        # conv2: its output gradient is the block's; its data gradient stays unmasked
        fused2 = bias_rides(ctx.has_bias[1], need[4], need[3], g.shape[-1])
        g2 = split_planes(g, colsum=fused2, site=conv2, role='g')
        fused1 = need_h and bias_rides(ctx.has_bias[0], need[2], need[1], h.shape[-1])
        # B1: conv2's data-gradient finish writes conv1's masked output-gradient planes
        rec = None
        if need_h and ctx.backward_tails and FUSED_FINISH and FUSED_FINISH_B1 and FUSED_MASKED_SPLIT and p2.bwd_tail:
            rec = _reader_record(conv1, 'g', g.device)
        tb1 = _Tail(_lib.TAIL_MASKED, tuple(h.shape), g.device, record=rec, role='g', mask=h, colsum=fused1) if rec is not None else None
        dh, dw2, db2 = _layer_gradients(g2, fused2, h_pl, w2, p2, bimg2, need_h, need[3], tail=tb1)
        if ctx.has_bias[1] and need[4] and not fused2:
            db2 = g.sum((0, 1, 2))
        # the shortcut, as its own node ran it
        other = g
        if ps is not None:
            ws = saved[13]
            fuseds = bias_rides(ctx.has_bias[2], need[6], need[5], g.shape[-1])
            gs = split_planes(g, colsum=fuseds, site=shortcut, role='g')
            other, dws, dbs = _layer_gradients(gs, fuseds, saved[10:13], ws, ps, bimgs, need[0], need[5])
            if ctx.has_bias[2] and need[6] and not fuseds:
                dbs = g.sum((0, 1, 2))
        # conv1: the ReLU between the two (mask: conv1's output h) happens while conv2's data gradient is split
        if need_h:
            if tb1 is not None:
                g1 = tb1.planes
            elif FUSED_MASKED_SPLIT:
                g1 = split_planes_masked(dh, h, site=conv1, role='g', colsum=fused1)
            else:
                g1 = split_planes(torch.ops.aten.threshold_backward(dh, h, 0), colsum=fused1, site=conv1, role='g')
            # B2: conv1's data-gradient finish writes the block input's gradient (identity-resolution blocks: `other` has x's shape)
            tb2 = None
            if (need[0] and ctx.backward_tails and FUSED_FINISH and FUSED_FINISH_B2 and FUSED_BLOCK_DX and not ctx.down and p1.bwd_tail
                    and _dense32(other, x.shape)):
                tb2 = _Tail(_lib.TAIL_DX, tuple(x.shape), g.device, mask=x, other=other)
            dx1, dw1, db1 = _layer_gradients(g1, fused1, x_pl, w1, p1, bimg1, need[0], need[1], tail=tb2)
            if tb2 is not None:
                dx = tb2.out
            if ctx.has_bias[0] and need[2] and not fused1:
                db1 = torch.ops.aten.threshold_backward(dh, h, 0).sum((0, 1, 2))
        if need[0] and dx is None:
            if FUSED_BLOCK_DX:
                dx = block_input_gradient(dx1, x, other, ctx.down)
            else:
                dx = torch.ops.aten.threshold_backward(dx1, x, 0)
                if ctx.down:
                    other = torch.ops.aten.avg_pool2d_backward(other.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), [2, 2], [2, 2], [0, 0],
                                                               False, True, None).permute(0, 2, 3, 1)
                dx = dx + other
        return dx, dw1, db1, dw2, db2, dws, dbs, None, None, None, None, None, None, None, None


# ---- the critic's FIRST block: conv1 -> ReLU -> conv2 as one autograd node -----------------------------------------------------------------
# discriminator.ResBlockDown with is_first: y = conv2(relu(conv1(x))) [pooled]; conv1 reads images (the narrow-input kernels), its output
# h is the critic's largest tensor.  As separate nodes h was written, read back whole to be split for conv2, and in the backward conv2's
# data gradient went through torch's threshold_backward (two reads, one write of that size) only for the narrow weight gradient to read
# the copy once.  Here:
#   PLANES  conv1's kernel writes conv2's planes from the registers that hold h (wc_conv_fwd_narrow_split_f32), where conv2's record can
#           be used (_reader_record) and the grid fits the record (narrow_split_supported); else the two launches.
#   MASK    when the image needs no gradient -- the critic's own updates -- the narrow weight gradient reads conv2's data gradient as it
#           comes and h beside it (wc_conv_wrw_narrow_masked_f32); when it does, threshold_backward, MIOpen's data gradient and the plain
#           entry run as before (the data gradient reads the masked copy anyway) -- unless conv1 is marked slim_blocks: then the image's
#           gradient is the masked narrow-output launch (wc_conv_narrow_out_f32) and the route stays MASK.
# conv2's launches, sites, roles and records are those of _FastConv; the shortcut and the block's add stay with the caller: same bits.
# FIRST_BLOCK = False: the separate nodes; the two flags below switch one part each (tests, tools/first_block_bench.py).  Independent of
# FUSED_BLOCK / FUSED_FINISH, which concern the blocks behind this one.
FIRST_BLOCK = True
FIRST_BLOCK_PLANES = True
FIRST_BLOCK_MASK = True
FIRST_BLOCK_NT = False          # y = h leaves conv1's kernel as non-temporal stores (measured: DESIGN.md section 4.5)


def narrow_shapes_supported(xshape, wshape):
    """narrow_wrw_supported from the shapes alone: x NHWC, w (Cout, Cin, k, k)"""
    if not NARROW_WRW or len(xshape) != 4 or len(wshape) != 4:
        return False
    k = wshape[2]
    if wshape[3] != k or k not in (1, 3) or wshape[1] != xshape[3]:
        return False
    N, H, W, C = xshape
    return bool(_lib.load().wc_conv_narrow64_supported(N, H, W, C, wshape[0], k))


def narrow_split_supported(xshape, wshape):
    """Does conv1's kernel take this narrow-input layer with the reader's planes as a second output?  Shapes only: the narrow layers
    (narrow_shapes_supported) whose grid has at most 512 workgroups -- one pair of the reader's record each at least."""
    if not narrow_shapes_supported(xshape, wshape):
        return False
    N, H, W, C = xshape
    return bool(_lib.load().wc_conv_fwd_narrow_split_supported(N, H, W, C, wshape[0], wshape[2]))


def first_block_route(xshape, w1shape, record):
    """What _CriticFirstBlock's forward runs for conv1 and conv2's input planes: 'planes' (one launch) or 'two' (narrow_forward +
    split_planes) -- from the switch, the shapes and conv2's record (_reader_record's answer) alone."""
    return 'planes' if (FIRST_BLOCK_PLANES and record is not None and narrow_split_supported(xshape, w1shape)) else 'two'


def narrow_forward_split(x, w, bias, record, relu=True, role='x'):
    """narrow_forward(x, w, bias) and split_planes(y, relu, site, role) of the site that owns `record` (a seeded record: _reader_record) in
    one launch: -> y, (hi, lo, scale).  Raises where narrow_split_supported says no."""
    lib = _lib.load()
    N, H, W, C = x.shape
    O, k = w.shape[0], w.shape[2]
    y = torch.empty((N, H, W, O), dtype=torch.float32, device=x.device)
    both = torch.empty((2, N, H, W, O), dtype=torch.float16, device=x.device)
    scale = torch.empty(1 + 512, dtype=torch.float32, device=x.device)        # (split_planes' layout: [scale | scratch])
    xc = x if x.is_contiguous() else x.contiguous()
    flags = (0 if _guarded(role) else 2) | (4 if FIRST_BLOCK_NT else 0)      # WC_NARROW_SPLIT_NO_REDO, WC_NARROW_SPLIT_NT
    _lib.check(lib.wc_conv_fwd_narrow_split_f32(_ptr(xc), _ptr(w), w.stride(1), w.stride(0), w.stride(2), w.stride(3), _ptr(bias), N, H, W, C, O, k,
                                                1 if relu else 0, 0.0, _ptr(y), _ptr(both[0]), _ptr(both[1]), _ptr(scale), _ptr(record[0]), flags,
                                                _stream()), "wc_conv_fwd_narrow_split_f32")
    return y, (both[0], both[1], scale)


def narrow_gradients(x, gy, w, has_bias, mask=None):
    """(dW in w's strides, db | None) of the 'same' convolution of an image-like NHWC x from its fp32 output gradient: the launches of
    _NarrowInConv.backward.  mask: gy is read through the backward of a ReLU whose pre-activation was `mask` (gy's shape) -- the bits of
    narrow_gradients(x, threshold_backward(gy, mask, 0), ...) without that tensor (wc_conv_wrw_narrow_masked_f32)."""
    N, H, W, C = x.shape
    O, k = w.shape[0], w.shape[2]
    lib = _lib.load()
    dw = torch.empty_strided(w.shape, w.stride(), dtype=torch.float32, device=w.device)
    if _storage_extent(dw) != dw.numel():
        raise ValueError("weight must be dense")
    db = torch.empty(O, dtype=torch.float32, device=w.device) if has_bias else None
    nb = lib.wc_conv_wrw_narrow64_workspace_bytes(N, H, W, C, O, k)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    xc = x if x.is_contiguous() else x.contiguous()
    g = gy if gy.is_contiguous() else gy.contiguous()
    if mask is None:
        _lib.check(lib.wc_conv_wrw_narrow64_f32(_ptr(xc), _ptr(g), N, H, W, C, O, k, _ptr(dw), dw.stride(1), dw.stride(0), dw.stride(2),
                                                dw.stride(3), _ptr(db), _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow64_f32")
        return dw, db
    if not (mask.is_contiguous() and mask.shape == g.shape and mask.dtype == torch.float32):
        raise ValueError("narrow_gradients: the mask is a dense fp32 tensor of the gradient's shape")
    _lib.check(lib.wc_conv_wrw_narrow_masked_f32(_ptr(xc), _ptr(g), _ptr(mask), N, H, W, C, O, k, _ptr(dw), dw.stride(1), dw.stride(0),
                                                 dw.stride(2), dw.stride(3), _ptr(db), _ptr(ws), nb, _stream()), "wc_conv_wrw_narrow_masked_f32")
    return dw, db


class _CriticFirstBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, sites, plan):
        conv1, conv2 = sites
        need = ctx.needs_input_grad
        need_h = need[0] or need[1] or need[2]
        rec = _reader_record(conv2, 'x', x.device)
        if first_block_route(tuple(x.shape), tuple(w1.shape), rec) == 'planes':
            h, h_pl = narrow_forward_split(x, w1, b1, rec, relu=True, role='x')
        else:
            h = narrow_forward(x, w1, b1)
            h_pl = split_planes(h, relu=True, site=conv2, role='x')
        img2, bimg2 = _images(w2, plan, need_h, conv2)
        y = run(h_pl, img2, plan.fwd[0], b2, nbytes=plan.fwd_ws)
        ctx.save_for_backward(x, h, w1, w2, *h_pl)
        ctx.sites, ctx.plan, ctx.bimg2 = sites, plan, bimg2
        ctx.has_bias = (b1 is not None, b2 is not None)
        # h leaves for whoever watches the block's second norm site (see _CriticBlock): no gradient, none made up for it
        ctx.mark_non_differentiable(h)
        ctx.set_materialize_grads(False)
        return y, h

    @staticmethod
    def backward(ctx, g, _gh):
        x, h, w1, w2 = ctx.saved_tensors[:4]
        h_pl = ctx.saved_tensors[4:7]
        conv1, conv2 = ctx.sites
        plan = ctx.plan
        need = ctx.needs_input_grad
        need_h = need[0] or need[1] or need[2]
        if g is None:
            return (None,) * 7
        g = g.contiguous()
        dx = dw1 = db1 = None
        # conv2: _FastConv.backward's launches; its data gradient stays unmasked
        fused2 = ctx.has_bias[1] and need[4] and need[3] and _colsum_ok(g.shape[-1])
        g2 = split_planes(g, colsum=fused2, site=conv2, role='g')
        dh, dw2, db2 = _layer_gradients(g2, fused2, h_pl, w2, plan, ctx.bimg2, need_h, need[3])
        if ctx.has_bias[1] and need[4] and not fused2:
            db2 = g.sum((0, 1, 2))
        if need_h:
            k = w1.shape[2]
            want1 = need[1] or (ctx.has_bias[0] and need[2])
            if need[0] and FIRST_BLOCK_MASK and _narrow_out_route(conv1, dh.shape, w1.shape):
                # the image's gradient on the MASK route as well: the narrow-output kernel reads conv2's data gradient as it comes and h beside
                # it, as the weight gradient does -- no threshold_backward, no convolution_backward
                dx = narrow_out_conv(dh, w1, mask=h)
                if want1:
                    dw1, db1 = narrow_gradients(x, dh, w1, ctx.has_bias[0], mask=h)
            elif need[0] or not FIRST_BLOCK_MASK:
                dh = torch.ops.aten.threshold_backward(dh, h, 0)
                if need[0]:
                    dx = torch.ops.aten.convolution_backward(dh.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), w1, None, [1, 1], [k // 2, k // 2],
                                                             [1, 1], False, [0, 0], 1, [True, False, False])[0].permute(0, 2, 3, 1)
                if want1:
                    dw1, db1 = narrow_gradients(x, dh, w1, ctx.has_bias[0])
            elif want1:
                dw1, db1 = narrow_gradients(x, dh, w1, ctx.has_bias[0], mask=h)
        return dx, dw1, db1, dw2, db2, None, None


def critic_first_block(x, w1, b1, w2, b2, sites, plan):
    """conv2(relu(conv1(x))) of the critic's first block (see above): x NHWC fp32 on the GPU with a handful of channels
    (narrow_wrw_supported(x, w1)), sites = (conv1's layer, conv2's), plan = conv2's ('same' or 'down3') on conv1's output.
    -> (y, h): conv2's output and detached conv1's output, the tensor the block's second norm site sees."""
    if _storage_extent(w1) != w1.numel():
        w1 = w1.contiguous()
    return _CriticFirstBlock.apply(x, w1, b1, w2, b2, sites, plan)


def critic_block(x, w1, b1, w2, b2, ws, bs, sites, plans, down, next_site=None, x_planes=None, backward_tails=False):
    """One critic block behind the first (see above): x NHWC fp32 on the GPU, the three weights as their layers hand them out (ws / bs
    None: identity shortcut), sites = the three layer objects (the shortcut's None with ws), plans from critic_block_plans.
    next_site: the layer that reads relu(y) next (the following block's conv1) -- its input planes then come out of conv2's finish where
    that can write them.  x_planes: such planes of relu(x), from the block in front: this block's first split is skipped.
    backward_tails: the finishes of the block's two data gradients do their followers' work as well (B1, B2 above).  The critic's pass
    asks for it (Discriminator.forward); a block called on its own keeps its backward's launches -- the masked split and the block
    input's gradient as launches of their own, which tests/test_critic_glue_gpu.py names for a block called that way.
    -> (y, h, planes): the block's output, detached conv1's output (the tensor the block's second norm site sees), and the (hi, lo,
    scale) planes of relu(y) for next_site or None."""
    out = _CriticBlock.apply(x, w1, b1, w2, b2, ws, bs, sites, plans, down, next_site, *(x_planes if x_planes is not None else (None, None, None)), backward_tails)
    return out[0], out[1], (tuple(out[2:5]) if len(out) > 2 else None)
