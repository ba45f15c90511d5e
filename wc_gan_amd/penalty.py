"""WGAN-GP's gradient penalty (scripts/cifar10_resnet_wgan_*.sh: --gradinet_penalty_weight 10) without second-order autograd
(DESIGN.md section 4.17).

    P(theta) = (weight / N) sum_n (||g_n|| - 1)^2,     g_n = grad of the critic's adversarial output with respect to x_hat_n

The critic of every recipe has no batch-dependent layer and ReLUs only, so with v_n = (2 weight / N)(1 - 1 / ||g_n||) g_n held constant

    grad_theta P = grad_theta T,     T = sum_n (output tangent of the critic at x_hat_n along v_n, the primal pass's ReLU masks frozen)

and back-propagating T through the tangent network meets the adjoints delta of the pass that produced g.  Per convolution l with input
tangent tau_l (behind the mask) and primal output z_l:  dP/dW_l = wrw(x = tau_l, gy = delta(z_l)),  dP/db_l = 0.  Three sweeps:

    1. primal forward at x_hat, every ReLU's pre-activation kept in fp32
    2. data-gradient sweep from the heads to the image: every delta(z_l) (kept) and g
    3. tangent forward of v: at each convolution the planes of mask * t feed the forward kernel (no bias) and the weight-gradient kernel

On the GPU the three primitives per convolution are conv.run, conv.run on the data-gradient image and conv.weight_gradient wherever
conv.supported takes the shape, the narrow-input kernels at the image layers (their data gradient stays torch's, as in the generator
update), and the same maps in torch ops everywhere else -- the CPU, float64, widths the kernels do not take.  Nothing here touches an
autograd graph or synchronises with the host: the whole call can be recorded into a hipGraph.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from . import conv as C
from .ops import _ptr, _stream

# after a call: the bool NHWC tensor each ReLU was applied with, in tests/critic_reference.py's order (one small `a > 0` launch per ReLU and
# call, 8 at the recipe's depth; the engine itself reads the fp32 pre-activations)
last_masks = []
last_route = {'hip': 0, 'torch': 0}   # after a call: convolution calls (forward, data gradient, weight gradient) per route


def _hip(t):
    return t.is_cuda and t.dtype == torch.float32


def interpolate(real, fake, eps=None):
    """x_hat[n] = eps[n] real[n] + (1 - eps[n]) fake[n]; eps (N,) -- drawn uniformly from the device's current generator when None"""
    N = real.shape[0]
    if eps is None:
        eps = torch.rand(N, device=real.device, dtype=real.dtype)
    eps = eps.reshape(N).to(real.dtype)
    if _hip(real):
        real, fake, eps = real.detach().contiguous(), fake.detach().contiguous(), eps.contiguous()
        out = torch.empty_like(real)
        _lib.check(_lib.load().wc_gp_interp_f32(_ptr(real), _ptr(fake), _ptr(eps), N, real.numel() // N, _ptr(out), _stream()), "wc_gp_interp_f32")
        return out
    e = eps.view(N, *([1] * (real.dim() - 1)))
    return e * real.detach() + (1 - e) * fake.detach()


def penalty_rows(g, weight):
    """g (N, ...) -> (norms (N,), v of g's shape, the penalty as a 0-d tensor)"""
    N = g.shape[0]
    if _hip(g):
        lib = _lib.load()
        g = g.contiguous()
        norms = torch.empty(N, dtype=torch.float32, device=g.device)
        v = torch.empty_like(g)
        pen = torch.empty(1, dtype=torch.float32, device=g.device)
        nb = lib.wc_gp_rows_workspace_bytes(N)
        ws = torch.empty(nb, dtype=torch.uint8, device=g.device)
        _lib.check(lib.wc_gp_rows_f32(_ptr(g), N, g.numel() // N, float(weight), 1.0 / N, _ptr(norms), _ptr(v), _ptr(pen), _ptr(ws), nb, _stream()),
                   "wc_gp_rows_f32")
        return norms, v, pen.reshape(())
    flat = g.reshape(N, -1)
    norms = flat.norm(dim=1)
    coef = torch.where(norms > 0, (2.0 * weight / N) * (1 - 1 / norms), torch.zeros_like(norms))
    return norms, (coef[:, None] * flat).view_as(g), (weight / N) * ((norms - 1) ** 2).sum()


def _pool(x):
    return F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()


def _unpool(g):
    """the transpose of _pool: every output gradient spread over its 2 x 2 window"""
    return (g * 0.25).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def _mask_(d, a):
    """d * 1[a > 0] (in place where the one-launch kernel takes the tensor)"""
    if _hip(d) and d.is_contiguous() and a.is_contiguous() and d.numel() % 4 == 0:
        return C.leaky_backward_(d, a, 0.0)
    return d * (a > 0).to(d.dtype)


class _Operand:
    """An fp32 NHWC tensor as a convolution operand: t itself, relu(t) (`relu`: the primal pass) or t * 1[a > 0] (`a`: a tangent behind
    the frozen ReLU of pre-activation a).  The dense form and the fp16 planes are made once, whoever asks first."""
    __slots__ = ('t', 'a', 'relu', '_dense', '_planes')

    def __init__(self, t, a=None, relu=False):
        self.t, self.a, self.relu, self._dense, self._planes = t, a, relu, None, None

    def dense(self):
        if self._dense is None:
            t = self.t
            self._dense = F.relu(t) if self.relu else t if self.a is None else t * (self.a > 0).to(t.dtype)
        return self._dense

    def planes(self, site, role):
        if self._planes is None:
            if self.a is not None:
                self._planes = C.split_planes_masked(self.t, self.a, 0.0, site=site, role=role)
            else:
                self._planes = C.split_planes(self.t, relu=self.relu, site=site, role=role)
        return self._planes


class _Layer:
    """One convolution of the critic during one call: its route and the three primitives.  `x`: the primal input (NHWC) -- shapes and the
    route come from it.  pooled: Conv2D 3x3 -> AveragePooling2D as the one 4x4 stride-2 layer ('down3'), outputs at half the grid."""

    def __init__(self, layer, x, pooled, route):
        self.layer, self.w, self.bias, self.x, self.pooled, self.count = layer, layer.conv.weight.detach(), layer.conv.bias, x, pooled, route
        self.kind = 'down3' if pooled else 'same'
        self.pad = self.w.shape[2] // 2
        self._images = None
        from . import generator as _g          # WC_FAST_CONV=0 means MIOpen everywhere: here too (the narrow layers follow conv.NARROW_WRW)
        ragged = C._ragged(layer)              # a layer marked ragged_conv takes a partial last tile here as in its own forward
        if _g.FAST_CONV and C.supported(x, self.w, self.kind, ragged):
            self.route, self.plan = 'block', C._plan(self.kind, x, self.w, ragged)
        elif not pooled and C.narrow_wrw_supported(x, self.w) and C._storage_extent(self.w) == self.w.numel():
            self.route = 'narrow'
        else:
            self.route = 'torch'

    def images(self):
        if self._images is None:                                    # the forward and the data-gradient image in one launch, once per call
            self._images = C.weight_image_pair(self.w, self.plan.fwd, self.plan.bwd)
        return self._images

    def _backward(self, g, x, which):
        if self.pooled:
            g = _unpool(g)
        self.count['torch'] += 1
        out = torch.ops.aten.convolution_backward(g.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), self.w, None, [1, 1], [self.pad, self.pad], [1, 1],
                                                  False, [0, 0], 1, [which == 0, which == 1, False])[which]
        return out.permute(0, 2, 3, 1).contiguous() if which == 0 else out

    def forward(self, op, role, bias):
        b = self.bias.detach() if (bias and self.bias is not None) else None
        if self.route == 'block':
            self.count['hip'] += 1
            return C.run(op.planes(self.layer, role), self.images()[0], self.plan.fwd[0], b, nbytes=self.plan.fwd_ws)
        if self.route == 'narrow':
            self.count['hip'] += 1
            return C.narrow_forward(op.dense(), self.w, b)
        self.count['torch'] += 1
        y = F.conv2d(op.dense().permute(0, 3, 1, 2), self.w, b, padding=self.pad)
        return (F.avg_pool2d(y, 2) if self.pooled else y).permute(0, 2, 3, 1).contiguous()

    def data_gradient(self, dop):
        if self.route == 'block':
            self.count['hip'] += 1
            return C.run(dop.planes(self.layer, 'd'), self.images()[1], self.plan.bwd[0], nbytes=self.plan.bwd_ws)
        return self._backward(dop.dense(), self.x, 0)               # (the image layers: torch's / MIOpen's, as in the generator update)

    def weight_gradient(self, top, dop):
        if self.route == 'block':
            self.count['hip'] += 1
            gf, kf, nf = self.plan.fwd
            return C.weight_gradient(top.planes(self.layer, 't'), dop.planes(self.layer, 'd'), gf, self.w, kf, nf, nbytes=self.plan.wrw_ws)
        if self.route == 'narrow':
            self.count['hip'] += 1
            return C.narrow_weight_gradient(top.dense(), dop.dense(), self.w)
        return self._backward(dop.dense(), top.dense(), 1)


class _Block:
    __slots__ = ('down', 'a1', 'a2', 'conv1', 'conv2', 'shortcut', 'd1', 'd2')


def _refuse(D):
    """a critic the identity does not cover"""
    from .discriminator import ResBlockDown
    from .generator import _UnfusedStack
    if getattr(D, 'arch', 'res') != 'res' or not all(isinstance(b, ResBlockDown) for b in D.blocks):
        raise NotImplementedError("gradient_penalty: arch='dcgan' (LeakyReLU blocks, the flatten tail) is not built; the ResNet critic is")
    if D.dropout is not None:
        raise NotImplementedError("gradient_penalty: a critic with dropout (a fresh mask per pass: the primal masks cannot be frozen)")
    for i, blk in enumerate(D.blocks):
        for name in ('bn1', 'bn2'):
            bn = getattr(blk, name)
            if not (isinstance(bn, _UnfusedStack) and bn.norm_layer is None and len(bn.branches) == 0):
                raise NotImplementedError(f"gradient_penalty: blocks.{i}.{name} is {type(bn).__name__}, a norm other than 'n' "
                                          "(the closed form needs a critic without batch-dependent or affine norm layers)")
    for name, mod in D.named_modules():
        if hasattr(mod, 'normalized_weight'):
            raise NotImplementedError(f"gradient_penalty: spectral=True ({name} is {type(mod).__name__}); the WGAN-GP critics carry no "
                                      "spectral normalisation")


def gradient_penalty(D, x_hat, cls=None, weight=10.0):
    """Adds d/dtheta of (weight / N) sum_n (||grad_x D(x_hat_n)|| - 1)^2 in place into the .grad of every parameter of D (zeros are
    allocated where .grad is None; .grad is never rebound) and returns (the penalty, a detached 0-d tensor; the (N,) gradient norms).
    The penalty is on the adversarial head; cls: the labels a PROJECTIVE critic embeds.  x_hat NHWC."""
    global last_masks, last_route
    _refuse(D)
    route = {'hip': 0, 'torch': 0}
    with torch.no_grad():
        for p in D.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        x = x_hat.detach().contiguous()
        N = x.shape[0]

        # ---- 1: the primal forward, every pre-activation kept ----
        blocks, masks = [], []
        for blk in D.blocks:
            r = _Block()
            r.down = blk.resample == 'DOWN'
            r.a1 = None if blk.is_first else x
            r.conv1 = _Layer(blk.conv1, x, False, route)
            r.a2 = r.conv1.forward(_Operand(x, relu=not blk.is_first), 'p', True)
            r.conv2 = _Layer(blk.conv2, r.a2, r.down, route)
            h = r.conv2.forward(_Operand(r.a2, relu=True), 'p', True)
            s = _pool(x) if r.down else x
            r.shortcut = None
            if blk.has_shortcut:
                r.shortcut = _Layer(blk.shortcut, s, False, route)
                s = r.shortcut.forward(_Operand(s), 'p', True)
            x = h + s
            if r.a1 is not None:
                masks.append(r.a1 > 0)
            masks.append(r.a2 > 0)
            blocks.append(r)
        a_last = x
        masks.append(a_last > 0)

        # ---- 2: the adjoints, from the adversarial head (seeded with 1 per sample) down to the image ----
        _, H, W, Cl = a_last.shape
        seed = D.out.weight.detach().reshape(1, Cl)
        if D.type == 'PROJECTIVE':
            idx = cls.reshape(-1).long()
            seed = seed + D.emb.weight.detach()[idx]
        pool_w = 1.0 if D.sum_pool else 1.0 / (H * W)
        d = (seed * pool_w).expand(N, Cl).reshape(N, 1, 1, Cl).expand(N, H, W, Cl).contiguous()
        d = _mask_(d, a_last)
        for r in reversed(blocks):
            r.d2 = _Operand(d)                          # delta of the block's output = of conv2's (pooled) output = of the shortcut's
            r.d1 = _Operand(_mask_(r.conv2.data_gradient(r.d2), r.a2))
            dx = r.conv1.data_gradient(r.d1)
            if r.a1 is not None:
                dx = _mask_(dx, r.a1)
            ds = r.shortcut.data_gradient(r.d2) if r.shortcut is not None else d
            d = dx + (_unpool(ds) if r.down else ds)
        norms, v, pen = penalty_rows(d, weight)

        # ---- 3: the tangent of v; each convolution's masked input meets the kept delta of its output ----
        t = v
        for r in blocks:
            top = _Operand(t, a=r.a1)
            r.conv1.layer.conv.weight.grad.add_(r.conv1.weight_gradient(top, r.d1))
            top = _Operand(r.conv1.forward(top, 't', False), a=r.a2)
            r.conv2.layer.conv.weight.grad.add_(r.conv2.weight_gradient(top, r.d2))
            th = r.conv2.forward(top, 't', False)
            ts = _pool(t) if r.down else t
            if r.shortcut is not None:
                top = _Operand(ts)
                r.shortcut.layer.conv.weight.grad.add_(r.shortcut.weight_gradient(top, r.d2))
                ts = r.shortcut.forward(top, 't', False)
            t = th + ts
        t = _mask_(t, a_last)
        phi = t.sum(dim=(1, 2)) if D.sum_pool else t.mean(dim=(1, 2))
        D.out.weight.grad.add_(phi.sum(dim=0, keepdim=True))
        if D.type == 'PROJECTIVE':
            D.emb.weight.grad.index_add_(0, idx, phi)
    last_masks, last_route = masks, route
    return pen.detach(), norms.detach()
