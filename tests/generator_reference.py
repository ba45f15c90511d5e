"""Float64 reference of the ResNet WC generator (generator.py:93-163 of the reference project), written out layer by layer; plain torch,
any device, not collected.

From a `state_dict` of wc_gan_amd.generator.Generator (arch='res', norms 'd') and the `make_generator` keywords, in the reference
project's op order -- none of this project's shortcuts (no merged 4x4 kernel, no shortcut at the input resolution, no fused site, no
class / sample switch, no table of all classes):

    y = dense(concat(emb[cls], z))  (concat_cls)  |  dense(z);   reshape to first_block_shape                 generator.py:121-129
    per block (generator.py:142-146, the SN-GAN generator block):
        h = relu(norm1(x));  h = conv3x3(upsample2x(h));  h = relu(norm2(h));  h = conv3x3(h)
        s = conv1x1(upsample2x(x));  y = h + s                  (SAME: no upsampling)
    y = tanh(conv3x3(relu(final_norm(y))))                                                                      generator.py:154-158

A convolution is unfold + matmul on the kernel itself ('same' zero padding); the upsampling is a literal nearest-neighbour repeat.

A WC site (generator.py:82-87: `_npart` then `_repart`) on the M = N H W rows of its NHWC input, per statistic group when groups > 1:

    mu = mean of the rows,  f = x - mu,  Sigma = f^T f / (M - ddof)
    L = chol((1 - eps) Sigma + eps I)  (oracle/wc_oracle.py's shrinkage),  W = L^-1 by a triangular solve against I -- both in float64
    xhat = f W^T;   y_n = xhat_n Gamma_n + beta_n
    moving <- momentum moving + (1 - momentum) (mu, Sigma), group after group; evaluation mode whitens with the moving buffers instead

Coloring (generator.py:49-78), one (Gamma_n, beta_n) per SAMPLE, chosen by its class:
    uconv    Gamma = U, beta = b                                     branches.0 = the 1x1 Conv2D (kernel (1, 1, Cin, Cout))
    ucconv   Gamma_n = K[cls_n] + U,  beta_n = B[cls_n] + b          branches.0 = ConditionalConv11, branches.1 = the 1x1 Conv2D
    ufconv   Gamma_n = sum_e alpha[cls_n, e] D[e] + U,  beta_n = b   branches.0 = FactorizedConv11 (filters_emb, no bias), branches.1 = 1x1

ReLU masks: an fp32 and a float64 network disagree on the sign of pre-activations within rounding of zero, and a handful of flipped
elements in millions moves every gradient behind them by 1e-3.  `masks` (one bool NHWC tensor per ReLU, in the order the network applies
them: norm1, norm2 of each block, then the final norm) replaces the reference's own signs: h * mask.  `pre` keeps the tensors the ReLUs
were applied to; `site_disagreement` / `mask_disagreement` say how many forced elements differ from the reference's own signs and how far
from zero they lie, so that forcing cannot hide a wrong mask.

The arithmetic runs in the dtype of `params` (float64 from `leaves`; `leaves(state, torch.float32)` gives the same network in fp32 on
torch's kernels -- the yardstick the HIP route's bounds come from); the C x C stage of a site is float64 either way.
"""
import torch
import torch.nn.functional as F

BRANCHES = {'uconv': ('u',), 'ucconv': ('c', 'u'), 'ufconv': ('f', 'u')}


def leaves(state, dtype=torch.float64):
    """copies of the state dict's parameters as autograd leaves, and of its moving statistics (the npart buffers)"""
    params, buffers = {}, {}
    for name, t in state.items():
        c = t.detach().to(dtype).clone()
        if name.endswith('.moving_mean') or name.endswith('.moving_cov'):
            buffers[name] = c
        else:
            params[name] = c.requires_grad_(True)
    return params, buffers


def upsample2x(x):
    """nearest neighbour, NHWC"""
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def conv2d(x, w, b):
    """'same' convolution of NHWC x with w (Cout, Cin, k, k), k odd: unfold + one matmul (torch's float64 convolution is the slow part
    of this reference on a GPU)"""
    N, H, W_, C = x.shape
    O, k = w.shape[0], w.shape[2]
    if k == 1:
        y = x.reshape(-1, C) @ w.reshape(O, C).t()
    else:
        cols = F.unfold(x.permute(0, 3, 1, 2), k, padding=k // 2)              # (N, Cin k k, H W), rows ordered (c, r, s) as w is
        y = cols.transpose(1, 2).reshape(-1, C * k * k) @ w.reshape(O, -1).t()
    if b is not None:
        y = y + b
    return y.view(N, H, W_, O)


class Generator:
    """generator(z, cls) -> image (N, H, W, 3); afterwards `pre` holds the tensor each ReLU was applied to (NHWC, detached), `sites` the
    state-dict prefix of each of those norms, and `moving` the {prefix: (moving_mean (C, 1), moving_cov (C, C))} a training-mode call
    leaves behind."""

    def __init__(self, params, buffers, masks=None, training=True, groups=1, block_sizes=(128, 128, 128), resamples=('UP', 'UP', 'UP'),
                 first_block_shape=(4, 4, 128), number_of_classes=10, concat_cls=False, block_norm='d', block_after_norm='uconv',
                 filters_emb=10, last_norm='d', last_after_norm='uconv', arch='res', spectral=False, ddof=1, epsilon=1e-3, momentum=0.99,
                 **_unused):
        assert arch == 'res' and not spectral and block_norm == 'd' and last_norm == 'd'
        assert block_after_norm in BRANCHES and last_after_norm in BRANCHES and len(block_sizes) == len(resamples)
        self.p, self.b = params, buffers
        self.masks, self.training, self.groups = masks, bool(training), int(groups)
        self.block_sizes, self.resamples = [int(b) for b in block_sizes], list(resamples)
        self.first_block_shape = tuple(int(v) for v in first_block_shape)
        self.concat_cls, self.block_after, self.last_after = bool(concat_cls), block_after_norm, last_after_norm
        self.ddof, self.eps, self.momentum = int(ddof), float(epsilon), float(momentum)
        self.pre, self.sites, self.moving = [], [], {}

    # -- a WC site ------------------------------------------------------------------------------------------------------------------
    def tables(self, prefix, after_norm, cls, N):
        """(Gamma (N, C, C) | (C, C), beta (N, C) | (C,)) of the samples: the branch tables added (generator.py:58, 77: `Add`)"""
        gamma = beta = None
        for i, kind in enumerate(BRANCHES[after_norm]):
            name = f'{prefix}.branches.{i}'
            kernel = self.p[name + '.kernel']
            if kind == 'u':
                C = kernel.shape[-1]
                g, b = kernel.view(C, C), self.p[name + '.bias']
            else:
                idx = cls.reshape(-1).long()
                assert idx.shape[0] == N
                if kind == 'c':
                    g, b = kernel[idx], self.p[name + '.bias'][idx]
                else:
                    E, C = kernel.shape[0], kernel.shape[-1]
                    g, b = (self.p[name + '.class_matrix'][idx] @ kernel.view(E, C * C)).view(N, C, C), None
            gamma = g if gamma is None else gamma + g
            if b is not None:
                beta = b if beta is None else beta + b
        return gamma, beta

    def _whitening(self, sigma):
        C = sigma.shape[0]
        eye = torch.eye(C, dtype=torch.float64, device=sigma.device)
        L = torch.linalg.cholesky((1.0 - self.eps) * sigma.double() + self.eps * eye)
        return torch.linalg.solve_triangular(L, eye, upper=False).to(sigma.dtype)

    def site(self, prefix, after_norm, x, cls):
        """x NHWC -> the coloured whitened x; training mode leaves the updated moving statistics in `moving`"""
        N, H, W_, C = x.shape
        mm, mc = self.b[prefix + '.npart.moving_mean'], self.b[prefix + '.npart.moving_cov']
        if self.training:
            assert N % self.groups == 0
            xhat = []
            for xg in x.reshape(self.groups, -1, C):
                M = xg.shape[0]
                mu = xg.mean(dim=0)
                f = xg - mu
                sigma = f.t() @ f / (M - self.ddof)
                xhat.append(f @ self._whitening(sigma).t())
                mm = self.momentum * mm + (1.0 - self.momentum) * mu.detach().view(C, 1)
                mc = self.momentum * mc + (1.0 - self.momentum) * sigma.detach()
            self.moving[prefix] = (mm, mc)
            xhat = torch.cat(xhat)
        else:
            xhat = (x.reshape(-1, C) - mm.view(C)) @ self._whitening(mc).t()
        gamma, beta = self.tables(prefix, after_norm, cls, N)
        if gamma.dim() == 3:
            y = torch.bmm(xhat.view(N, H * W_, C), gamma)
            if beta is not None:
                y = y + (beta.unsqueeze(1) if beta.dim() == 2 else beta)
        else:
            y = xhat @ gamma + beta
        return y.view(N, H, W_, C)

    def _relu(self, prefix, h):
        k = len(self.pre)
        self.pre.append(h.detach())
        self.sites.append(prefix)
        if self.masks is None:
            return F.relu(h)
        m = self.masks[k]
        assert m.dtype == torch.bool and m.shape == h.shape, (prefix, m.dtype, tuple(m.shape), tuple(h.shape))
        return h * m.to(h.dtype)

    # -- the network ----------------------------------------------------------------------------------------------------------------
    def _conv(self, prefix, x):
        return conv2d(x, self.p[prefix + '.conv.weight'], self.p.get(prefix + '.conv.bias'))

    def _block(self, i, x, resample, cls):
        name = f'blocks.{i}'
        up = upsample2x if resample == 'UP' else (lambda t: t)
        h = self._relu(name + '.bn1', self.site(name + '.bn1', self.block_after, x, cls))
        h = self._conv(name + '.conv1', up(h))
        h = self._relu(name + '.bn2', self.site(name + '.bn2', self.block_after, h, cls))
        h = self._conv(name + '.conv2', h)
        return h + self._conv(name + '.shortcut', up(x))

    def __call__(self, z, cls=None):
        self.pre, self.sites, self.moving = [], [], {}
        y = z
        if self.concat_cls:
            y = torch.cat([self.p['emb.weight'][cls.reshape(-1).long()], z], dim=-1)
        y = (y @ self.p['dense.weight'].t() + self.p['dense.bias']).view(-1, *self.first_block_shape)
        for i, resample in enumerate(self.resamples):
            y = self._block(i, y, resample, cls)
        y = self._relu('final_norm', self.site('final_norm', self.last_after, y, cls))
        return torch.tanh(self._conv('final_conv', y))


def relu_count(block_sizes):
    """norm1 and norm2 of every block and the final norm: 7 for three blocks, 9 for four"""
    return 2 * len(block_sizes) + 1


def site_disagreement(masks, pre):
    """per ReLU: (worst |h| / max|h| over the elements where the forced mask differs from the sign of the reference's own
    pre-activation -- 0.0 when none differs --, the share of such elements)"""
    out = []
    for m, h in zip(masks, pre):
        diff = m != (h > 0)
        n = int(diff.sum())
        out.append((float(h[diff].abs().max() / h.abs().max()) if n else 0.0, n / h.numel()))
    return out


def mask_disagreement(masks, pre):
    """(worst |h| / max|h| over all disagreeing elements, how many disagree)"""
    worst, count = 0.0, 0
    for (band, share), h in zip(site_disagreement(masks, pre), pre):
        worst, count = max(worst, band), count + int(round(share * h.numel()))
    return worst, count


# -----------------------------------------------------------------------------------------------------------------------------------
# the comparison the tests make (CPU sensitivity asserts and GPU parity alike)
# -----------------------------------------------------------------------------------------------------------------------------------
KINDS = ('image', 'conv_w', 'conv_b', 'gamma', 'beta', 'dense', 'moving')


def kind_of(name):
    if name.startswith(('dense.', 'emb.')):
        return 'dense'
    if '.branches.' in name:
        return 'beta' if name.endswith('.bias') else 'gamma'          # (kernel, class_matrix: what Gamma is made of)
    assert '.conv.' in name, name
    return 'conv_w' if name.endswith('.weight') else 'conv_b'


def zero_in_exact_arithmetic(name):
    """The bias of a block convolution: conv1's output is read by norm2, conv2's and the shortcut's by the next block's norm1 (or the final
    norm) with only the add in between, and by the next shortcut, a 1x1 convolution, which turns a per-channel constant into a per-channel
    constant in front of the norm after it.  A site subtracts the batch mean, so these gradients are zero in training mode."""
    return name.startswith('blocks.') and name.endswith('.conv.bias')


def rel(a, ref):
    return float((a.detach().double() - ref.detach().double()).abs().max() / ref.detach().double().abs().max().clamp_min(1e-300))


def run(state, kw, z, cls, w=None, masks=None, training=True, groups=1, dtype=torch.float64, **changes):
    """One call of the reference on copies of the state dict's tensors -> (generator, image, {name: gradient} | None).
    The loss is (image * w).sum(); w None: forward only."""
    params, buffers = leaves(state, dtype)
    ref = Generator(params, buffers, masks=masks, training=training, groups=groups, **dict(kw, **changes))
    if w is None:
        with torch.no_grad():
            return ref, ref(z.to(dtype), cls), None
    img = ref(z.to(dtype), cls)
    names = [n for n in params if params[n].requires_grad]
    grads = torch.autograd.grad((img * w.to(dtype)).sum(), [params[n] for n in names], allow_unused=True)
    return ref, img.detach(), {n: g for n, g in zip(names, grads) if g is not None}


def errors(img, grads, moving, ref, ref_img, ref_grads):
    """{kind: worst max|a - ref| / max|ref| over the tensors of that kind}: the image, every parameter gradient, the moving mean and
    covariance of every site (moving: {prefix: (mean, cov)}; grads / moving None: not compared).  A gradient that is zero in exact
    arithmetic is measured, on BOTH sides, against the maximum of the same layer's weight gradient."""
    errs = dict.fromkeys(KINDS, 0.0)
    assert img.shape == ref_img.shape
    errs['image'] = rel(img, ref_img)
    if grads is not None:
        assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
        for n, g in grads.items():
            assert g.shape == ref_grads[n].shape, n
            if zero_in_exact_arithmetic(n) and ref.training:
                scale = float(ref_grads[n.replace('.bias', '.weight')].abs().max())
                e = max(float(g.abs().max()), float(ref_grads[n].abs().max())) / scale
            else:
                e = rel(g, ref_grads[n])
            errs[kind_of(n)] = max(errs[kind_of(n)], e)
    if moving is not None:
        assert set(moving) == set(ref.moving)
        for prefix, (mm, mc) in moving.items():
            errs['moving'] = max(errs['moving'], rel(mm.reshape(-1), ref.moving[prefix][0].reshape(-1)), rel(mc, ref.moving[prefix][1]))
    return errs
