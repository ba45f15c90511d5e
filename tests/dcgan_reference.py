"""Float64 reference of the DC critic and the DC generator (arch='dcgan': discriminator.py:41-85 and generator.py:142-158 of the reference
project), written out layer by layer; plain torch, any device, not collected.

The block body (`gan.layer_utils.dcblock`) is not in the reference's tree; its call sites fix it: both networks
apply an activation BEHIND the last block and `dcblock` takes `is_first`, so the blocks are pre-activation.

Critic, from a `state_dict` of wc_gan_amd.discriminator.Discriminator and the `make_discriminator` keywords (norm 'n'), NHWC in:

    block 0:   y = conv(x)                 every other block:   y = conv(leaky(x))
    SAME = F.conv2d 3x3, padding 1         DOWN = F.conv2d 4x4, stride 2, padding 1   (Keras 'same' pads 1 and 1 there)
    tail:      leaky -> flatten in NHWC order -> the dense head `out` (+ the plain class head beside it for AC_GAN)

leaky = F.leaky_relu(., 0.3) (Keras's LeakyReLU() default; gradient 0.3 g wherever x <= 0).  Spectral normalisation exactly as in
tests/critic_reference.py: oracle.wc_oracle.spectral_normalize on the weight as a matrix in memory order, from the (u, v) the caller copied
before the forward under test.

Generator, from a `state_dict` of wc_gan_amd.generator.Generator with norm in ('n', 'b') and after-norm in ('n', 'ucs'):

    y = dense(z) viewed (N, h, w, C);  per block  y = conv_transpose2d(relu(norm(y)), 4x4, stride 2, padding 1) + bias;
    then  tanh(conv3x3(relu(final_norm(y))))

norm 'b' = training-mode batch normalisation without affine (epsilon 1e-3, biased variance), 'ucs' = gamma * . + beta per channel.

Activation masks: as in critic_reference -- `masks` (one bool NHWC tensor per activation, in the order the network applies them) replaces
the reference's own signs (leaky: h * (m + 0.3 (1 - m)); relu: h * m); `mask_disagreement` (critic_reference's) says how far from zero the
forced elements lie, against the same MASK_BAND = 1e-4.
"""
import numpy as np
import torch
import torch.nn.functional as F

from critic_reference import as_matrix, leaves, mask_disagreement      # noqa: F401  (re-exported for the tests)
from oracle import wc_oracle as O

MASK_BAND = 1e-4
SLOPE = 0.3


class Critic:
    """critic(x, cls) -> out | (out, cls_out); afterwards `pre` holds the tensor each LeakyReLU was applied to (NHWC, detached) and `uv`
    the power-iteration vectors after the forward, per spectrally normalised layer."""

    def __init__(self, params, buffers, block_sizes, resamples, type=None, spectral=False, fully_diff_spectral=False,
                 spectral_iterations=1, dropout=False, iterations=None, masks=None, **_unused):
        assert not dropout and type in (None, 'AC_GAN') and len(block_sizes) == len(resamples)
        self.p, self.b = params, buffers
        self.block_sizes, self.resamples, self.type = [int(b) for b in block_sizes], list(resamples), type
        self.spectral, self.fully_diff = bool(spectral), bool(fully_diff_spectral)
        self.iterations = int(spectral_iterations) if iterations is None else int(iterations)
        self.masks = masks
        self.pre, self.uv = [], {}

    def _weight(self, prefix, normalised=True):
        w = self.p[prefix + '.weight']
        if not (self.spectral and normalised):
            return w
        wm = as_matrix(w)
        _w, sigma_o, u, v = O.spectral_normalize(wm.detach().cpu().numpy(), self.b[prefix + '.sn_u'].cpu().numpy(),
                                                 self.b[prefix + '.sn_v'].cpu().numpy(), self.iterations)
        self.uv[prefix] = (u, v)
        ut, vt = (torch.from_numpy(np.ascontiguousarray(a)).to(w.device) for a in (u, v))
        sigma = ut @ (wm @ vt)
        assert abs(float(sigma.detach()) - sigma_o) <= 1e-12 * abs(sigma_o)
        return w / (sigma if self.fully_diff else sigma.detach())

    def _leaky(self, h):
        """h NCHW"""
        k = len(self.pre)
        self.pre.append(h.detach().permute(0, 2, 3, 1))
        if self.masks is None:
            return F.leaky_relu(h, SLOPE)
        m = self.masks[k].permute(0, 3, 1, 2)
        assert m.dtype == torch.bool and m.shape == h.shape
        m = m.to(h.dtype)
        return h * (m + SLOPE * (1 - m))

    def __call__(self, x, cls=None):
        self.pre, self.uv = [], {}
        y = x.permute(0, 3, 1, 2)
        for i, resample in enumerate(self.resamples):
            w = self._weight(f'blocks.{i}.conv.conv')
            h = y if i == 0 else self._leaky(y)
            if resample == 'DOWN':
                assert tuple(w.shape[2:]) == (4, 4)
                y = F.conv2d(h, w, self.p[f'blocks.{i}.conv.conv.bias'], stride=2, padding=1)
            else:
                assert resample == 'SAME' and tuple(w.shape[2:]) == (3, 3)
                y = F.conv2d(h, w, self.p[f'blocks.{i}.conv.conv.bias'], padding=1)
            assert y.shape[1] == self.block_sizes[i]
        y = self._leaky(y).permute(0, 2, 3, 1).flatten(1)
        out = F.linear(y, self._weight('out'), self.p['out.bias'])
        if self.type == 'AC_GAN':
            return out, F.linear(y, self._weight('cls_out', normalised=False), self.p['cls_out.bias'])
        return out


def leaky_count(block_sizes):
    """one in front of every block but the first, and the one behind the last block"""
    return len(block_sizes)


class Generator:
    """generator(z) -> image NHWC; afterwards `pre` holds the tensor each ReLU was applied to (NHWC, detached) and `sites` the shape
    (N, H, W, C) of every norm site's input, in order."""

    def __init__(self, params, first_block_shape, block_sizes, resamples=None, block_norm='n', block_after_norm='n', last_norm='n',
                 last_after_norm='n', masks=None, eps=1e-3, **_unused):
        assert block_norm in ('n', 'b') and last_norm in ('n', 'b') and block_after_norm in ('n', 'ucs') and last_after_norm in ('n', 'ucs')
        assert resamples is None or all(r == 'UP' for r in resamples)
        self.p, self.first = params, tuple(int(v) for v in first_block_shape)
        self.block_sizes = [int(b) for b in block_sizes]
        self.norms = (block_norm, block_after_norm), (last_norm, last_after_norm)
        self.masks, self.eps = masks, eps
        self.pre, self.sites = [], []

    def _norm_relu(self, h, prefix, which):
        """h NCHW"""
        norm, after = self.norms[which]
        self.sites.append((h.shape[0], h.shape[2], h.shape[3], h.shape[1]))
        if norm == 'b':
            mean = h.mean(dim=(0, 2, 3), keepdim=True)
            var = ((h - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
            h = (h - mean) / torch.sqrt(var + self.eps)
        if after == 'ucs':
            h = h * self.p[prefix + '.branches.0.gamma'].view(1, -1, 1, 1) + self.p[prefix + '.branches.0.beta'].view(1, -1, 1, 1)
        k = len(self.pre)
        self.pre.append(h.detach().permute(0, 2, 3, 1))
        if self.masks is None:
            return F.relu(h)
        return h * self.masks[k].permute(0, 3, 1, 2).to(h.dtype)

    def __call__(self, z):
        self.pre, self.sites = [], []
        y = F.linear(z, self.p['dense.weight'], self.p['dense.bias']).view(-1, *self.first).permute(0, 3, 1, 2)
        for i, width in enumerate(self.block_sizes):
            h = self._norm_relu(y, f'blocks.{i}.bn', 0)
            w = self.p[f'blocks.{i}.deconv.weight']
            assert tuple(w.shape) == (y.shape[1], width, 4, 4)
            y = F.conv_transpose2d(h, w, self.p[f'blocks.{i}.deconv.bias'], stride=2, padding=1)
        h = self._norm_relu(y, 'final_norm', 1)
        y = F.conv2d(h, self.p['final_conv.conv.weight'], self.p['final_conv.conv.bias'], padding=1)
        return torch.tanh(y).permute(0, 2, 3, 1)
