"""`make_discriminator` with the reference's keyword surface (discriminator.py:15-20).

The discriminator holds NO whitening-and-coloring site in any shipped recipe (`--discriminator_norm`
defaults to 'n', run.py:298), so it is the stock-torch part of the surrounding step: SN-ResNet blocks
on the block convolutions of wc_gan_amd/conv.py (the narrow kernels for the 3-channel first layers; their data gradient MIOpen's, or with
slim_blocks=True the narrow-output kernel's) with the fused spectral-norm op
(wc_gan_amd/spectral.py) standing in for gan.SNConv2D /
SNDense / SNEmbeding (discriminator.py:26-33).  Three heads as in discriminator.py:73-85.

arch='dcgan' (scripts/*_dcgan_sn_uncond.sh): DCBlockDown -- LeakyReLU -> Conv2D, 3x3 'same' or 4x4 stride 2 -- and the flatten tail of
discriminator.py:57-85.
"""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from .generator import Conv2D, create_norm, to_nchw_view, to_nhwc


def downsample2x(x):
    return to_nhwc(F.avg_pool2d(to_nchw_view(x), 2))


class ResBlockDown(nn.Module):
    def __init__(self, in_ch, nfilters, resample, name, norm, conv_layer, is_first):
        super().__init__()
        assert resample in ('DOWN', 'SAME')
        self.resample, self.is_first = resample, is_first
        self.bn1 = norm(axis=-1, name=name + '.bn1', channels=in_ch)
        self.conv1 = conv_layer(in_ch, nfilters, (3, 3), name=name + '.conv1')
        self.bn2 = norm(axis=-1, name=name + '.bn2', channels=nfilters)
        self.conv2 = conv_layer(nfilters, nfilters, (3, 3), name=name + '.conv2')
        self.has_shortcut = (in_ch != nfilters) or resample == 'DOWN'
        if self.has_shortcut:
            self.shortcut = conv_layer(in_ch, nfilters, (1, 1), name=name + '.shortcut')

    def _fusable(self):
        """The part of _fused_plans that does not depend on the input: a block behind the first, no norm at either site (the identity
        stack of norm 'n'), Conv2D layers of stride 1 with fp32 weights, the route switched on."""
        from . import conv as fc, generator as _g
        if self.is_first or not (fc.FUSED_BLOCK and _g.FAST_CONV):
            return False
        if not all(isinstance(bn, _g._UnfusedStack) and bn.norm_layer is None and len(bn.branches) == 0 for bn in (self.bn1, self.bn2)):
            return False
        convs = [self.conv1, self.conv2] + ([self.shortcut] if self.has_shortcut else [])
        return all(isinstance(c, Conv2D) and c.kind == 'same' and c.conv.weight.dtype == torch.float32 for c in convs)

    def _fused_plans(self, x):
        """The three convolutions' plans when the block runs as one autograd node (conv.critic_block), else None: _fusable(), a dense fp32
        NHWC input on the GPU, shapes the convolution kernel takes."""
        from . import generator as _g
        if not self._fusable():
            return None
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
                and getattr(x, '_wc_planes', None) is None and _g.split_of(x) is None):
            return None
        return self._plans_of(tuple(x.shape))

    def _plans_of(self, xshape):
        from . import conv as fc
        return fc.critic_block_plans(xshape, tuple(self.conv1.conv.weight.shape), tuple(self.conv2.conv.weight.shape),
                                     tuple(self.shortcut.conv.weight.shape) if self.has_shortcut else None, self.resample == 'DOWN',
                                     ragged=fc._ragged(self.conv1), blocks=fc._blocks(self.conv1))

    def _first_plan(self, x):
        """conv2's plan when the FIRST block's conv1 -> ReLU -> conv2 runs as one autograd node (conv.critic_first_block), else None: the
        route switched on, no norm at the second site, conv1 a narrow-input layer on an image-like fp32 GPU tensor (the layer the
        block kernels do not take), conv2 a 3x3 layer the block kernels take ('down3' in a DOWN block)."""
        from . import generator as _g
        # (any strides: the narrow kernels read a dense copy, as on the separate nodes -- the generator hands over a permuted view)
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
                and getattr(x, '_wc_planes', None) is None and _g.split_of(x) is None):
            return None
        return self._first_plan_of(tuple(x.shape))

    def _first_plan_of(self, xshape):
        """_first_plan's answer for a dense fp32 GPU tensor of this NHWC shape (the layers and the shapes alone)"""
        from . import conv as fc, generator as _g
        if not (self.is_first and fc.FIRST_BLOCK and _g.FAST_CONV):
            return None
        bn = self.bn2
        if not (isinstance(bn, _g._UnfusedStack) and bn.norm_layer is None and len(bn.branches) == 0):
            return None
        if not all(isinstance(c, Conv2D) and c.kind == 'same' and c.conv.weight.dtype == torch.float32 for c in (self.conv1, self.conv2)):
            return None
        w1, w2 = self.conv1.conv.weight, self.conv2.conv.weight
        if len(xshape) != 4 or tuple(w2.shape[2:]) != (3, 3) or w1.shape[0] <= 4:
            return None
        xs = fc._Shape(xshape)
        p1 = fc._plan('same', xs, w1, fc._ragged(self.conv1), False, fc._blocks(self.conv1))
        if (p1 and p1.ok) or not fc.narrow_shapes_supported(xshape, tuple(w1.shape)):       # (a layer the block kernels take is not conv1 on images)
            return None
        if self.resample == 'DOWN' and (xshape[1] % 2 or xshape[2] % 2):
            return None
        hs = fc._Shape(tuple(xshape[:3]) + (w1.shape[0],))
        p = fc._plan('down3' if self.resample == 'DOWN' else 'same', hs, w2, fc._ragged(self.conv2), False, fc._blocks(self.conv2))
        return p if (p and p.ok) else None

    def takes_input_planes(self, xshape):
        """Would this block, given a dense fp32 GPU tensor of this NHWC shape that the block in front has just written, run as the fused
        node -- so that the block in front may split it for conv1 (conv.critic_block's next_site) and hand the planes over?"""
        return self._fusable() and self._plans_of(tuple(xshape)) is not None

    def forward(self, x, cls, x_planes=None, handover=None):
        """x_planes: the planes of relu(x) for conv1, handed over by the block in front (only ever with a block that said
        takes_input_planes).  handover: a dict {'next': the block behind this one}; the block leaves its output's planes for that block's
        conv1 under 'planes' when its conv2 wrote them, else None.  A block given a handover runs inside the critic's pass: the finishes of its
        data gradients then take over their followers' launches too (conv.critic_block's backward_tails)."""
        if handover is not None:
            handover['planes'] = None
        plans = self._fused_plans(x)
        if plans is not None:
            from . import conv as fc
            w1, w2 = self.conv1._weight(), self.conv2._weight()
            ws = self.shortcut._weight() if self.has_shortcut else None
            x = self.bn1(x, cls)        # the identity (_fused_plans checked): called so that a forward hook on the site sees its tensor
            nxt = handover.get('next') if handover is not None else None
            g2 = plans[1].fwd[0]
            next_site = None
            if isinstance(nxt, ResBlockDown) and nxt.takes_input_planes((g2.N, g2.Hout, g2.Wout, g2.Cout)):
                next_site = nxt.conv1
            y, h, planes = fc.critic_block(x, w1, self.conv1.conv.bias, w2, self.conv2.conv.bias, ws, self.shortcut.conv.bias if self.has_shortcut else None,
                                           (self.conv1, self.conv2, self.shortcut if self.has_shortcut else None), plans, self.resample == 'DOWN',
                                           next_site=next_site, x_planes=x_planes, backward_tails=handover is not None)
            if handover is not None:
                handover['planes'] = planes
            self.bn2(h, cls)            # likewise
            return y
        if x_planes is not None:
            raise RuntimeError("ResBlockDown: planes handed to a block that does not run as the fused node")
        plan2 = self._first_plan(x)
        if plan2 is not None:
            # the first block's conv1 -> ReLU -> conv2 as one node (conv.critic_first_block); the shortcut and the add stay below
            from . import conv as fc
            h2, h = fc.critic_first_block(x, self.conv1._weight(), self.conv1.conv.bias, self.conv2._weight(), self.conv2.conv.bias,
                                          (self.conv1, self.conv2), plan2)
            self.bn2(h, cls)            # the identity (_first_plan checked): called so that a forward hook on the site sees its tensor
            s = downsample2x(x) if self.resample == 'DOWN' else x
            if self.has_shortcut:
                s = self.shortcut(s)
            return h2 + s
        # relu -> conv as one layer call: on the fast path the ReLU happens while the activation is split
        h = self.conv1(x) if self.is_first else self.conv1.forward_relu(self.bn1(x, cls))
        h = self.bn2(h, cls)
        s = x
        if self.resample == 'DOWN':
            # conv2 + average pooling as one 4x4 stride-2 convolution (same map): always on the fast kernel; with MIOpen
            # only from 32x32 on (measured 1.23 -> 0.71 ms forward+backward at 128x32x32x128, slower than the two ops at 16x16)
            from . import generator as _g
            if h.shape[1] * h.shape[2] >= 1024 or (_g.FAST_CONV and h.is_cuda):
                h = self.conv2.forward_pooled(h, relu_input=True)
            else:
                h = downsample2x(self.conv2.forward_relu(h))
            s = downsample2x(s)
        else:
            h = self.conv2.forward_relu(h)
        if self.has_shortcut:
            s = self.shortcut(s)
        return h + s


LEAKY_SLOPE = 0.3       # Keras's LeakyReLU() default (discriminator.py:59); gradient at x <= 0: slope * g (torch's convention)


class DCBlockDown(nn.Module):
    """The DC critic's block, pre-activation (`dcblock` takes `is_first` like `resblock`, and discriminator.py:59-60 applies a LeakyReLU
    behind the last block): y = conv(x) for the first block, else conv(leaky(norm(x))); SAME = 3x3 stride 1, DOWN = 4x4 stride 2, both
    Keras 'same'.  The activation and the convolution are one layer call (Conv2D.forward_leaky)."""

    def __init__(self, in_ch, nfilters, resample, name, norm, conv_layer, is_first):
        super().__init__()
        assert resample in ('DOWN', 'SAME')
        self.resample, self.is_first = resample, is_first
        self.bn = norm(axis=-1, name=name + '.bn', channels=in_ch)
        if resample == 'DOWN':
            self.conv = conv_layer(in_ch, nfilters, (4, 4), name=name + '.conv', stride=2)
        else:
            self.conv = conv_layer(in_ch, nfilters, (3, 3), name=name + '.conv')

    def forward(self, x, cls):
        if self.is_first:
            return self.conv(x)
        return self.conv.forward_leaky(self.bn(x, cls), LEAKY_SLOPE)


class Discriminator(nn.Module):
    def __init__(self, in_ch, block_sizes, resamples, norm_layer, conv_layer, dense, emb, number_of_classes, type,
                 sum_pool, dropout, arch='res', input_hw=None, fused_tail=False, fused_projection=False):
        super().__init__()
        # fused_tail: ReLU -> pooling -> heads (-> cross entropy) as the one autograd node of tail.critic_tail where
        # that covers the critic: arch='res', no dropout, type None or 'AC_GAN'.  Off by default: every other recipe keeps the torch tail
        self.fused_tail = bool(fused_tail)
        # fused_projection: the same for type 'PROJECTIVE' -- tail.projection_tail; a switch of its own, off by default
        self.fused_projection = bool(fused_projection)
        blocks = []
        ch = in_ch
        self.arch = arch
        block = ResBlockDown if arch == 'res' else DCBlockDown
        for i, (bs, rs) in enumerate(zip(block_sizes, resamples)):
            bs = int(bs)
            blocks.append(block(ch, bs, rs, 'Discriminator.' + str(i), norm_layer, conv_layer, is_first=(i == 0)))
            ch = bs
        self.blocks = nn.ModuleList(blocks)
        self.sum_pool, self.type = sum_pool, type
        self.dropout = nn.Dropout(dropout) if dropout else None
        emb_dim = ch
        if arch == 'dcgan':     # Flatten in NHWC order (discriminator.py:61-62): the heads read every grid point; sum_pool is ignored
            h, w = (int(v) for v in input_hw)
            for rs in resamples:
                if rs == 'DOWN':
                    if h % 2 or w % 2:
                        raise ValueError(f"arch='dcgan': a DOWN block halves a {h} x {w} grid")
                    h, w = h // 2, w // 2
            if type == 'PROJECTIVE' and h * w != 1:
                # the reference embeds into block_sizes[-1] dimensions while y is flattened: the product only exists on a 1 x 1 grid
                raise ValueError(f"arch='dcgan' with type='PROJECTIVE' needs a 1 x 1 final grid (the embedding has block_sizes[-1] = {ch} "
                                 f"dimensions, the flattened features {h} x {w} x {ch}); no shipped recipe combines them")
            ch = h * w * ch
        self.out = dense(ch, 1)
        if type == 'AC_GAN':
            # the class head is a plain Dense in the reference even when spectral=True (discriminator.py:74)
            self.cls_out = nn.Linear(ch, number_of_classes)
            nn.init.xavier_uniform_(self.cls_out.weight); nn.init.zeros_(self.cls_out.bias)
        elif type == 'PROJECTIVE':
            self.emb = emb(number_of_classes, emb_dim)

    def _tail_is_fused(self):
        return self.fused_tail and self.arch == 'res' and self.dropout is None and self.type in (None, 'AC_GAN')

    def _projection_is_fused(self):
        return self.fused_projection and self.arch == 'res' and self.dropout is None and self.type == 'PROJECTIVE'

    def forward(self, x, cls=None, labels=None):
        """labels (type='AC_GAN' only): the class of each sample, (N,) or (N, 1) integers -- the call then returns (out, logits, ce) with
        ce[n] the cross entropy of logits[n] against labels[n]; without labels it returns what it always did."""
        if labels is not None and self.type != 'AC_GAN':
            raise ValueError("Discriminator.forward: labels are the AC_GAN class head's; this critic has type " + repr(self.type))
        from .spectral import prepare_spectral
        prepare_spectral(self)              # all spectral-norm layers' weights in one launch (no-op without any)
        from . import conv as fc
        batch = torch.is_tensor(x) and x.is_cuda
        if batch:                           # ... and all the block convolutions' weight images in one (conv.prepare_images)
            fc.prepare_images(self, fc.pass_key(self, x))
        try:
            y, planes = x, None
            for i, blk in enumerate(self.blocks):
                if isinstance(blk, ResBlockDown):
                    # consecutive fused blocks: conv2's finish of one writes conv1's input planes of the next (conv.critic_block)
                    box = {'next': self.blocks[i + 1] if i + 1 < len(self.blocks) else None}
                    y = blk(y, cls, x_planes=planes, handover=box)
                    planes = box['planes']
                else:
                    y = blk(y, cls)
        finally:
            if batch:
                fc.finish_images(self)
        if self._tail_is_fused():
            from .tail import critic_tail
            w_out = self.out.normalized_weight() if hasattr(self.out, 'normalized_weight') else self.out.weight
            ac = self.type == 'AC_GAN'
            out, logits, ce = critic_tail(y, w_out, self.out.bias, self.cls_out.weight if ac else None, self.cls_out.bias if ac else None,
                                          labels, self.sum_pool)
            if not ac:
                return out
            return (out, logits) if labels is None else (out, logits, ce)
        if self._projection_is_fused():
            from .tail import projection_tail
            w_out = self.out.normalized_weight() if hasattr(self.out, 'normalized_weight') else self.out.weight
            table = self.emb.normalized_weight() if hasattr(self.emb, 'normalized_weight') else self.emb.weight
            return projection_tail(y, w_out, self.out.bias, table, cls, self.sum_pool)
        if self.arch == 'dcgan':
            y = F.leaky_relu(y, LEAKY_SLOPE).flatten(1)
        else:
            y = F.relu(y)
            y = y.sum(dim=(1, 2)) if self.sum_pool else y.mean(dim=(1, 2))
        if self.dropout is not None:
            y = self.dropout(y)
        out = self.out(y)
        if self.type == 'AC_GAN':
            logits = self.cls_out(y)
            if labels is None:
                return out, logits
            return out, logits, F.cross_entropy(logits, labels.reshape(-1).long(), reduction='none')
        if self.type == 'PROJECTIVE':
            out = out + (self.emb(cls.reshape(-1).long()) * y).sum(dim=1, keepdim=True)
        return out


def make_discriminator(input_image_shape=(32, 32, 3), input_cls_shape=(1,), block_sizes=(128, 128, 128, 128),
                       resamples=('DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=10,
                       type='AC_GAN', norm='n', after_norm='n', spectral=False,
                       fully_diff_spectral=False, spectral_iterations=1, conv_singular=True,
                       sum_pool=False, dropout=False, arch='res', filters_emb=10, fused_tail=False, fused_projection=False,
                       ragged_conv=False, slim_blocks=False):
    """Keyword surface AND defaults of discriminator.py:15-20.  The shipped recipes pass type / spectral / sum_pool
    explicitly (run.py:230-233 from --gan_type, --discriminator_spectral, --sum_pool default 1), as wc_gan_amd.train's
    configs do.  `conv_singular=True` (the reference's default here; run.py:270 passes 0) asks for the
    convolution-operator singular value of SNConv2D, which this harness does not build: it warns and uses the
    reshaped-kernel sigma of the SN-GAN paper.  `fused_tail`, `fused_projection` (ours, default False): see Discriminator.
    `ragged_conv`, `slim_blocks` (ours, default False): mark every convolution layer -- see generator.Conv2D."""
    assert arch in ('res', 'dcgan')
    assert type in [None, 'AC_GAN', 'PROJECTIVE']
    if spectral and conv_singular:
        import warnings
        warnings.warn("conv_singular=True is not built: spectral normalisation uses the reshaped-kernel singular value",
                      stacklevel=2)
    sn_kw = dict(spectral_iterations=spectral_iterations, fully_diff_spectral=fully_diff_spectral)
    conv_layer = partial(Conv2D, spectral=bool(spectral), conv_singular=conv_singular, ragged_conv=bool(ragged_conv), slim_blocks=bool(slim_blocks), **sn_kw)

    def dense(i, o):        # SNDense / Dense (discriminator.py:29-30)
        if spectral:
            from .spectral import SNLinear
            lin = SNLinear(i, o, **sn_kw)
            with torch.no_grad():
                nn.init.xavier_uniform_(lin.weight); nn.init.zeros_(lin.bias)
                lin._sn_init(**sn_kw)
            return lin
        lin = nn.Linear(i, o)
        nn.init.xavier_uniform_(lin.weight); nn.init.zeros_(lin.bias)
        return lin

    def emb(k, d):          # SNEmbeding / Embedding (discriminator.py:33)
        if spectral:
            from .spectral import SNEmbedding
            return SNEmbedding(k, d, **sn_kw)
        return nn.Embedding(k, d)

    norm_layer = create_norm(norm, after_norm, number_of_classes=number_of_classes, filters_emb=filters_emb)
    return Discriminator(int(input_image_shape[-1]), block_sizes, resamples, norm_layer, conv_layer, dense, emb,
                         number_of_classes, type, sum_pool, dropout, arch=arch, input_hw=input_image_shape[:2], fused_tail=fused_tail,
                         fused_projection=fused_projection)
