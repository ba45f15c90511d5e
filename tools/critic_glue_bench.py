"""Development: one critic block behind the first (discriminator.ResBlockDown, 128 -> 128, batch 128, no spectral norm), forward +
backward replayed from a hipGraph: the separate autograd nodes (conv.FUSED_BLOCK = False) against the block as one node, and the one node
with each of its three parts switched off alone -- (a) the masked split, (b) the residual operand of conv2's finish, (c) the block-input
gradient in one launch.  Every form's outputs are compared bit for bit with the separate nodes'.
usage: critic_glue_bench.py      -> profiles/critic_glue_shapes.txt"""
import copy, os, sys, statistics
from functools import partial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import conv as C
from wc_gan_amd.discriminator import ResBlockDown
from wc_gan_amd.generator import Conv2D, create_norm

N = 128
SHAPES = [  # name, resample, H = W of the block's input (CIFAR-10: 16 and 8; STL-10: 24 and 12)
    ('DOWN 16->8', 'DOWN', 16),
    ('SAME 8x8', 'SAME', 8),
    ('DOWN 24->12', 'DOWN', 24),
    ('SAME 12x12', 'SAME', 12),
]
FORMS = [  # name, FUSED_BLOCK, FUSED_MASKED_SPLIT, FUSED_RESIDUAL, FUSED_BLOCK_DX
    ('separate', False, True, True, True),
    ('fused', True, True, True, True),
    ('fused -a', True, False, True, True),
    ('fused -b', True, True, False, True),
    ('fused -c', True, True, True, False),
]
REPLAYS, REPEATS = 100, 7


def timed(g):
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / REPLAYS)
    return out


def fmt(v):
    return f"{statistics.median(v):7.1f} [{min(v):6.1f},{max(v):6.1f}]"


def main():
    print(f"N={N}, 128->128, forward + backward of one block, us per replay: median [min,max] of {REPEATS} x {REPLAYS} replays")
    print(f"{'block':<14}" + ''.join(f"{f[0]:>24}" for f in FORMS))
    conv_layer = partial(Conv2D, spectral=False)
    for name, resample, H in SHAPES:
        torch.manual_seed(0)
        proto = ResBlockDown(128, 128, resample, 'D.1', create_norm('n', 'n'), conv_layer, is_first=False).cuda().train()
        x = torch.randn(N, H, H, 128, device='cuda').requires_grad_(True)
        Ho = H // 2 if resample == 'DOWN' else H
        gy = torch.randn(N, Ho, Ho, 128, device='cuda')
        assert proto._fused_plans(x) is not None, name
        cols, ref = [], None
        try:
            for form, *flags in FORMS:
                C.FUSED_BLOCK, C.FUSED_MASKED_SPLIT, C.FUSED_RESIDUAL, C.FUSED_BLOCK_DX = flags
                blk = copy.deepcopy(proto)
                params = list(blk.parameters())

                def call():
                    y = blk(x, None)
                    return (y,) + torch.autograd.grad(y, [x] + params, gy)
                call(); torch.cuda.synchronize()            # the sites' first call measures and allocates their records
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = call()
                g.replay(); torch.cuda.synchronize()
                if ref is None:
                    ref = [o.clone() for o in out]
                same = all(torch.equal(a, b) for a, b in zip(out, ref))
                cols.append(fmt(timed(g)) + ('' if same else ' !BITS'))
        finally:
            C.FUSED_BLOCK = C.FUSED_MASKED_SPLIT = C.FUSED_RESIDUAL = C.FUSED_BLOCK_DX = True
        print(f"{name:<14}" + ''.join(f"{c:>24}" for c in cols), flush=True)


if __name__ == '__main__':
    main()
