"""Development: the k-split finishes with a tail (conv.FUSED_FINISH; csrc/wc_conv.hip conv_finish_tail_kernel) on the critic's blocks
behind the first (discriminator.ResBlockDown, 128 -> 128, batch 128, no spectral norm), forward + backward replayed from a hipGraph: the
two-launch route (FUSED_FINISH = False) against all four parts, and all with each of F1, F2, B1, B2 switched off alone.  F2 hands planes
from one block to the next, so besides the single SAME and DOWN block a DOWN -> SAME -> SAME chain (the CIFAR-10 critic's blocks 1-3) is
timed, its blocks called as Discriminator.forward calls them.  Every form's outputs are compared bit for bit with the two-launch route's.
usage: finish_split_bench.py      -> profiles/finish_split_shapes.txt"""
import copy, os, sys, statistics
from functools import partial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import conv as C
from wc_gan_amd.discriminator import ResBlockDown
from wc_gan_amd.generator import Conv2D, create_norm

N = 128
SHAPES = [  # name, resamples of the chain, H = W of its input
    ('SAME 8x8', ('SAME',), 8),
    ('DOWN 16->8', ('DOWN',), 16),
    ('DOWN,SAME,SAME', ('DOWN', 'SAME', 'SAME'), 16),
]
PARTS = ('FUSED_FINISH_F1', 'FUSED_FINISH_F2', 'FUSED_FINISH_B1', 'FUSED_FINISH_B2')
FORMS = [('two launches', False, ()), ('all four', True, ())] + [('all -' + p[-2:], True, (p,)) for p in PARTS]
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


def chain(blocks, x):
    y, planes = x, None
    for i, blk in enumerate(blocks):
        box = {'next': blocks[i + 1] if i + 1 < len(blocks) else None}
        y = blk(y, None, x_planes=planes, handover=box)
        planes = box['planes']
    return y


def main():
    print(f"N={N}, 128->128, forward + backward, us per replay: median [min,max] of {REPEATS} x {REPLAYS} replays")
    print(f"{'blocks':<16}" + ''.join(f"{f[0]:>24}" for f in FORMS))
    conv_layer = partial(Conv2D, spectral=False)
    for name, resamples, H in SHAPES:
        torch.manual_seed(0)
        proto = [ResBlockDown(128, 128, r, f'D.{i + 1}', create_norm('n', 'n'), conv_layer, is_first=False).cuda().train()
                 for i, r in enumerate(resamples)]
        x = torch.randn(N, H, H, 128, device='cuda').requires_grad_(True)
        Ho = H // 2 if 'DOWN' in resamples else H
        gy = torch.randn(N, Ho, Ho, 128, device='cuda')
        cols, ref = [], None
        try:
            for form, on, off in FORMS:
                C.FUSED_FINISH = on
                for p in PARTS:
                    setattr(C, p, p not in off)
                blocks = copy.deepcopy(proto)
                params = [p for b in blocks for p in b.parameters()]

                def call():
                    y = chain(blocks, x)
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
            C.FUSED_FINISH = True
            for p in PARTS:
                setattr(C, p, True)
        print(f"{name:<16}" + ''.join(f"{c:>24}" for c in cols), flush=True)


if __name__ == '__main__':
    main()
