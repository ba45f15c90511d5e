"""Development: the critic's first block as one autograd node (conv.FIRST_BLOCK; csrc/wc_conv.hip conv_fwd_narrow_split_kernel and
conv_wrw_narrow_masked_kernel) at the CIFAR-10 critic's shape -- discriminator.ResBlockDown(3 -> 128, DOWN, is_first) on 128x32x32x3,
no spectral norm -- forward + backward replayed from a hipGraph: the separate nodes (FIRST_BLOCK = False) against both parts, each part
switched off alone, and both with conv1's fp32 output leaving as non-temporal stores.  Two passes: the critic's own update (the image needs
no gradient: the mask rides in conv1's weight gradient) and the critic pass of the generator's update (it does: threshold_backward stays).
Every form's outputs are compared bit for bit with the separate nodes' in the same run (the image's gradient excepted: MIOpen's data
gradient, the same call on every route, is not reproducible from one call to the next).
usage: first_block_bench.py      -> profiles/first_block_shapes.txt"""
import copy, os, sys, statistics
from functools import partial
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import conv as C
from wc_gan_amd.discriminator import ResBlockDown
from wc_gan_amd.generator import Conv2D, create_norm

N, H = 128, 32
FLAGS = ('FIRST_BLOCK', 'FIRST_BLOCK_PLANES', 'FIRST_BLOCK_MASK', 'FIRST_BLOCK_NT')
FORMS = [('separate nodes', (False, True, True, False)), ('planes + mask', (True, True, True, False)), ('mask only', (True, False, True, False)),
         ('planes only', (True, True, False, False)), ('planes(nt) + mask', (True, True, True, True))]
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
    print(f"block 0: {N}x{H}x{H}x3 -> 128, DOWN, forward + backward, us per replay: median [min,max] of {REPEATS} x {REPLAYS} replays")
    print(f"{'pass':<18}" + ''.join(f"{f[0]:>26}" for f in FORMS))
    old = {k: getattr(C, k) for k in FLAGS}
    torch.manual_seed(0)
    proto = ResBlockDown(3, 128, 'DOWN', 'D.0', create_norm('n', 'n'), partial(Conv2D, spectral=False), is_first=True).cuda().train()
    gy = torch.randn(N, H // 2, H // 2, 128, device='cuda')
    for name, need_x in (('critic update', False), ('generator update', True)):
        x = (torch.rand(N, H, H, 3, device='cuda') * 2 - 1).requires_grad_(need_x)
        cols, ref = [], None
        try:
            for form, values in FORMS:
                for k, v in zip(FLAGS, values):
                    setattr(C, k, v)
                blk = copy.deepcopy(proto)
                params = list(blk.parameters())

                def call():
                    y = blk(x, None)
                    return (y,) + torch.autograd.grad(y, params + ([x] if need_x else []), gy)
                call(); torch.cuda.synchronize()            # the sites' first call measures and allocates their records
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    out = call()
                g.replay(); torch.cuda.synchronize()
                out = out[:1 + len(params)]                 # (without the image's gradient: see above)
                if ref is None:
                    ref = [o.clone() for o in out]
                same = all(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) for a, b in zip(out, ref))
                cols.append(fmt(timed(g)) + ('' if same else ' !BITS'))
        finally:
            for k, v in old.items():
                setattr(C, k, v)
        print(f"{name:<18}" + ''.join(f"{c:>26}" for c in cols), flush=True)


if __name__ == '__main__':
    main()
