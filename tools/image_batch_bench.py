"""Development: the weight images of one CIFAR-10 critic pass (8 layers of 128 -> 128, forward and data-gradient image each, max|w| known as
the spectral-norm op leaves it) as the layers built them -- 8 launches of wc_conv_weights_pair_f32 -- and as conv.build_images builds
them -- one launch of wc_conv_weights_batch_f32; and the same without a known maximum (16 launches: sweep + pair per layer, against a
batched sweep and the batched images).  hipGraph replay, median [min, max]; every image and scale compared bit for bit in the same run.
usage: image_batch_bench.py      -> profiles/image_batch_shapes.txt"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import _lib, conv as C

N = 128
LAYERS = [  # name, kind, H, W, k: the block convolutions of discriminator blocks 0-3 at 32 x 32 images
    ('0.conv2 down3 32->16', 'down3', 32, 32, 3),
    ('1.conv1 same 16x16', 'same', 16, 16, 3), ('1.conv2 down3 16->8', 'down3', 16, 16, 3), ('1.shortcut 1x1 8x8', 'same', 8, 8, 1),
    ('2.conv1 same 8x8', 'same', 8, 8, 3), ('2.conv2 same 8x8', 'same', 8, 8, 3),
    ('3.conv1 same 8x8', 'same', 8, 8, 3), ('3.conv2 same 8x8', 'same', 8, 8, 3),
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
    torch.manual_seed(0)
    print("library:", _lib.LIB_PATH)
    print(f"N={N}, {len(LAYERS)} layers, 128->128, two images each; us per replay: median [min,max] of {REPEATS} x {REPLAYS} replays")
    for known in (True, False):
        requests = []
        for name, kind, H, W, k in LAYERS:
            x = torch.empty(N, H, W, 128, device='cuda')
            w = (torch.randn(128, 128, k, k, device='cuda') * 0.05).contiguous(memory_format=torch.channels_last)
            if known:
                w._wc_amax = torch.cat([w.abs().max().reshape(1), torch.zeros(39, device='cuda')])
            plan = C._plan(kind, x, w)
            assert plan and plan.ok
            requests.append((w, (plan.fwd, plan.bwd)))

        def per_layer():
            return [C.weight_image_pair(w, fwd, bwd) for w, (fwd, bwd) in requests]

        def batched():
            return C.build_images(requests)

        ref = per_layer()
        torch.cuda.synchronize()
        cols = []
        for f in (per_layer, batched):
            f(); torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = f()
            g.replay(); torch.cuda.synchronize()
            same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for o, r in zip(out, ref) for a, b in zip(o, r))
            cols.append(fmt(timed(g)) + ('' if same else ' !BITS'))
        what = "max|w| known" if known else "max|w| swept "
        print(f"{what}   per layer ({8 if known else 16} launches) {cols[0]}    batched ({1 if known else 2}) {cols[1]}", flush=True)


main()
