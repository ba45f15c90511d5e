"""Development: data gradient + weight gradient of one critic layer (128 -> 128, batch 128), hipGraph replay, three forms in one run:
sequential (wc_conv_f16x3 then wc_conv_wrw_bias_f16x3, as the backward issued them: four launches) | the same two entries on two streams |
the pair entry (wc_conv_bwd_pair_f16x3: two launches).  Each form's outputs are compared bit for bit with the sequential form's.
A library from before the pair entry (the parent's) runs too: the pair column is then empty -- the table that bounds the gain beforehand.
usage: conv_pair_bench.py [lib.so]      -> profiles/conv_pair_shapes.txt"""
import ctypes, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import _lib
if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
PAIR = ('wc_conv_bwd_pair_supported', 'wc_conv_bwd_pair_workspace_bytes', 'wc_conv_bwd_pair_f16x3')
HAS_PAIR = hasattr(ctypes.CDLL(_lib.LIB_PATH), PAIR[2])
if not HAS_PAIR:                    # an older library: no pair symbols to bind, and no layer takes the pair
    for name in PAIR:
        _lib.SIGNATURES.pop(name)
    _lib.load().wc_conv_bwd_pair_supported = lambda *a: 0
from wc_gan_amd import conv as C

N = 128
SHAPES = [  # name, kind, H, W, k
    ('2.conv1 same 8x8 3x3', 'same', 8, 8, 3),
    ('1.conv1 same 16x16 3x3', 'same', 16, 16, 3),
    ('1.conv2 down3 16->8', 'down3', 16, 16, 3),
    ('1.shortcut same 8x8 1x1', 'same', 8, 8, 1),
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
    print(f"N={N}, 128->128, us per replay: median [min,max] of {REPEATS} x {REPLAYS} replays; pair entry present: {HAS_PAIR}")
    print(f"{'layer':<28}{'sequential':>24}{'two streams':>24}{'pair':>24}")
    side = torch.cuda.Stream()
    for name, kind, H, W, k in SHAPES:
        x = torch.randn(N, H, W, 128, device='cuda')
        w = (torch.randn(128, 128, k, k, device='cuda') * 0.05).contiguous(memory_format=torch.channels_last)
        plan = C._plan(kind, x, w)
        assert plan and plan.ok
        gf, kf, nf = plan.fwd
        gb, kb, nb = plan.bwd
        gy = torch.randn(N, gf.Hout, gf.Wout, 128, device='cuda')
        xp = C.split_planes(x, relu=True)
        gp = C.split_planes(gy, colsum=True)
        img = C.weight_image(w, gb, kb, nb)

        def seq():
            dx = C.run(gp[:3], img, gb, nbytes=plan.bwd_ws)
            dw, db = C.weight_gradient(xp, gp, gf, w, kf, nf, nbytes=plan.wrw_ws, colsum=gp[3])
            return dx, dw, db

        def conc():
            cur = torch.cuda.current_stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                dw, db = C.weight_gradient(xp, gp, gf, w, kf, nf, nbytes=plan.wrw_ws, colsum=gp[3])
            dx = C.run(gp[:3], img, gb, nbytes=plan.bwd_ws)
            cur.wait_stream(side)
            return dx, dw, db

        def pair():
            return C.backward_pair(gp, img, xp, plan, w, colsum=gp[3])

        forms = [seq, conc] + ([pair] if plan.pair else [])
        ref = seq()
        torch.cuda.synchronize()
        cols = []
        for f in forms:
            f(); torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = f()
            g.replay(); torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip(out, ref))
            cols.append(fmt(timed(g)) + ('' if same else ' !BITS'))
        while len(cols) < 3:
            cols.append('-')
        print(f"{name:<28}" + ''.join(f"{c:>24}" for c in cols), flush=True)


main()
