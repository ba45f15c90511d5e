"""Development: the k-split whose shares are summed inside the workgroup (conv.LOCAL_KSPLIT; csrc/wc_conv.hip conv_local_kernel) on the
critic's eligible layer shapes at batch 128 -- the SAME blocks' 3x3 convolutions at 8x8 (forward and data gradient) and the DOWN block's
conv2 (16x16 -> 8x8) -- one convolution with each finish it runs with, replayed from a hipGraph that holds CALLS of them: the two launches
(LOCAL_KSPLIT = False) against the one.  Every form's outputs are compared bit for bit between the routes in the same run.
usage: local_ksplit_bench.py      -> profiles/local_ksplit_shapes.txt"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from wc_gan_amd import _lib, conv as C

N, CALLS = 128, 8
SHAPES = [  # name, kind, x's shape, geometry ('fwd' | 'bwd'), the forms it runs with
    ('SAME 8x8 forward', 'same', (N, 8, 8, 128), 'fwd', ('plain', 'res', 'split', 'split+res')),
    ('DOWN 16->8 conv2', 'down3', (N, 16, 16, 128), 'fwd', ('plain', 'res', 'split', 'split+res')),
    ('SAME 8x8 data gradient', 'same', (N, 8, 8, 128), 'bwd', ('plain', 'masked', 'dx')),
]
REPLAYS, REPEATS = 100, 7


class Site:
    training = True


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
        out.append(a.elapsed_time(b) * 1000.0 / (REPLAYS * CALLS))
    return out


def fmt(v):
    return f"{statistics.median(v):6.1f} [{min(v):5.1f},{max(v):5.1f}]"


def main():
    default = C.LOCAL_KSPLIT
    print(f"N={N}, 128->128, one convolution with its finish, us per call: median [min,max] of {REPEATS} x {REPLAYS} replays of {CALLS} calls")
    print(f"{'layer':<24}{'finish':<12}{'two launches':>22}{'one launch':>22}{'saved':>8}")
    for name, kind, shape, side, forms in SHAPES:
        torch.manual_seed(0)
        w = (torch.randn(128, 128, 3, 3, device='cuda') * 0.05).contiguous(memory_format=torch.channels_last)
        b = torch.randn(128, device='cuda') * 0.1
        plan = C._plan(kind, C._Shape(shape), C._Shape(tuple(w.shape)))
        img, bimg = C.weight_image_pair(w, plan.fwd, plan.bwd)
        g, image, nbytes = (plan.fwd[0], img, plan.fwd_ws) if side == 'fwd' else (plan.bwd[0], bimg, plan.bwd_ws)
        assert plan.local if side == 'fwd' else plan.bwd_local
        out = (g.N, g.Hout, g.Wout, g.Cout)
        x_pl = C.split_planes(torch.randn((g.N, g.Hin, g.Win, g.Cin), device='cuda'), relu=side == 'fwd')[:3]
        res, mask, other = (torch.randn(out, device='cuda') for _ in range(3))
        bias = b if side == 'fwd' else None
        for form in forms:
            cols, ref = [], None
            try:
                for local in (False, True):
                    C.LOCAL_KSPLIT = local
                    site = Site()
                    role = 'x' if side == 'fwd' else 'g'
                    y0 = C.run(x_pl, image, g, bias, nbytes=nbytes)
                    if form == 'masked':
                        C.split_planes_masked(y0, mask, site=site, role=role)       # (seeds the reader's record)
                    else:
                        C.split_planes(y0 + res if form == 'split+res' else y0, relu=True, site=site, role=role)

                    def call():
                        if form == 'plain':
                            return (C.run(x_pl, image, g, bias, nbytes=nbytes),)
                        if form == 'res':
                            return (C.run(x_pl, image, g, bias, nbytes=nbytes, res=res),)
                        if form == 'dx':
                            t = C._Tail(_lib.TAIL_DX, out, w.device, mask=mask, other=other)
                            C.run_tail(x_pl, image, g, t, nbytes=nbytes)
                            return (t.out,)
                        rec = C._reader_record(site, role, w.device)
                        if form == 'masked':
                            t = C._Tail(_lib.TAIL_MASKED, out, w.device, record=rec, role=role, mask=mask)
                        else:
                            t = C._Tail(_lib.TAIL_SPLIT, out, w.device, record=rec, role=role, res=res if form == 'split+res' else None)
                        return (C.run_tail(x_pl, image, g, t, bias=bias, nbytes=nbytes), t.planes[0], t.planes[1], t.planes[2][:1])
                    call(); torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        for _ in range(CALLS):
                            o = call()
                    graph.replay(); torch.cuda.synchronize()
                    if ref is None:
                        ref = [t.clone() for t in o]
                    same = all(torch.equal(a, e) for a, e in zip(o, ref))
                    cols.append((timed(graph), same))
            finally:
                C.LOCAL_KSPLIT = default
            (told, _), (tnew, same) = cols
            print(f"{name:<24}{form:<12}{fmt(told):>22}{fmt(tnew):>22}{statistics.median(told) - statistics.median(tnew):>8.1f}"
                  + ('' if same else ' !BITS'), flush=True)


if __name__ == '__main__':
    main()
