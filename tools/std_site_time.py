"""Timings of the fused batch-norm site (csrc/wc_std.hip) at 128x32x32x256 and 128x16x16x256, `ucs` and `ccs` (10 classes), ReLU on.

    python tools/std_site_time.py kernels     each streaming kernel a few times next to wc_stream_copy_f32 moving the same number of
                                              bytes and a read-only pass (the moments kernel) over the same bytes -- meant to run under
                                              `rocprofv3 --kernel-trace --stats -- python tools/std_site_time.py kernels`
    python tools/std_site_time.py site        the site through the layer, forward + backward, fused against torch's route
                                              (fused_batch_norm=False), alternating in one process, HIP events, with the spread of rounds
    python tools/std_site_time.py site_conv   the fused site's forward + the 3x3 convolution behind it (what a store policy is judged by)
    python tools/std_site_time.py trace       one forward + backward of torch's route alone (its launches and bytes, under rocprofv3)
    python tools/std_site_time.py report DIR [DIR2]   the table of `kernels` from the kernel trace rocprofv3 left under DIR, and the launches
                                              of `trace` from the one under DIR2 (no GPU needed)
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(128, 32, 32, 256), (128, 16, 16, 256)]
K = 10


def stacks(after_norm, C):
    from wc_gan_amd.generator import create_norm
    torch.manual_seed(0)
    fused = create_norm('b', after_norm, number_of_classes=K, fused_batch_norm=True)(axis=-1, name='s', channels=C).cuda()
    plain = create_norm('b', after_norm, number_of_classes=K)(axis=-1, name='s', channels=C).cuda()
    return fused, plain


def kernels():
    from wc_gan_amd import _lib, ops
    lib = _lib.load()
    for shape in SHAPES:
        N, H, W, C = shape
        M = N * H * W
        for an in ('ucs', 'ccs'):
            Kc = K if an == 'ccs' else 1
            x = torch.randn(shape, device="cuda") * 2 + 1
            gy = torch.randn(shape, device="cuda")
            gamma = 1 + 0.5 * torch.randn(Kc, C, device="cuda")
            beta = 0.3 * torch.randn(Kc, C, device="cuda")
            slot = torch.randint(0, Kc, (N,), device="cuda", dtype=torch.int32) if Kc > 1 else None
            for _ in range(12):
                s, sq = ops.std_stats(x.view(M, C))
                mu, w, a, b = ops.std_factor(s, sq, M, C, 1e-3, 0.99, 0, True, None, None, gamma, beta, x.device)
                y = ops.std_apply(x, a, b, slot, relu=True)
                gsum, gxsum = ops.std_bwd_reduce(x, gy, a, b, slot, Kc, relu=True)
                _, _, q, r = ops.std_bwd_factor(gsum, gxsum, mu.view(-1), w.view(-1), gamma, M)
                dx = ops.std_bwd_apply(x, gy, a, b, q, r, slot, relu=True)
            torch.cuda.synchronize()
        # the yardstick: a copy moving as many bytes as the apply (2 M C 4) and one moving as many as the backward apply (3 M C 4: a
        # copy of 1.5 M C elements)
        src = torch.randn(3 * M * C // 2, device="cuda")
        dst = torch.empty_like(src)
        st = torch.cuda.current_stream().cuda_stream
        for n in (M * C, 3 * M * C // 2):
            for _ in range(12):
                _lib.check(lib.wc_stream_copy_f32(src.data_ptr(), dst.data_ptr(), n, st), "wc_stream_copy_f32")
        torch.cuda.synchronize()
    print("kernels: done (read the times from the profiler's kernel statistics)")


def _fwd_bwd(stack, x, cls, gy, fused):
    stack.zero_grad(set_to_none=True)
    x.grad = None
    y = stack(x, cls, relu=True) if fused else torch.relu(stack(x, cls))
    y.backward(gy)


def site(rounds=7, iters=50):
    print(f"site, forward + backward through the layer, ReLU on; ms per call = median of {rounds} alternating rounds of {iters} calls (spread = max - min)")
    for shape in SHAPES:
        for an in ('ucs', 'ccs'):
            fused, plain = stacks(an, shape[-1])
            x = (torch.randn(shape, device="cuda") * 2 + 1).requires_grad_(True)
            gy = torch.randn(shape, device="cuda")
            cls = torch.randint(0, K, (shape[0], 1), device="cuda", dtype=torch.int32)
            legs = {'fused': (fused, True), 'torch': (plain, False)}
            for st, f in legs.values():
                for _ in range(10):
                    _fwd_bwd(st, x, cls, gy, f)
            torch.cuda.synchronize()
            ms = {k: [] for k in legs}
            for _ in range(rounds):
                for k, (st, f) in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        _fwd_bwd(st, x, cls, gy, f)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / iters)
            med = {k: statistics.median(v) for k, v in ms.items()}
            spr = {k: max(v) - min(v) for k, v in ms.items()}
            nbytes = 8 * shape[0] * shape[1] * shape[2] * shape[3] * 4
            print(f"  {'x'.join(map(str, shape))} {an}: fused {med['fused']:.4f} ms (spread {spr['fused']:.4f}; {nbytes / med['fused'] / 1e9:.2f} TB/s of its 8 M C 4 bytes)  "
                  f"torch {med['torch']:.4f} ms (spread {spr['torch']:.4f})  ratio torch / fused {med['torch'] / med['fused']:.2f}  "
                  f"faster by more than the spread: {med['torch'] - med['fused'] > max(spr.values())}")


def site_conv(rounds=7, iters=50):
    """The fused site's forward followed by the convolution that reads it (Conv2D 3x3, C -> C, the block's conv2), under no_grad: what a
    store policy of the apply kernel has to be judged by (the consumer pays for what the producer saves)."""
    from wc_gan_amd.generator import Conv2D
    print(f"site forward + next 3x3 convolution, no_grad; us per call = median of {rounds} rounds of {iters} calls (spread = max - min)")
    for shape in SHAPES:
        fused, _ = stacks('ucs', shape[-1])
        conv = Conv2D(shape[-1], shape[-1], (3, 3), name='c').cuda()
        x = torch.randn(shape, device="cuda") * 2 + 1
        ms = {'site': [], 'site+conv': []}
        with torch.no_grad():
            for _ in range(10):
                conv(fused(x, None, relu=True))
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k in ms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        y = fused(x, None, relu=True)
                        if k == 'site+conv':
                            conv(y)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[k].append(1e3 * e0.elapsed_time(e1) / iters)
        print("  " + "x".join(map(str, shape)) + ": " + "  ".join(f"{k} {statistics.median(v):.1f} us (spread {max(v) - min(v):.1f})" for k, v in ms.items()))


def trace():
    shape = SHAPES[0]
    _, plain = stacks('ucs', shape[-1])
    x = (torch.randn(shape, device="cuda") * 2 + 1).requires_grad_(True)
    gy = torch.randn(shape, device="cuda")
    for _ in range(3):
        _fwd_bwd(plain, x, None, gy, False)
    torch.cuda.synchronize()
    print("trace: three forward + backward calls of torch's route at", shape)


def _trace_rows(root):
    """[(kernel name, microseconds)] in start order, from rocprofv3's kernel trace under root: the CSV, or the database newer versions write."""
    import csv
    import glob
    f = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    if f:
        rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r['Start_Timestamp']))
        return [(r['Kernel_Name'], (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows]
    import sqlite3
    db = sqlite3.connect(glob.glob(os.path.join(root, '**', '*_results.db'), recursive=True)[0])
    return [(n, (e - b) / 1e3) for n, b, e in db.execute('select name, start, "end" from kernels order by start')]


def report(root, root_torch=None):
    """kernels() launches, per shape and after-norm, 12 x [moments, combine, factor, apply, bwd reduce, combine, bwd factor, bwd apply] and then
    12 copies of 2 M C 4 bytes and 12 of 3 M C 4 bytes: the trace is read in that order; a figure is the median of a group's last 8."""
    # keyed by kernel name: the k-th launch of a kernel belongs to iteration k of kernels()' loops, whatever else ran in between
    KEY = {'moments': 'std_reduce_kernel<0>', 'bwd_reduce': 'std_reduce_kernel<1>', 'combine': 'std_combine_kernel', 'factor': 'std_factor_kernel',
           'bwd_factor': 'std_bwd_factor_kernel', 'apply': 'std_apply_kernel<false>', 'bwd_apply': 'std_apply_kernel<true>', 'copy': 'stream_copy_kernel'}
    rows = _trace_rows(root)
    seq = {k: [us for n, us in rows if v in n] for k, v in KEY.items()}
    groups = 12 * 2 * len(SHAPES)
    want = {k: groups for k in KEY}
    want['combine'] = 2 * groups            # the forward's and the backward's, alternating
    want['copy'] = 24 * len(SHAPES)
    got = {k: len(v) for k, v in seq.items()}
    assert got == want, f"launch counts {got} are not what kernels() launches {want}"
    seq['bwd_combine'] = seq['combine'][1::2]
    seq['combine'] = seq['combine'][0::2]
    take = {k: 0 for k in seq}

    def nxt(k):
        take[k] += 1
        return seq[k][take[k] - 1]
    med = lambda v: statistics.median(v[-8:])
    names = ['moments', 'combine', 'factor', 'apply', 'bwd_reduce', 'bwd_combine', 'bwd_factor', 'bwd_apply']
    bytes_of = {'moments': 1, 'apply': 2, 'bwd_reduce': 2, 'bwd_apply': 3}
    print("kernel times from rocprofv3 --kernel-trace, microseconds (median of the last 8 of 12 launches); TB/s = algorithmic bytes / time; "
          "share of 8 TB/s; ratio = time of wc_stream_copy_f32 moving the same bytes / time")
    for shape in SHAPES:
        N, H, W, C = shape
        unit = N * H * W * C * 4
        per = {}
        for an in ('ucs', 'ccs'):
            t = {k: [] for k in names}
            for _ in range(12):
                for k in names:
                    t[k].append(nxt(k))
            per[an] = {k: med(v) for k, v in t.items()}
        copy2 = med([nxt('copy') for _ in range(12)])
        copy3 = med([nxt('copy') for _ in range(12)])
        print(f"{'x'.join(map(str, shape))}: wc_stream_copy_f32 of 2 M C 4 bytes {copy2:.1f} us ({2 * unit / copy2 / 1e6:.2f} TB/s), of 3 M C 4 bytes {copy3:.1f} us "
              f"({3 * unit / copy3 / 1e6:.2f} TB/s)")
        for an in ('ucs', 'ccs'):
            for k in names:
                us = per[an][k]
                if k in bytes_of:
                    b = bytes_of[k] * unit
                    # the reductions read and write (almost) nothing: against the copy of the same bytes AND against the read-only moments pass
                    ref = {1: copy2 / 2, 2: copy2, 3: copy3}[bytes_of[k]]
                    extra = f"  vs read-only moments pass x2 {2 * per[an]['moments'] / us:.2f}" if k == 'bwd_reduce' else ""
                    print(f"  {an} {k:11s} {us:8.1f} us  {b / us / 1e6:5.2f} TB/s  {b / us / 8e6:5.2f} of 8 TB/s  copy / kernel {ref / us:.2f}{extra}")
                else:
                    print(f"  {an} {k:11s} {us:8.1f} us")
    if root_torch:
        rows = _trace_rows(root_torch)
        n = len(rows) // 3                  # trace() runs three calls; the last one is steady state
        last = rows[-n:]
        print(f"torch's route (fused_batch_norm=False), one forward + backward of a ucs site at {'x'.join(map(str, SHAPES[0]))}: {n} launches, "
              f"{sum(us for _, us in last):.1f} us of kernel time")
        for name, us in last:
            print(f"  {us:8.1f} us  {name[:150]}")


if __name__ == "__main__":
    if '--lib' in sys.argv:             # another build of the library (tools/build_var.py), for variant measurements
        i = sys.argv.index('--lib')
        from wc_gan_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    if len(sys.argv) > 2 and sys.argv[1] == 'report':
        report(*sys.argv[2:4])
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit("std_site_time.py needs the GPU")
    {'kernels': kernels, 'site': site, 'site_conv': site_conv, 'trace': trace}[sys.argv[1] if len(sys.argv) > 1 else 'site']()
