"""The projection-critic recipes (train.CONFIGS['cifar10_cond'], train.PROJECTION_CONFIGS) on one GPU: what the fused projection tail
(csrc/wc_tail.hip) costs against torch's composition of the same tail, alone and inside the captured G+D step.
Writes profiles/projection_step.json; prints only what it measured.

Tail leg: forward + backward of the tail -- ReLU, sum pooling, the adversarial head, the projection on the class's row of the table;
gradients to y, the head and the table -- at (N, H x W, C, K) = (128, 8 x 8, 256, 10), the CIFAR-10 recipes' critic pass,
(128, 8 x 8, 256, 100), CIFAR-100's, and (128, 8 x 8, 1024, 200).  tail.projection_tail against relu -> sum -> linear + (embedding * f).sum
differentiated by autograd, which is what a PROJECTIVE critic runs without the flag; the table goes through the spectral-norm op (an
SNEmbedding in training mode) in both legs.  Each leg is captured into ONE hipGraph of `--calls` consecutive forward + backward calls; the
two graphs are replayed ALTERNATING, HIP events around each replay; a leg's figure is the median over the rounds of the time per call, its
spread max - min.

(`max_relative_gradient_difference_between_legs` compares the last call of each graph.  The power iteration advances on every call, so the
two graphs see different states of the table's u, v: for a table of many classes the figure shows that drift, not the kernels' error, which
is tests/test_projection_tail_gpu.py's subject.)

Step leg: the captured G+D step at batch 64 under the recipes' schedules: cifar10_cond and cifar100_cond_sa, each with fused_projection
True and False, replayed alternating.

The flag ships on in train.PROJECTION_CONFIGS only if the hip leg is faster than the torch leg in every round at all three shapes
(`ships_on` below).

    python tools/projection_step.py [--rounds 7] [--calls 20] [--steps 5] [--no-step] [--out profiles/projection_step.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

BATCH = 64
TAIL_SHAPES = [(128, 8, 8, 256, 10), (128, 8, 8, 256, 100), (128, 8, 8, 1024, 200)]


def _timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(v, digits=4):
    return {'values': [round(t, digits) for t in v], 'median': round(statistics.median(v), digits), 'spread': round(max(v) - min(v), digits)}


def _captured(call, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            keep = call()
    graph.replay()
    torch.cuda.synchronize()
    return graph, keep


def _tail_leg(shape, rounds, calls):
    from wc_gan_amd import tail
    from wc_gan_amd.spectral import SNEmbedding
    N, H, W, C, K = shape
    g = torch.Generator().manual_seed(0)
    y = torch.randn(N, H, W, C, generator=g).cuda().requires_grad_(True)
    size = 0.4 * H * W * C ** 0.5
    w_out = (torch.randn(1, C, generator=g) / size).cuda().requires_grad_(True)
    b_out = torch.zeros(1).cuda().requires_grad_(True)
    torch.manual_seed(0)
    emb = SNEmbedding(K, C).cuda().train()
    cls = torch.randint(0, K, (N,), generator=g, dtype=torch.int32).cuda()
    idx = cls.long()
    leaves = [y, w_out, b_out, emb.weight]
    half = N // 2

    def loss(out):              # the critic update's: the hinge loss of both halves
        return F.relu(1.0 - out[:half]).mean() + F.relu(1.0 + out[half:]).mean()

    def fused():
        return torch.autograd.grad(loss(tail.projection_tail(y, w_out, b_out, emb.normalized_weight(), cls, True)), leaves)

    def composed():
        f = F.relu(y).sum(dim=(1, 2))
        out = F.linear(f, w_out, b_out) + (F.embedding(idx, emb.normalized_weight()) * f).sum(dim=1, keepdim=True)
        return torch.autograd.grad(loss(out), leaves)

    graphs = {'torch': _captured(composed, calls), 'hip': _captured(fused, calls)}
    if tail.last_route != 'hip':
        sys.exit("projection_step.py: the tail did not run on the kernels")
    worst = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(graphs['hip'][1], graphs['torch'][1]))
    us = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (graph, _) in graphs.items():
            us[k].append(_timed(graph.replay, 10) * 1e3 / calls)
    out = {'shape': dict(N=N, HW=H * W, C=C, K=K), 'torch': _summary(us['torch'], 2), 'hip': _summary(us['hip'], 2),
           'max_relative_gradient_difference_between_legs': worst}
    out['hip_over_torch'] = round(out['hip']['median'] / out['torch']['median'], 3)
    out['hip_faster_in_every_round'] = all(a < b for a, b in zip(us['hip'], us['torch']))
    return out


def _step_leg(rounds, steps):
    from wc_gan_amd.train import CONFIGS, PROJECTION_CONFIGS, PROJECTION_SCHEDULES, RECIPE_SCHEDULES, build_trainer, fused_projection_config
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    reals = [(torch.rand(BATCH, 32, 32, 3, generator=g) * 2 - 1).cuda()]
    recipes = (('cifar10_cond', CONFIGS['cifar10_cond'], RECIPE_SCHEDULES['cifar10_cond'], 10),
               ('cifar100_cond_sa', PROJECTION_CONFIGS['cifar100_cond_sa'], PROJECTION_SCHEDULES['cifar100_cond_sa'], 100))
    legs, keep = {}, []
    for name, cfg, schedule, classes in recipes:
        labels = [torch.randint(0, classes, (BATCH,), generator=g, dtype=torch.int32).cuda()]
        on = fused_projection_config(cfg)
        off = copy.deepcopy(on)
        off['discriminator']['fused_projection'] = False
        for flag, c in ((False, off), (True, on)):
            torch.manual_seed(0)
            tr = build_trainer(c, 'cuda', batch_size=BATCH, **schedule)
            replay = tr.capture(reals, labels)
            for _ in range(3):
                losses = replay()
            torch.cuda.synchronize()
            if not all(bool(torch.isfinite(l)) for l in losses):
                sys.exit(f"projection_step.py: {name}: losses are not finite")
            legs[f'{name} fused_projection={flag}'] = replay
            keep += [tr, labels]        # the graph reads the label tensor it was captured with: it must outlive the replays
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, steps))
    out = {k: _summary(v) for k, v in ms.items()}
    for name, *_ in recipes:
        a, b = f'{name} fused_projection=True', f'{name} fused_projection=False'
        out[f'{name} fused_minus_unfused_ms'] = round(out[a]['median'] - out[b]['median'], 4)
        out[f'{name} fused_minus_unfused_ms_per_round'] = [round(x - y, 4) for x, y in zip(ms[a], ms[b])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="forward + backward calls captured into one graph (tail leg)")
    ap.add_argument("--steps", type=int, default=5, help="replays per leg and round (step leg)")
    ap.add_argument("--no-step", action="store_true", help="the tail leg alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("projection_step.py needs the GPU")
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'tail': {'what': f'us per forward + backward of the projection tail, {args.calls} calls per captured graph, the two graphs replayed alternately',
                    'rows': [_tail_leg(s, args.rounds, args.calls) for s in TAIL_SHAPES]}}
    out['tail']['ships_on'] = all(r['hip_faster_in_every_round'] for r in out['tail']['rows'])
    if not args.no_step:
        out['step'] = {'what': f'captured G+D step at batch {BATCH}, ms per step, {args.steps} replays per leg and round, alternating'}
        out['step'].update(_step_leg(args.rounds, args.steps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
