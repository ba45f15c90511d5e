"""The conditional WGAN-GP recipes (train.ACGAN_CONFIGS) on one GPU: what the fused critic tail (csrc/wc_tail.hip)
costs against torch's composition of the same tail, alone and inside the captured G+D step.  Writes profiles/acgan_step.json; prints only
what it measured.

Tail leg: forward + backward of the tail -- ReLU, sum pooling, the adversarial head, the class head, the cross entropy; gradients to y and
to both heads -- at (N, H x W, C, K) = (128, 8 x 8, 128, 10), the recipe's critic pass, and (128, 8 x 8, 1024, 200).  tail.critic_tail
against relu -> sum -> linear x 2 -> cross_entropy differentiated by autograd, which is what an AC_GAN critic runs without the flag.  Each
is captured into ONE hipGraph of `--calls` consecutive forward + backward calls; the two graphs are replayed ALTERNATING, HIP events around
each replay; a leg's figure is the median over the rounds of the time per call, its spread max - min.

Step leg: the captured G+D step at batch 64 under the recipe's schedule: cifar10_wgan_cond with fused_tail True and False, and
cifar10_wgan_uncond beside them (no class head, the unconditional generator), replayed alternating.

    python tools/acgan_step.py [--rounds 7] [--calls 20] [--steps 5] [--no-step] [--out profiles/acgan_step.json]
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
TAIL_SHAPES = [(128, 8, 8, 128, 10), (128, 8, 8, 1024, 200)]


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
    N, H, W, C, K = shape
    g = torch.Generator().manual_seed(0)
    y = torch.randn(N, H, W, C, generator=g).cuda().requires_grad_(True)
    size = 0.4 * H * W * C ** 0.5
    w_out = (torch.randn(1, C, generator=g) / size).cuda().requires_grad_(True)
    b_out = torch.zeros(1).cuda().requires_grad_(True)
    w_cls = (torch.randn(K, C, generator=g) / size).cuda().requires_grad_(True)
    b_cls = torch.zeros(K).cuda().requires_grad_(True)
    labels = torch.randint(0, K, (N,), generator=g).cuda()
    leaves = [y, w_out, b_out, w_cls, b_cls]
    half = N // 2

    def loss(out, ce):          # the critic update's: Wasserstein + class loss of both halves
        return out[half:].mean() - out[:half].mean() + ce[:half].mean() + ce[half:].mean()

    def fused():
        out, _logits, ce = tail.critic_tail(y, w_out, b_out, w_cls, b_cls, labels, True)
        return torch.autograd.grad(loss(out, ce), leaves)

    def composed():
        f = F.relu(y).sum(dim=(1, 2))
        out = F.linear(f, w_out, b_out)
        ce = F.cross_entropy(F.linear(f, w_cls, b_cls), labels, reduction='none')
        return torch.autograd.grad(loss(out, ce), leaves)

    graphs = {'torch': _captured(composed, calls), 'hip': _captured(fused, calls)}
    if tail.last_route != 'hip':
        sys.exit("acgan_step.py: the tail did not run on the kernels")
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
    from wc_gan_amd.train import ACGAN_CONFIGS, ACGAN_SCHEDULES, RECIPE_SCHEDULES, WGAN_CONFIGS, build_trainer
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    reals = [(torch.rand(BATCH, 32, 32, 3, generator=g) * 2 - 1).cuda()]
    labels = [torch.randint(0, 10, (BATCH,), generator=g, dtype=torch.int32).cuda()]
    plain = copy.deepcopy(ACGAN_CONFIGS['cifar10_wgan_cond'])
    plain['discriminator']['fused_tail'] = False
    fused = copy.deepcopy(plain)
    fused['discriminator']['fused_tail'] = True
    rows = (('cifar10_wgan_cond fused_tail=False', plain, ACGAN_SCHEDULES['cifar10_wgan_cond'], labels),
            ('cifar10_wgan_cond fused_tail=True', fused, ACGAN_SCHEDULES['cifar10_wgan_cond'], labels),
            ('cifar10_wgan_uncond', WGAN_CONFIGS['cifar10_wgan_uncond'], RECIPE_SCHEDULES['cifar10_wgan_uncond'], None))
    legs, keep = {}, []
    for name, cfg, schedule, lab in rows:
        torch.manual_seed(0)
        tr = build_trainer(cfg, 'cuda', batch_size=BATCH, **schedule)
        replay = tr.capture(reals, lab)
        for _ in range(3):
            losses = replay()
        torch.cuda.synchronize()
        extra = [t for t in tr.last_class_losses if t is not None] + [tr.last_penalty]
        if not all(bool(torch.isfinite(l)) for l in list(losses) + extra):
            sys.exit(f"acgan_step.py: {name}: losses are not finite")
        legs[name] = replay
        keep.append(tr)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, steps))
    out = {k: _summary(v) for k, v in ms.items()}
    a, b = 'cifar10_wgan_cond fused_tail=True', 'cifar10_wgan_cond fused_tail=False'
    out['fused_minus_unfused_ms'] = round(out[a]['median'] - out[b]['median'], 4)
    out['fused_minus_unfused_ms_per_round'] = [round(x - y, 4) for x, y in zip(ms[a], ms[b])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="forward + backward calls captured into one graph (tail leg)")
    ap.add_argument("--steps", type=int, default=5, help="replays per leg and round (step leg)")
    ap.add_argument("--no-step", action="store_true", help="the tail leg alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acgan_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("acgan_step.py needs the GPU")
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'tail': {'what': f'us per forward + backward of the critic tail, {args.calls} calls per captured graph, the two graphs replayed alternately',
                    'rows': [_tail_leg(s, args.rounds, args.calls) for s in TAIL_SHAPES]}}
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
