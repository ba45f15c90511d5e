"""The optimiser update of the headline recipe (train.CIFAR10_UNCOND) on one GPU: torch's fused capturable Adam against
optim.ScheduledAdam (csrc/wc_adam.hip).  Writes profiles/adam_step.json; prints only what it measured.

Update leg, per network (generator, critic): both optimisers over their own copy of the network's parameters and the same static
gradients, each captured into ONE hipGraph of `--updates` consecutive updates (so a replay's launch cost is spread over them); the graphs
of a network are replayed ALTERNATING, HIP events around each replay; a leg's figure is the median over the rounds of the time per update,
its spread max - min.  `bytes` is what the formula has to move (torch: 7 fp32 streams = 28 bytes per parameter; ScheduledAdam at beta1 = 0:
5 streams = 20), `fraction_of_8TBps` = bytes / time / 8e12.  The parameter sets (a few tens of MB) fit the 256 MiB Infinity Cache and
nothing else runs between the updates here, so this fraction is a rate of the update formula's bytes, not measured HBM traffic.

Step leg: the captured G+D step at batch 64 with optimizer='hip' against the default, alternating.

    python tools/adam_step.py [--rounds 7] [--updates 20] [--steps 10] [--chunk N] [--no-step] [--out profiles/adam_step.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH = 64
LR, BETAS = 2e-4, (0.0, 0.9)


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


def _captured(step, updates):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(updates):
            step()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def _update_leg(module, rounds, updates):
    from wc_gan_amd.optim import ScheduledAdam
    torch.manual_seed(0)
    base = [p for p in module.parameters() if p.requires_grad]
    grads = [torch.randn_like(p) * 1e-2 for p in base]
    sets = {}
    for route in ('torch', 'hip'):
        ps = [p.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for p in base]
        for p, g in zip(ps, grads):
            p.grad = g
        opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, capturable=True, fused=True) if route == 'torch' else ScheduledAdam(ps, LR, BETAS)
        sets[route] = (ps, opt, _captured(opt.step, updates))
    us = {k: [] for k in sets}
    for _ in range(rounds):
        for k, (_, _, graph) in sets.items():
            us[k].append(_timed(graph.replay, 10) * 1e3 / updates)
    n = sum(p.numel() for p in base)
    out = {'tensors': len(base), 'parameters': n, 'launches_per_update_hip': 1 + len(sets['hip'][1]._tables)}
    for k, per_param in (('torch', 28), ('hip', 20)):
        s = _summary(us[k], 2)
        out[k] = {'us_per_update': s, 'bytes': per_param * n, 'fraction_of_8TBps': round(per_param * n / (s['median'] * 1e-6) / 8e12, 4)}
    out['hip_over_torch'] = round(out['hip']['us_per_update']['median'] / out['torch']['us_per_update']['median'], 3)
    # the two legs ran the same number of updates on the same gradients: their parameters agree to the parameters' rounding
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(sets['torch'][0], sets['hip'][0]))
    out['max_abs_parameter_difference_between_legs'] = worst
    return out


def _step_leg(rounds, steps):
    from wc_gan_amd.train import CIFAR10_UNCOND, build_trainer
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    reals = [(torch.rand(BATCH, 32, 32, 3, generator=g) * 2 - 1).cuda()]
    legs, keep = {}, []
    for route, kw in (('torch', dict()), ('hip', dict(optimizer='hip'))):
        torch.manual_seed(0)
        tr = build_trainer(CIFAR10_UNCOND, 'cuda', batch_size=BATCH, **kw)
        replay = tr.capture(reals)
        for _ in range(3):
            losses = replay()
        torch.cuda.synchronize()
        if not all(bool(torch.isfinite(l)) for l in losses):
            sys.exit("adam_step.py: a leg's losses are not finite")
        legs[route] = replay
        keep.append(tr)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, steps))
    out = {k: _summary(v) for k, v in ms.items()}
    out['hip_minus_torch_ms'] = round(out['hip']['median'] - out['torch']['median'], 4)
    out['hip_minus_torch_ms_per_round'] = [round(a - b, 4) for a, b in zip(ms['hip'], ms['torch'])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=20, help="updates captured into one graph (update leg)")
    ap.add_argument("--steps", type=int, default=10, help="replays per leg and round (step leg)")
    ap.add_argument("--chunk", type=int, default=None, help="elements per workgroup of the update kernel (default: optim.CHUNK)")
    ap.add_argument("--no-step", action="store_true", help="the update leg alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_step.py needs the GPU")
    from wc_gan_amd import optim
    from wc_gan_amd.discriminator import make_discriminator
    from wc_gan_amd.generator import make_generator
    from wc_gan_amd.train import CIFAR10_UNCOND
    if args.chunk is not None:
        optim.CHUNK = args.chunk
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'config': 'cifar10_uncond', 'chunk': optim.CHUNK,
           'update': {'what': f'us per optimiser update, {args.updates} updates per captured graph, the two graphs replayed alternately'},
           'step': {'what': f'captured G+D step at batch {BATCH}, ms per step, {args.steps} replays per leg and round, alternating'}}
    torch.manual_seed(0)
    nets = {'generator': make_generator(**CIFAR10_UNCOND['generator']).cuda(), 'critic': make_discriminator(**CIFAR10_UNCOND['discriminator']).cuda()}
    for name, net in nets.items():
        out['update'][name] = _update_leg(net, args.rounds, args.updates)
    del nets
    if args.no_step:
        del out['step']
    else:
        out['step'].update(_step_leg(args.rounds, args.steps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
