"""WC's overhead over the batch-norm generator on one GPU: the number of the reference's poster (sup-mat/iclr-2019-wc.png: 32 %).

One process builds the CIFAR-10 unconditional trainer three ways -- CONFIGS['cifar10_uncond'] (WC), baseline_config(...) (batch norm on
the fused HIP route) and baseline_config(..., fused=False) (batch norm through torch's kernels) -- warms each up, captures each G+D step
as one hipGraph (what bench.py times) and then times the three ALTERNATING, leg by leg (A B C A B C ...), HIP events around each leg.
Writes profiles/wc_overhead.json; prints only what it measured.

    python tools/wc_overhead.py [--rounds 5] [--steps 200]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="replays per leg (a leg should last well over a second)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wc_overhead.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wc_overhead.py needs the GPU")
    from wc_gan_amd.train import CONFIGS, baseline_config, build_trainer
    base = CONFIGS['cifar10_uncond']
    legs = {'wc': base, 'bn_fused': baseline_config(base), 'bn_torch': baseline_config(base, fused=False)}
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    H, W, Ci = base['image_shape']
    reals = [(torch.rand(64, H, W, Ci, generator=g) * 2 - 1).cuda() for _ in range(5)]
    replay = {}
    for name, cfg in legs.items():
        torch.manual_seed(0)
        tr = build_trainer(cfg, "cuda")
        replay[name] = tr.capture(reals)
        for _ in range(5):
            replay[name]()
        torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                replay[name]()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / args.steps)
    out = {'workload': 'CIFAR-10 ResNet-SN unconditional G+D step, batch 64, training_ratio 5, generator_batch_multiple 2, one hipGraph per step',
           'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'steps_per_leg': args.steps, 'order': list(legs), 'legs': {}}
    for name, v in ms.items():
        out['legs'][name] = {'ms_per_step': [round(t, 4) for t in v], 'median': round(statistics.median(v), 4),
                             'spread': round(max(v) - min(v), 4), 'leg_seconds': round(statistics.median(v) * args.steps / 1e3, 3)}
    med = {k: out['legs'][k]['median'] for k in legs}
    out['overhead_pct'] = round(100.0 * (med['wc'] - med['bn_fused']) / med['bn_fused'], 2)
    out['overhead_pct_per_round'] = [round(100.0 * (a - b) / b, 2) for a, b in zip(ms['wc'], ms['bn_fused'])]
    out['overhead_pct_over_torch_batch_norm'] = round(100.0 * (med['wc'] - med['bn_torch']) / med['bn_torch'], 2)
    out['poster_overhead_pct'] = 32
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
