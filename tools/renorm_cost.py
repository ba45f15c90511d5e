"""What a renorm ('dr') site costs on one GPU.  Writes profiles/renorm_cost.json; prints only what it measured.

Site leg: one WC site, forward + backward, `uconv` coloring, at 128x32x32x256 and 128x8x8x256, timed ALTERNATING in one process
(A B C A B C ..., HIP events around each leg):
    d          the plain Cholesky site, create_norm('d', 'uconv')
    dr         the renorm site on the fused route, create_norm('dr', 'uconv'): ops.renorm around K2, W_m in the coloring, ops.bwd_factor_renorm
    dr_parent  the composition the layer ran before it had that route, rebuilt here from public ops: a second moments pass (ops.stats), two
               ops.factor calls, C0 = W_m L_batch folded into the coloring by a torch matmul that stays in the autograd graph, then the plain site
The three legs see the same input, the same coloring weights and the same moving statistics (restored before every call); before anything
is timed the tool checks that 'dr' and 'dr_parent' agree on y and dx to 1e-4.
Step leg (optional, --step): the CIFAR-10 unconditional G+D step with CONFIGS['cifar10_uncond'] against train.renorm_config(...) of it, one
captured graph each, alternating.  A renorm layer has no grouped form, so the 'dr' trainer runs SEPARATE generator passes where the 'd'
trainer runs one grouped pass (GanTrainer.generate): the step figure measures that too, not the site alone.

    python tools/renorm_cost.py [--rounds 7] [--calls 30] [--step] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

EPS, MOMENTUM = 1e-3, 0.99
SHAPES = ((128, 32, 32, 256), (128, 8, 8, 256))


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(v):
    return {'ms': [round(t, 4) for t in v], 'median': round(statistics.median(v), 4), 'spread': round(max(v) - min(v), 4)}


def _parent_fold(x, gamma, moving_mean, moving_cov):
    """Gamma' = (W_m L_batch)^T Gamma as the layer's _renorm_gamma built it: its own pass over x, two factor calls, a torch matmul."""
    from wc_gan_amd import ops
    C = x.shape[-1]
    with torch.no_grad():
        s, xtx = ops.stats(x.contiguous().view(-1, C))
        M = x.numel() // C
        _, Lb, _ = ops.factor(s, xtx, M, C, EPS, MOMENTUM, 1, True, None, None, x.device)
        _, _, Wm = ops.factor(None, None, M, C, EPS, MOMENTUM, 1, False, moving_mean.view(-1), moving_cov, x.device)
        C0t = (Wm @ Lb).t().to(torch.float32)
    return torch.matmul(C0t.unsqueeze(0), gamma)


def site_leg(shape, rounds, calls):
    from oracle import wc_oracle as o
    from wc_gan_amd.functional import whiten_color
    from wc_gan_amd.generator import create_norm
    C = shape[-1]
    rng = np.random.default_rng(C + shape[1])
    x = torch.tensor((1.3 * o.synth_activation(rng, shape, 'well') + 0.1).astype(np.float32), device='cuda').requires_grad_(True)
    gy = torch.tensor(rng.standard_normal(shape).astype(np.float32), device='cuda')
    mm0, mc0 = o.moments_to_stats(*o.batch_moments(o.synth_activation(rng, (16 * C, C), 'well')))
    mm0 = torch.tensor(mm0.astype(np.float32), device='cuda').view(C, 1)
    mc0 = torch.tensor(mc0.astype(np.float32), device='cuda')
    stacks = {}
    for name, norm in (('d', 'd'), ('dr', 'dr')):
        torch.manual_seed(1)
        stacks[name] = create_norm(norm, 'uconv')(axis=-1, name=name, channels=C).cuda()
    d, dr = stacks['d'], stacks['dr']
    params = list(dr.parameters())

    def reset(stack):
        stack.npart.moving_mean.copy_(mm0); stack.npart.moving_cov.copy_(mc0)

    def through(stack):
        def run():
            reset(stack)
            y = stack(x, None, relu=True)
            return y, torch.autograd.grad(y, [x] + list(stack.parameters()), gy)
        return run

    def parent():
        reset(dr)
        gamma, beta, slot, _ = dr.coloring_table(x, None)
        g = _parent_fold(x, gamma, dr.npart.moving_mean, dr.npart.moving_cov)
        y = whiten_color(x, g.contiguous(), beta.contiguous(), slot, dr.npart.moving_mean, dr.npart.moving_cov, True, EPS, MOMENTUM, 1,
                         None, relu=True)
        return y, torch.autograd.grad(y, [x] + params, gy)

    legs = {'d': through(d), 'dr': through(dr), 'dr_parent': parent}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    (ya, ga), (yb, gb) = legs['dr'](), legs['dr_parent']()
    agree = {'y': float((ya - yb).abs().max() / yb.abs().max()), 'dx': float((ga[0] - gb[0]).abs().max() / gb[0].abs().max())}
    if max(agree.values()) > 1e-4:
        sys.exit(f"renorm_cost.py: the fused 'dr' site and the parent composition disagree at {shape}: {agree}")
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(_timed(fn, calls))
    out = {name: _summary(v) for name, v in ms.items()}
    out['dr_vs_parent_agreement'] = {k: float(f"{v:.3g}") for k, v in agree.items()}
    out['dr_over_parent'] = round(out['dr']['median'] / out['dr_parent']['median'], 3)
    out['dr_over_parent_per_round'] = [round(a / b, 3) for a, b in zip(ms['dr'], ms['dr_parent'])]
    out['dr_over_d'] = round(out['dr']['median'] / out['d']['median'], 3)
    return out


def step_leg(rounds, steps):
    from wc_gan_amd.train import CONFIGS, build_trainer, renorm_config
    base = CONFIGS['cifar10_uncond']
    legs = {'d': base, 'dr': renorm_config(base)}
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    H, W, Ci = base['image_shape']
    reals = [(torch.rand(64, H, W, Ci, generator=g) * 2 - 1).cuda() for _ in range(5)]
    replay = {}
    for name, cfg in legs.items():
        torch.manual_seed(0)
        tr = build_trainer(cfg, "cuda")
        replay[name] = tr.capture(reals)
        for _ in range(3):
            replay[name]()
        torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(rounds):
        for name in legs:
            ms[name].append(_timed(replay[name], steps))
    out = {name: _summary(v) for name, v in ms.items()}
    out['dr_over_d'] = round(out['dr']['median'] / out['d']['median'], 3)
    out['workload'] = ('CIFAR-10 ResNet-SN unconditional G+D step, batch 64, training_ratio 5, generator_batch_multiple 2, one hipGraph per step; '
                       "the 'dr' trainer runs separate generator passes (renorm has no grouped form), the 'd' trainer one grouped pass")
    out['steps_per_leg'] = steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30, help="site leg: calls per leg and round")
    ap.add_argument("--step", action="store_true", help="also time the CIFAR-10 step with renorm_config")
    ap.add_argument("--steps", type=int, default=20, help="step leg: replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "renorm_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("renorm_cost.py needs the GPU")
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'calls_per_leg': args.calls, 'eps': EPS,
           'what': "one WC site, forward + backward (dx, dGamma, dbeta), uconv coloring with the ReLU folded, eager; ms per call",
           'site': {'x'.join(map(str, s)): site_leg(s, args.rounds, args.calls) for s in SHAPES}}
    out['condition'] = {'dr_not_slower_than_parent': {k: v['dr_over_parent'] <= 1.0 for k, v in out['site'].items()}}
    if args.step:
        out['step'] = step_leg(args.rounds, args.steps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
