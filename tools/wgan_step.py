"""The G+D step of the WGAN-GP recipe (train.WGAN_CONFIGS['cifar10_wgan_uncond']) at batch 64 on one GPU.  Writes
profiles/wgan_step.json; prints only what it measured.

Two legs, the same networks, training_ratio 5:
    hip       the shipped route: the HIP critic, the penalty in closed form on the block convolution kernels (wc_gan_amd/penalty.py)
    autograd  what a user can write without penalty.py: generator.FAST_CONV and conv.NARROW_WRW off while the leg is built and recorded
              (torch's / MIOpen's convolutions, which are differentiable twice) and the penalty by torch.autograd.grad(create_graph=True)
Both legs run in ONE mode: each as a captured hipGraph, or -- when torch's double backward cannot be recorded -- both eagerly (`mode`).
The legs alternate in one process (A B A B ..., HIP events around `--steps` steps each), so clock and temperature drift hit both alike;
a leg's figure is the median over the rounds, its spread max - min.
Critic leg: per-kernel device-time totals of one eager critic update of the hip leg (Wasserstein pass at batch 128 + penalty at batch 64),
from torch's profiler.

    python tools/wgan_step.py [--rounds 7] [--steps 10] [--out profiles/wgan_step.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

BATCH = 64
NAME = 'cifar10_wgan_uncond'


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


def _reals(cfg):
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    H, W, C = cfg['image_shape']
    return [(torch.rand(BATCH, H, W, C, generator=g) * 2 - 1).cuda()]


def _autograd_trainer(cfg):
    """the same trainer with the critic update a user can write today"""
    from wc_gan_amd.train import GanTrainer, _bump_versions, build_trainer
    from wc_gan_amd.penalty import interpolate

    class AutogradPenaltyTrainer(GanTrainer):
        def d_step(self, real, real_cls=None, fake=None, cls=None, eps=None):
            if fake is None:
                (fake,), (cls,) = self.generate(1)
            self.d_bucket.zero()
            n = real.shape[0]
            out = self._d(torch.cat([real, fake], dim=0), None)
            x_hat = interpolate(real, fake, eps).requires_grad_(True)
            g, = torch.autograd.grad(self._d(x_hat, None).sum(), x_hat, create_graph=True)
            norms = g.flatten(1).norm(dim=1)
            pen = weight * ((norms - 1) ** 2).mean()
            loss = out[n:].mean() - out[:n].mean() + pen
            loss.backward()
            self.last_penalty, self.last_grad_norms = pen.detach(), norms.detach()
            self._sync_grads(self.d_bucket)
            self.opt_d.step()
            _bump_versions(self.d_bucket.params)
            return loss.detach()

    weight = float(cfg['gradient_penalty_weight'])
    tr = build_trainer(cfg, "cuda", batch_size=BATCH, gradient_penalty_weight=0.0)
    tr.__class__ = AutogradPenaltyTrainer
    return tr


def _leg(cfg, hip, captured):
    """-> (callable that runs one G+D step, trainer); captured: as one hipGraph (raises if the step cannot be recorded)"""
    import wc_gan_amd.conv as conv
    import wc_gan_amd.generator as gen
    from wc_gan_amd.train import build_trainer
    before = gen.FAST_CONV, conv.NARROW_WRW
    gen.FAST_CONV, conv.NARROW_WRW = (before if hip else (False, False))
    try:
        torch.manual_seed(0)
        tr = build_trainer(cfg, "cuda", batch_size=BATCH) if hip else _autograd_trainer(cfg)
        reals = _reals(cfg)
        if captured:
            run = tr.capture(reals)
        else:
            if not hip:     # an eager leg reads the switches on every step
                def run():
                    keep = gen.FAST_CONV, conv.NARROW_WRW
                    gen.FAST_CONV = conv.NARROW_WRW = False
                    try:
                        return tr.step(reals)
                    finally:
                        gen.FAST_CONV, conv.NARROW_WRW = keep
            else:
                def run():
                    return tr.step(reals)
        for _ in range(3):
            losses = run()
        torch.cuda.synchronize()
        if not all(bool(torch.isfinite(l)) for l in losses) or not bool(torch.isfinite(tr.last_penalty)):
            sys.exit("wgan_step.py: a leg's losses are not finite")
    finally:
        gen.FAST_CONV, conv.NARROW_WRW = before
    return run, tr


def _critic_kernels(tr, cfg, top=16):
    """device-time totals per kernel of one eager critic update of the hip leg"""
    from torch.profiler import ProfilerActivity, profile
    from dcgan_step import _kernel_name
    real = _reals(cfg)[0]
    fake = torch.rand_like(real) * 2 - 1
    for _ in range(2):
        tr.d_step(real, fake=fake, cls=None)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        tr.d_step(real, fake=fake, cls=None)
        torch.cuda.synchronize()
    totals = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            t = totals.setdefault(_kernel_name(e.name), [0.0, 0])
            t[0] += e.device_time if hasattr(e, 'device_time') else e.cuda_time
            t[1] += 1
    rows = sorted(totals.items(), key=lambda kv: -kv[1][0])
    return {'device_us_total': round(sum(v[0] for v in totals.values()), 1),
            'kernels': [{'kernel': k[:120], 'us': round(v[0], 1), 'launches': v[1]} for k, v in rows[:top]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="steps per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgan_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wgan_step.py needs the GPU")
    if args.rounds < 5:
        sys.exit("wgan_step.py: at least 5 rounds")
    from wc_gan_amd.train import WGAN_CONFIGS
    cfg = WGAN_CONFIGS[NAME]
    mode, why = 'captured', None
    try:
        tor, tr_t = _leg(cfg, False, True)
    except Exception as exc:                    # torch's double backward could not be recorded: both legs eager
        mode, why = 'eager', f"{type(exc).__name__}: {str(exc)[:300]}"
        torch.cuda.synchronize()
        tor, tr_t = _leg(cfg, False, False)
    hip, tr_h = _leg(cfg, True, mode == 'captured')
    legs = {'hip': hip, 'autograd': tor}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, run in legs.items():
            ms[k].append(_timed(run, args.steps))
    h, t = _summary(ms['hip']), _summary(ms['autograd'])
    out = {'device': torch.cuda.get_device_name(0), 'config': NAME, 'batch': BATCH, 'training_ratio': tr_h.training_ratio, 'mode': mode,
           'rounds': args.rounds, 'steps_per_leg_and_round': args.steps,
           'what': 'G+D step, ms per step, the two legs alternating in one process',
           'hip': h, 'autograd': t, 'hip_over_autograd': round(h['median'] / t['median'], 3),
           'hip_over_autograd_per_round': [round(a / b, 3) for a, b in zip(ms['hip'], ms['autograd'])],
           'critic_update_hip': _critic_kernels(tr_h, cfg)}
    if why:
        out['capture_of_the_autograd_leg_failed_with'] = why
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
