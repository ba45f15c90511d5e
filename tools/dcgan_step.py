"""The G+D step of the two DCGAN-SN configurations (train.DCGAN_CONFIGS) on one GPU.  Writes
profiles/dcgan_step.json; prints only what it measured.

Per configuration two legs, one captured hipGraph per leg, batch 64, training_ratio 1, generator_batch_multiple 1:
    hip     the HIP route: block kernels of csrc/wc_conv.hip (64-wide tiles, LeakyReLU in the split), narrow first layer, planes hand-off
    torch   generator.FAST_CONV = False while the leg is built and captured: the same networks on torch's / MIOpen's convolutions (the
            WC sites, the spectral-norm op and the narrow image layers are the same code in both legs)
The four graphs are replayed ALTERNATING in one process (A B C D A B C D ..., HIP events around `--steps` replays each), so clock and
temperature drift hit all legs alike; the figure of a leg is the median over the rounds, its spread max - min.
Layer leg: every block convolution of the critic (LeakyReLU -> Conv2D at the critic's batch of 2 x 64) and every deconvolution of the
generator, forward + backward (dx, dW, db) on both routes, eager, alternating; `slower_on_hip` names the layers whose HIP median is above
torch's.
Critic leg: per-kernel device-time totals of one eager critic update (forward + backward at batch 128, the critic's batch in a step) on
the HIP route, from torch's profiler.

    python tools/dcgan_step.py [--rounds 7] [--steps 20] [--out profiles/dcgan_step.json]
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BATCH = 64


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


def _leg(cfg, fast):
    import wc_gan_amd.generator as gen
    from wc_gan_amd.train import build_trainer
    gen.FAST_CONV = fast
    try:
        torch.manual_seed(0)
        tr = build_trainer(cfg, "cuda", batch_size=BATCH)
        replay = tr.capture(_reals(cfg))
        for _ in range(3):
            losses = replay()
        torch.cuda.synchronize()
        if not all(bool(torch.isfinite(l)) for l in losses):
            sys.exit("dcgan_step.py: a leg's losses are not finite")
    finally:
        gen.FAST_CONV = True
    return replay, tr


def _layers(cfg):
    """(name, kind, N, H, W, Cin, Cout) of the critic's block convolutions behind the image layer and of the generator's deconvolutions"""
    d, g = cfg['discriminator'], cfg['generator']
    H, W, c = d['input_image_shape']
    rows = []
    for i, (bs, rs) in enumerate(zip(d['block_sizes'], d['resamples'])):
        if i > 0:
            rows.append((f'Discriminator.{i}.conv', 'down' if rs == 'DOWN' else 'same', 2 * BATCH, H, W, c, int(bs)))
        if rs == 'DOWN':
            H, W = H // 2, W // 2
        c = int(bs)
    H, W, c = g['first_block_shape']
    for i, bs in enumerate(g['block_sizes']):
        rows.append((f'Generator.{i}.deconv', 'up', BATCH, H, W, c, int(bs)))
        H, W, c = 2 * H, 2 * W, int(bs)
    return rows


def _layer_leg(cfg, rounds, calls):
    import torch.nn.functional as F
    from wc_gan_amd import conv as C
    from wc_gan_amd.discriminator import LEAKY_SLOPE
    out = {}
    for name, kind, N, H, W, ci, co in _layers(cfg):
        torch.manual_seed(ci + co + H)
        x = torch.randn(N, H, W, ci, device='cuda').requires_grad_(True)
        shape = (ci, co, 4, 4) if kind == 'up' else (co, ci, 4, 4) if kind == 'down' else (co, ci, 3, 3)
        w = (torch.randn(*shape, device='cuda') / (ci * shape[2] * shape[3]) ** 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        b = torch.zeros(co, device='cuda', requires_grad=True)
        site = torch.nn.Identity()          # (something with a __dict__: the splits' scale history)
        site.train()

        def hip():
            y = C.fast_conv_or_none(x, w, b, kind, site=site, leaky_input=None if kind == 'up' else LEAKY_SLOPE)
            return y

        def tor():
            xn = x.permute(0, 3, 1, 2)
            if kind == 'up':
                y = F.conv_transpose2d(xn, w, b, stride=2, padding=1)
            else:
                y = F.conv2d(F.leaky_relu(xn, LEAKY_SLOPE), w, b, stride=2 if kind == 'down' else 1, padding=1)
            return y.permute(0, 2, 3, 1)
        y = hip()
        if y is None:
            sys.exit(f"dcgan_step.py: the HIP route does not take {name} {(kind, N, H, W, ci, co)}")
        gy = torch.randn_like(y)
        legs = {'hip': lambda: torch.autograd.grad(hip(), (x, w, b), gy), 'torch': lambda: torch.autograd.grad(tor(), (x, w, b), gy)}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ms[k].append(_timed(fn, calls))
        hm, tm = statistics.median(ms['hip']), statistics.median(ms['torch'])
        out[name] = {'layer': [kind, N, H, W, ci, co], 'hip_ms': round(hm, 4), 'torch_ms': round(tm, 4), 'hip_over_torch': round(hm / tm, 3)}
    return out


def _kernel_name(raw):
    """a kernel's plain name: without the return type, the anonymous namespace, template and call arguments, or the mangling around it"""
    m = re.match(r'_ZN?(?:12_GLOBAL__N_1)?\d+([A-Za-z_][A-Za-z0-9_]*?)(?:I|E)', raw)
    if m:
        return m.group(1)
    name = raw.replace('void ', '').replace('(anonymous namespace)::', '')
    return re.split(r'[<(]', name)[0].strip() or raw[:80]


def _critic_kernels(cfg, top=12):
    """device-time totals per kernel of one critic update (forward + backward, batch 2 x 64) on the HIP route"""
    from torch.profiler import ProfilerActivity, profile
    from wc_gan_amd.discriminator import make_discriminator
    torch.manual_seed(0)
    D = make_discriminator(**cfg['discriminator']).cuda().train()
    H, W, C = cfg['image_shape']
    x = torch.rand(2 * BATCH, H, W, C, device='cuda') * 2 - 1

    def update():
        for p in D.parameters():
            p.grad = None
        torch.relu(1.0 - D(x)).mean().backward()
    for _ in range(3):
        update()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        update()
        torch.cuda.synchronize()
    totals = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            name = _kernel_name(e.name)
            t = totals.setdefault(name, [0.0, 0])
            t[0] += e.device_time if hasattr(e, 'device_time') else e.cuda_time
            t[1] += 1
    rows = sorted(totals.items(), key=lambda kv: -kv[1][0])
    whole = sum(v[0] for v in totals.values())
    return {'device_us_total': round(whole, 1),
            'kernels': [{'kernel': k[:120], 'us': round(v[0], 1), 'launches': v[1]} for k, v in rows[:top]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20, help="replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcgan_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dcgan_step.py needs the GPU")
    from wc_gan_amd.train import DCGAN_CONFIGS
    legs, keep = {}, []
    for name, cfg in DCGAN_CONFIGS.items():
        for route, fast in (('hip', True), ('torch', False)):
            legs[(name, route)], tr = _leg(cfg, fast)
            keep.append(tr)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, args.steps))
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'steps_per_leg_and_round': args.steps, 'batch': BATCH,
           'what': 'captured G+D step (training_ratio 1, generator_batch_multiple 1), ms per step, the four graphs replayed alternately',
           'configs': {}}
    for name, cfg in DCGAN_CONFIGS.items():
        hip, tor = _summary(ms[(name, 'hip')]), _summary(ms[(name, 'torch')])
        out['configs'][name] = {'hip': hip, 'torch': tor, 'hip_over_torch': round(hip['median'] / tor['median'], 3),
                                'hip_over_torch_per_round': [round(a / b, 3) for a, b in zip(ms[(name, 'hip')], ms[(name, 'torch')])],
                                'critic_update_hip': _critic_kernels(cfg)}
        layers = _layer_leg(cfg, min(args.rounds, 5), 10)
        out['configs'][name]['layers_fwd_bwd'] = layers
        out['configs'][name]['slower_on_hip'] = sorted(k for k, v in layers.items() if v['hip_over_torch'] > 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
