"""The G+D step of the two MNIST configurations (train.MNIST_CONFIGS 'mnist_uncond' and 'mnist_cond') on one GPU,
with the block convolutions' partial last tile on and off.  Writes profiles/mnist_step.json; prints only what it measured.

Per configuration two legs, one captured hipGraph per leg, batch 64, the trainer's defaults (training_ratio 5, generator_batch_multiple 2):
    ragged  train.ragged_config(cfg): every convolution layer marked ragged_conv -- the 7x7 layers whose N*H*W is a multiple of 32 run the
            block kernels of csrc/wc_conv.hip on a partial last tile, their WC sites hand planes over
    off     train.ragged_config(cfg, on=False): the same networks unmarked -- those layers on torch's / MIOpen's convolutions
The four graphs are replayed ALTERNATING in one process (A B C D A B C D ..., HIP events around `--steps` replays each), so clock and
temperature drift hit all legs alike; the figure of a leg is the median over the rounds, its spread max - min.  `ragged_faster_every_round`
is the rule train.MNIST_RAGGED_SHIPS follows: the mark ships on only if it is true for both configurations.
Layer leg: every 7x7 convolution of the two networks, forward + backward (dx, dW, db), on both routes: the device time of its kernels per
call (torch's profiler, summed over the call's kernels), and which grids the step itself gives them (N = 64 x rounds in the generation,
2 x 64 in the critic's updates, 64 x generator_batch_multiple in the generator's).

    python tools/mnist_step.py [--rounds 7] [--steps 10] [--out profiles/mnist_step.json]
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
NAMES = ('mnist_uncond', 'mnist_cond')


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


def _leg(cfg, on):
    from wc_gan_amd.train import build_trainer, ragged_config
    torch.manual_seed(0)
    tr = build_trainer(ragged_config(cfg, on=on), "cuda", batch_size=BATCH)
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    H, W, C = cfg['image_shape']
    reals = [(torch.rand(BATCH, H, W, C, generator=g) * 2 - 1).cuda() for _ in range(tr.training_ratio)]
    labels = [torch.randint(0, 10, (BATCH,), generator=g, dtype=torch.int32).cuda() for _ in range(tr.training_ratio)] if cfg['conditional'] else None
    replay = tr.capture(reals, labels)
    for _ in range(3):
        losses = replay()
    torch.cuda.synchronize()
    if not all(bool(torch.isfinite(l)) for l in losses):
        sys.exit("mnist_step.py: a leg's losses are not finite")
    # the graph reads the real batches and the label tensors it was captured with (GanTrainer.capture keeps no reference of its own): they
    # must outlive the replays -- a freed label tensor's memory is handed to the next leg, and the class gathers then index with its bytes
    return replay, (tr, reals, labels)


def _layers(cfg):
    """(name, kind, N, H, W, Cin, Cout, k, where) of the 7x7 convolutions: N as the step's passes give it"""
    F_ = cfg['generator']['first_block_shape'][2]
    rows = [('Generator.0.conv1', 'up3', 5 * BATCH, 7, 7, F_, F_, 3, 'generation, 5 rounds'),
            ('Generator.0.conv1', 'up3', BATCH, 7, 7, F_, F_, 3, 'a generator pass of 64'),
            ('Generator.0.shortcut', 'same', 5 * BATCH, 7, 7, F_, F_, 1, 'generation, 5 rounds'),
            ('Generator.0.shortcut', 'same', BATCH, 7, 7, F_, F_, 1, 'a generator pass of 64'),
            ('Discriminator.1.conv2', 'down3', BATCH, 14, 14, 128, 128, 3, 'a critic pass of 64'),
            ('Discriminator.1.shortcut', 'same', BATCH, 7, 7, 128, 128, 1, 'a critic pass of 64'),
            ('Discriminator.2.conv1', 'same', BATCH, 7, 7, 128, 128, 3, 'a critic pass of 64 (2.conv2, 3.conv1, 3.conv2 alike)')]
    return rows


def _device_us(fn, calls):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    total = 0.0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            total += e.device_time if hasattr(e, 'device_time') else e.cuda_time
    return total / calls


def _layer_leg(cfg, calls):
    import torch.nn.functional as F
    from wc_gan_amd import conv as C
    out = []
    for name, kind, N, H, W, ci, co, k, where in _layers(cfg):
        torch.manual_seed(ci + co + H)
        x = torch.randn(N, H, W, ci, device='cuda').requires_grad_(True)
        w = (torch.randn(co, ci, k, k, device='cuda') / (ci * k * k) ** 0.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        b = torch.zeros(co, device='cuda', requires_grad=True)
        site = torch.nn.Identity()          # (something with a __dict__: the splits' scale history, and the mark)
        site.train()
        site.ragged_conv = True
        plain = torch.nn.Identity()         # (the unmarked layer)
        plain.train()

        def hip():
            return C.fast_conv_or_none(x, w, b, kind, site=site)

        def tor():                          # the unmarked layer's route: generator.Conv2D.forward / forward_pooled / ResBlockUp below 8x8
            xn = x.permute(0, 3, 1, 2)
            if kind == 'up3':
                up = F.interpolate(xn, scale_factor=2, mode='nearest').permute(0, 2, 3, 1).contiguous()
                return C.fast_conv_or_none(up, w, b, 'same', site=plain) if N * 4 * H * W % 128 == 0 else \
                    F.conv2d(up.permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
            if kind == 'down3':
                kk = (F.pad(w, (0, 1, 0, 1)) + F.pad(w, (1, 0, 0, 1)) + F.pad(w, (0, 1, 1, 0)) + F.pad(w, (1, 0, 1, 0))) * 0.25
                return F.conv2d(xn, kk.contiguous(memory_format=torch.channels_last), b, stride=2, padding=1).permute(0, 2, 3, 1)
            return F.conv2d(xn, w, b, padding=k // 2).permute(0, 2, 3, 1)
        y = hip()
        if y is None:
            sys.exit(f"mnist_step.py: the marked route does not take {name} {(kind, N, H, W, ci, co)}")
        gy = torch.randn_like(y)
        legs = {'ragged': lambda: torch.autograd.grad(hip(), (x, w, b), gy), 'off': lambda: torch.autograd.grad(tor(), (x, w, b), gy)}
        us = {}
        for key, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us[key] = _device_us(fn, calls)
        out.append({'layer': name, 'where': where, 'shape': [kind, N, H, W, ci, co, k], 'ragged_us': round(us['ragged'], 1),
                    'off_us': round(us['off'], 1), 'ragged_over_off': round(us['ragged'] / us['off'], 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10, help="replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnist_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mnist_step.py needs the GPU")
    from wc_gan_amd.train import MNIST_CONFIGS
    legs, keep = {}, []
    for name in NAMES:
        for route, on in (('ragged', True), ('off', False)):
            legs[(name, route)], held = _leg(MNIST_CONFIGS[name], on)
            keep.append(held)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, args.steps))
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'steps_per_leg_and_round': args.steps, 'batch': BATCH,
           'what': 'captured G+D step (training_ratio 5, generator_batch_multiple 2), ms per step, the four graphs replayed alternately',
           'configs': {}}
    for name in NAMES:
        on, off = _summary(ms[(name, 'ragged')]), _summary(ms[(name, 'off')])
        per_round = [round(a / b, 4) for a, b in zip(ms[(name, 'ragged')], ms[(name, 'off')])]
        out['configs'][name] = {'ragged': on, 'off': off, 'ragged_over_off': round(on['median'] / off['median'], 4),
                                'ragged_over_off_per_round': per_round, 'ragged_faster_every_round': all(r < 1.0 for r in per_round),
                                'layers_7x7_fwd_bwd_device_us': _layer_leg(MNIST_CONFIGS[name], 10)}
    out['ragged_conv_ships'] = all(c['ragged_faster_every_round'] for c in out['configs'].values())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
