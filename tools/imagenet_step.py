"""The G+D step of the ImageNet configuration (train.IMAGENET_CONFIGS 'imagenet_cond_sa') on one GPU, with the
generator's 64- and 32-channel block convolutions on the block kernels (slim_conv) and off.  Writes profiles/imagenet_step.json; prints only
what it measured.

Two legs, one captured hipGraph per leg, batch 64 (32 if 64 does not fit: the file says which), the trainer's defaults (training_ratio 5,
generator_batch_multiple 2):
    slim    train.slim_config(cfg): every convolution layer of the generator marked slim_conv -- blocks 3 (128 -> 64) and 4 (64 -> 32) run
            csrc/wc_conv.hip's kernels: the 64-wide tiles they always had, the 32-output and 32 x 32 tiles
    off     train.slim_config(cfg, on=False): the same networks unmarked -- those six layers on torch's / MIOpen's convolutions
The two graphs are replayed ALTERNATING in one process (A B A B ..., HIP events around `--steps` replays each), so clock and temperature
drift hit both legs alike; the figure of a leg is the median over the rounds, its spread max - min.  `slim_faster_every_round` is the rule
train.IMAGENET_SLIM_SHIPS follows.
Layer leg: blocks 3 and 4's conv1, conv2 and shortcut as generator.Conv2D layers, forward + backward (dx, dW, db) at the generator update's
grid (N = 64 x generator_batch_multiple), marked against unmarked: the device time of the call's kernels (torch's profiler, summed).
Left on torch / MIOpen on both legs: the critic's 64-wide first block, its 64 -> 128 block and the generator's 32 -> 3 last layer -- the
device time of one forward + backward and of one forward of each at a pass of 2 x batch images, weighted by the step's passes (the critic's
blocks: five critic updates on real + generated images and one generator update on batch x generator_batch_multiple, six forward + backward
passes; the last layer: that one generator update, and the forward-only generation of 5 x batch images = 2.5 such passes), as a share of the
marked leg's step.  (An estimate from the layers run alone: the graph's own kernels overlap on two streams.)

    python tools/imagenet_step.py [--rounds 7] [--steps 2] [--out profiles/imagenet_step.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

NAME = 'imagenet_cond_sa'


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _summary(v):
    return {'ms': [round(t, 3) for t in v], 'median': round(statistics.median(v), 3), 'spread': round(max(v) - min(v), 3)}


def _leg(cfg, on, batch):
    from wc_gan_amd.train import build_trainer, slim_config
    torch.manual_seed(0)
    tr = build_trainer(slim_config(cfg, on=on), "cuda", batch_size=batch)
    g = torch.Generator(device="cpu"); g.manual_seed(1)
    H, W, C = cfg['image_shape']
    K = cfg['generator']['number_of_classes']
    reals = [(torch.rand(batch, H, W, C, generator=g) * 2 - 1).cuda() for _ in range(tr.training_ratio)]
    labels = [torch.randint(0, K, (batch,), generator=g, dtype=torch.int32).cuda() for _ in range(tr.training_ratio)]
    replay = tr.capture(reals, labels)
    for _ in range(2):
        losses = replay()
    torch.cuda.synchronize()
    if not all(bool(torch.isfinite(l)) for l in losses):
        sys.exit("imagenet_step.py: a leg's losses are not finite")
    # (the graph reads the tensors it was captured with: they must outlive the replays)
    return replay, (tr, reals, labels)


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


def _layers(n):
    """(name, call, N, H, W, Cin, Cout, k) of the six marked-width convolutions at a generator pass of n images"""
    return [('Generator.3.conv1', 'upsampled', n, 32, 32, 128, 64, 3), ('Generator.3.conv2', 'same', n, 64, 64, 64, 64, 3),
            ('Generator.3.shortcut', 'same', n, 32, 32, 128, 64, 1),
            ('Generator.4.conv1', 'upsampled', n, 64, 64, 64, 32, 3), ('Generator.4.conv2', 'same', n, 128, 128, 32, 32, 3),
            ('Generator.4.shortcut', 'same', n, 64, 64, 64, 32, 1)]


def _layer_leg(n, calls):
    from wc_gan_amd.generator import Conv2D
    out = []
    for name, call, N, H, W, ci, co, k in _layers(n):
        torch.manual_seed(ci + co + H)
        x = torch.randn(N, H, W, ci, device='cuda').requires_grad_(True)
        us = {}
        for key, on in (('slim', True), ('off', False)):
            torch.manual_seed(3)
            layer = Conv2D(ci, co, (k, k), slim_conv=on).cuda().train()
            params = (x, layer.conv.weight, layer.conv.bias)
            run = (lambda l=layer: l.forward_upsampled(x)) if call == 'upsampled' else (lambda l=layer: l(x))
            gy = torch.randn_like(run())
            fn = lambda: torch.autograd.grad(run(), params, gy)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            us[key] = _device_us(fn, calls)
        out.append({'layer': name, 'shape': [call, N, H, W, ci, co, k], 'slim_us': round(us['slim'], 1), 'off_us': round(us['off'], 1),
                    'slim_over_off': round(us['slim'] / us['off'], 3)})
        _say("layer", out[-1])
    return out


def _left_on_torch(tr, batch, step_ms, calls):
    """forward + backward device time of the parts both legs leave on torch / MIOpen, at a pass of 2 x batch images"""
    n = 2 * batch
    D, G = tr.D, tr.G
    parts = []

    def part(name, mod, x, with_dx, call, both, fwd_only):
        params = [p for p in mod.parameters()] + ([x] if with_dx else [])
        y = call(x)
        gy = torch.randn_like(y)
        fn = lambda: torch.autograd.grad(call(x), params, gy)

        def fwd():
            with torch.no_grad():
                call(x)
        for _ in range(2):
            fn()
            fwd()
        torch.cuda.synchronize()
        us, us_f = _device_us(fn, calls), _device_us(fwd, calls)
        parts.append({'part': name, 'input': list(x.shape), 'fwd_bwd_device_us': round(us, 1), 'fwd_device_us': round(us_f, 1),
                      'fwd_bwd_passes_per_step': both, 'fwd_passes_per_step': fwd_only,
                      'share_of_slim_step': round((both * us + fwd_only * us_f) / 1000.0 / step_ms, 4)})
        _say("left on torch", parts[-1])

    torch.manual_seed(5)
    img = torch.randn(n, 128, 128, 3, device='cuda')
    part("critic block 0 (3 -> 64 at 128 x 128, DOWN)", D.blocks[0], img, False, lambda t: D.blocks[0](t, None), 6, 0)
    h = torch.randn(n, 64, 64, 64, device='cuda').requires_grad_(True)
    part("critic block 1 (64 -> 128 at 64 x 64, DOWN)", D.blocks[1], h, True, lambda t: D.blocks[1](t, None), 6, 0)
    f = torch.randn(n, 128, 128, 32, device='cuda').requires_grad_(True)
    part("generator last layer (32 -> 3 at 128 x 128)", G.final_conv, f, True, lambda t: G.final_conv(t), 1, 2.5)
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2, help="replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imagenet_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("imagenet_step.py needs the GPU")
    from wc_gan_amd.train import IMAGENET_CONFIGS
    cfg = IMAGENET_CONFIGS[NAME]
    legs, keep, batch, note = {}, [], 64, None
    for attempt in (64, 32):
        try:
            legs, keep = {}, []
            for route, on in (('slim', True), ('off', False)):
                _say("capturing", route, "at batch", attempt)
                legs[route], held = _leg(cfg, on, attempt)
                keep.append(held)
            batch = attempt
            break
        except torch.OutOfMemoryError as e:
            note = f"batch {attempt} does not fit: {str(e).splitlines()[0]}"
            _say(note)
            legs, keep = {}, []
            torch.cuda.empty_cache()
    if not legs:
        sys.exit("imagenet_step.py: neither batch 64 nor 32 fits")
    ms = {k: [] for k in legs}
    for r in range(args.rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, args.steps))
        _say("round", r, {k: round(v[-1], 2) for k, v in ms.items()})
    on, off = _summary(ms['slim']), _summary(ms['off'])
    per_round = [round(a / b, 4) for a, b in zip(ms['slim'], ms['off'])]
    out = {'device': torch.cuda.get_device_name(0), 'config': NAME, 'rounds': args.rounds, 'steps_per_leg_and_round': args.steps, 'batch': batch,
           'batch_note': note,
           'what': 'captured G+D step (training_ratio 5, generator_batch_multiple 2), ms per step, the two graphs replayed alternately',
           'slim': on, 'off': off, 'slim_over_off': round(on['median'] / off['median'], 4), 'slim_over_off_per_round': per_round,
           'slim_faster_every_round': all(r < 1.0 for r in per_round),
           'peak_memory_GiB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    out['imagenet_slim_ships'] = out['slim_faster_every_round']
    out['layers_fwd_bwd_device_us'] = _layer_leg(batch * 2, 5)
    out['left_on_torch'] = _left_on_torch(keep[0][0], batch, on['median'], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
