"""The G+D step of the ImageNet configuration (train.IMAGENET_CONFIGS 'imagenet_cond_sa') on one GPU with the generator's last layer,
Generator.Final (32 -> 3 at 128 x 128), marked narrow_last and unmarked.  Writes profiles/imagenet_last_step.json;
prints only what it measured.

Two legs, one captured hipGraph per leg, batch 64 (32 if 64 does not fit: the file says which), the trainer's defaults (training_ratio 5,
generator_batch_multiple 2); the generator keeps its slim_conv mark and the critic its slim_blocks mark in both:
    marked    train.narrow_last_config(cfg): the layer's forward on wc_conv_narrow_out_bias_f32, its weight gradient on
              wc_conv_wrw_narrow32_f32, its data gradient on wc_conv_fwd_narrow32_f32 (conv._NarrowLastConv)
    unmarked  train.narrow_last_config(cfg, on=False): the fp32 GEMM + fold and aten.convolution_backward -- the parent commit's route
The two graphs are replayed ALTERNATING in one process (A B A B ..., HIP events around `--steps` replays each), so clock and temperature
drift hit both legs alike; the figure of a leg is the median over the rounds, its spread max - min.  `marked_faster_every_round` is the rule
train.IMAGENET_NARROW_LAST_SHIPS follows.  Peak memory is taken per leg.
Beside the step, the layer alone at (128, 128 x 128, 32 -> 3), marked against unmarked, as device time of the call's kernels (torch's
profiler, summed): the forward under no_grad, forward + backward with the input's gradient, and each of the three launches by itself with
the bytes it has to move and the rate that makes.

    python tools/imagenet_last_step.py [--rounds 7] [--steps 2] [--out profiles/imagenet_last_step.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from imagenet_step import NAME, _device_us, _say, _summary, _timed  # noqa: E402


def _leg(cfg, on, batch):
    from wc_gan_amd.train import build_trainer, narrow_last_config, slim_blocks_config, slim_config
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tr = build_trainer(narrow_last_config(slim_blocks_config(slim_config(cfg)), on=on), "cuda", batch_size=batch)
    if tr.G.final_conv.narrow_last != on:
        sys.exit("imagenet_last_step.py: the mark did not reach Generator.Final")
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
        sys.exit("imagenet_last_step.py: a leg's losses are not finite")
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    # (the graph reads the tensors it was captured with: they must outlive the replays)
    return replay, (tr, reals, labels), round(peak, 2)


def _layer(n, calls):
    """the layer alone at a generator pass of n images: marked against unmarked, then the marked route's launches one by one"""
    from wc_gan_amd import conv as C
    from wc_gan_amd.generator import Conv2D
    torch.manual_seed(4)
    H = W = 128
    x = torch.randn(n, H, W, 32, device='cuda').requires_grad_(True)
    gy = torch.randn(n, H, W, 3, device='cuda')
    layers = {}
    for key, on in (('marked', True), ('unmarked', False)):
        torch.manual_seed(3)
        layers[key] = Conv2D(32, 3, (3, 3), narrow_last=on).cuda().train()
        with torch.no_grad():
            layers[key].conv.bias.normal_(0, 0.1)
    if not layers['marked']._narrow_last_route(x) or layers['unmarked']._narrow_last_route(x):
        sys.exit("imagenet_last_step.py: the layer's routes are not the two it compares")
    rows = []

    def compare(what, make):
        row = {'part': what, 'shape': [n, H, W, 32, 3, 3]}
        for key, layer in layers.items():
            fn = make(layer)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            row[key + '_us'] = round(_device_us(fn, calls), 1)
        row['marked_over_unmarked'] = round(row['marked_us'] / row['unmarked_us'], 3)
        rows.append(row)
        _say("layer", row)

    def forward(layer):
        def fn():
            with torch.no_grad():
                return layer(x)
        return fn
    compare('forward (no_grad)', forward)
    compare('forward + backward (dx, dW, db)',
            lambda layer: lambda: torch.autograd.grad(layer(x), (x, layer.conv.weight, layer.conv.bias), gy))
    compare('forward + backward (dW, db: the input needs no gradient)',
            lambda layer: lambda: torch.autograd.grad(layer(x.detach()), (layer.conv.weight, layer.conv.bias), gy))
    # the three launches, with the bytes each has to move (the wide tensor once; the narrow ones beside it)
    w, b = layers['marked'].conv.weight.detach(), layers['marked'].conv.bias.detach()
    xd = x.detach()
    wide, narrow = xd.numel() * 4, gy.numel() * 4
    launches = []
    for what, fn, nbytes in (('forward: wc_conv_narrow_out_bias_f32', lambda: C.narrow_out_conv(xd, w, forward=True, bias=b), wide + narrow),
                             ('dW: wc_conv_wrw_narrow32_f32 (kernel + reduce)', lambda: C.narrow_out_weight_gradient(xd, gy, w, wide32=True),
                              wide + narrow),
                             ('dx: wc_conv_fwd_narrow32_f32', lambda: C.narrow_forward(gy, w, None, mirrored=True, wide32=True), wide + narrow)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        us = _device_us(fn, calls)
        row = {'launch': what, 'us': round(us, 1), 'bytes': nbytes, 'GB_per_s': round(nbytes / us / 1e3, 1),
               'of_8_TB_per_s_peak': round(nbytes / us / 1e3 / 8000.0, 3)}
        launches.append(row)
        _say("launch", row)
    return rows, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2, help="replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imagenet_last_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("imagenet_last_step.py needs the GPU")
    from wc_gan_amd.train import IMAGENET_CONFIGS
    cfg = IMAGENET_CONFIGS[NAME]
    legs, keep, peaks, batch, note = {}, {}, {}, 64, None
    for attempt in (64, 32):
        try:
            legs, keep, peaks = {}, {}, {}
            for route, on in (('marked', True), ('unmarked', False)):
                _say("capturing", route, "at batch", attempt)
                legs[route], keep[route], peaks[route] = _leg(cfg, on, attempt)
            batch = attempt
            break
        except torch.OutOfMemoryError as e:
            note = f"batch {attempt} does not fit: {str(e).splitlines()[0]}"
            _say(note)
            legs, keep, peaks = {}, {}, {}
            torch.cuda.empty_cache()
    if not legs:
        sys.exit("imagenet_last_step.py: neither batch 64 nor 32 fits")
    ms = {k: [] for k in legs}
    for r in range(args.rounds):
        for k, replay in legs.items():
            ms[k].append(_timed(replay, args.steps))
        _say("round", r, {k: round(v[-1], 2) for k, v in ms.items()})
    on, off = _summary(ms['marked']), _summary(ms['unmarked'])
    per_round = [round(a / b, 4) for a, b in zip(ms['marked'], ms['unmarked'])]
    out = {'device': torch.cuda.get_device_name(0), 'config': NAME, 'rounds': args.rounds, 'steps_per_leg_and_round': args.steps, 'batch': batch,
           'batch_note': note,
           'what': 'captured G+D step (training_ratio 5, generator_batch_multiple 2), ms per step, the two graphs replayed alternately; '
                   'the generator marked slim_conv and the critic slim_blocks in both legs',
           'marked': on, 'unmarked': off, 'marked_over_unmarked': round(on['median'] / off['median'], 4),
           'marked_over_unmarked_per_round': per_round, 'marked_faster_every_round': all(r < 1.0 for r in per_round),
           'peak_memory_GiB': peaks}
    out['imagenet_narrow_last_ships'] = out['marked_faster_every_round']
    legs.clear(); keep.clear()
    torch.cuda.empty_cache()
    out['layer_device_us'], out['launches_device_us'] = _layer(batch * 2, 5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
