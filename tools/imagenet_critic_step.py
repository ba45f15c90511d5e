"""The G+D step of the ImageNet configuration (train.IMAGENET_CONFIGS 'imagenet_cond_sa') on one GPU with the critic marked slim_blocks
 and unmarked.  Writes profiles/imagenet_critic_step.json; prints only what it measured.

Two legs, one captured hipGraph per leg, batch 64 (32 if 64 does not fit: the file says which), the trainer's defaults (training_ratio 5,
generator_batch_multiple 2); the generator keeps its slim_conv mark in both:
    marked    train.slim_blocks_config(cfg): every convolution layer of the critic marked -- block 0 (3 -> 64 at 128 x 128) runs as
              conv.critic_first_block, block 1 (64 -> 128 at 64 x 64) as conv.critic_block, the image layers' data gradient on
              wc_conv_narrow_out_f32
    unmarked  train.slim_blocks_config(cfg, on=False): those two blocks as separate torch / MIOpen nodes -- the parent commit's route
The two graphs are replayed ALTERNATING in one process (A B A B ..., HIP events around `--steps` replays each), so clock and temperature
drift hit both legs alike; the figure of a leg is the median over the rounds, its spread max - min.  `marked_faster_every_round` is the rule
train.IMAGENET_SLIM_BLOCKS_SHIPS follows.  Peak memory is taken per leg (the marked route keeps h's planes).
Beside the step, at a pass of 128 images, marked against unmarked, the device time of the call's kernels (torch's profiler, summed):
block 0 forward + backward with and without the image's gradient, block 1 forward + backward; and the narrow-output kernel against
threshold_backward + torch's input gradient at (128, 128, 128, 64 -> 3, k = 3) and against torch's input gradient at
(128, 64, 64, 64 -> 3, k = 1).

    python tools/imagenet_critic_step.py [--rounds 7] [--steps 2] [--out profiles/imagenet_critic_step.json]
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
    from wc_gan_amd.train import build_trainer, slim_blocks_config, slim_config
    torch.manual_seed(0)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tr = build_trainer(slim_blocks_config(slim_config(cfg), on=on), "cuda", batch_size=batch)
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
        sys.exit("imagenet_critic_step.py: a leg's losses are not finite")
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    # (the graph reads the tensors it was captured with: they must outlive the replays)
    return replay, (tr, reals, labels), round(peak, 2)


def _blocks(trainers, n, calls):
    """forward + backward device time of the critic's blocks 0 and 1 at a pass of n images, per leg"""
    out = []

    def part(name, index, x, with_dx):
        row = {'part': name, 'input': list(x.shape), 'image_gradient': with_dx}
        for key, tr in trainers.items():
            blk = tr.D.blocks[index]
            params = list(blk.parameters()) + ([x] if with_dx else [])
            xin = x if with_dx else x.detach()
            gy = torch.randn_like(blk(xin, None))
            fn = lambda: torch.autograd.grad(blk(xin, None), params, gy)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            row[key + '_us'] = round(_device_us(fn, calls), 1)
        row['marked_over_unmarked'] = round(row['marked_us'] / row['unmarked_us'], 3)
        out.append(row)
        _say("block", row)

    torch.manual_seed(5)
    img = torch.randn(n, 128, 128, 3, device='cuda').requires_grad_(True)
    part("critic block 0 (3 -> 64 at 128 x 128, DOWN), critic update", 0, img, False)
    part("critic block 0 (3 -> 64 at 128 x 128, DOWN), generator update", 0, img, True)
    h = torch.randn(n, 64, 64, 64, device='cuda').requires_grad_(True)
    part("critic block 1 (64 -> 128 at 64 x 64, DOWN)", 1, h, True)
    return out


def _kernel(n, calls):
    """the narrow-output kernel against the launches it replaces"""
    from wc_gan_amd import conv as C
    out = []
    for H, k, masked in ((128, 3, True), (128, 3, False), (64, 1, False)):
        torch.manual_seed(H + k)
        g, h = torch.randn(n, H, H, 64, device='cuda'), torch.randn(n, H, H, 64, device='cuda')
        w = (torch.randn(64, 3, k, k, device='cuda') * 0.1).contiguous(memory_format=torch.channels_last)
        x = torch.zeros(n, H, H, 3, device='cuda').permute(0, 3, 1, 2)

        def hip():
            return C.narrow_out_conv(g, w, mask=h if masked else None)

        def torch_route():
            gm = torch.ops.aten.threshold_backward(g, h, 0) if masked else g
            return torch.ops.aten.convolution_backward(gm.permute(0, 3, 1, 2), x, w, None, [1, 1], [k // 2, k // 2], [1, 1], False, [0, 0], 1,
                                                       [True, False, False])[0]
        for fn in (hip, torch_route):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        row = {'shape': [n, H, H, 64, 3, k], 'masked': masked, 'hip_us': round(_device_us(hip, calls), 1),
               'torch_us': round(_device_us(torch_route, calls), 1)}
        row['hip_over_torch'] = round(row['hip_us'] / row['torch_us'], 3)
        row['hip_GB_per_s'] = round((2 if masked else 1) * g.numel() * 4 / row['hip_us'] / 1e3, 1)
        out.append(row)
        _say("kernel", row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=2, help="replays per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imagenet_critic_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("imagenet_critic_step.py needs the GPU")
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
        sys.exit("imagenet_critic_step.py: neither batch 64 nor 32 fits")
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
                   'the generator marked slim_conv in both legs',
           'marked': on, 'unmarked': off, 'marked_over_unmarked': round(on['median'] / off['median'], 4),
           'marked_over_unmarked_per_round': per_round, 'marked_faster_every_round': all(r < 1.0 for r in per_round),
           'peak_memory_GiB': peaks}
    out['imagenet_slim_blocks_ships'] = out['marked_faster_every_round']
    out['blocks_fwd_bwd_device_us'] = _blocks({k: keep[k][0] for k in keep}, batch * 2, 3)
    out['narrow_out_kernel_device_us'] = _kernel(batch * 2, 5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
