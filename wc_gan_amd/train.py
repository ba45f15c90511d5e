"""Minimal G+D training step around the WC generator: hinge loss, Adam(beta1=0, beta2=0.9)
(run.py:58-59,255-256), `training_ratio` critic updates per generator update (run.py:101), the
generator update at batch_size x generator_batch_multiple (run.py:293-294).

Data parallelism is new design (the reference is single-process): one process per
GPU, per-replica WC statistics by default, and ONE flat gradient bucket per network that is
all-reduced (mean) over RCCL after each backward.  The bucket is zero-copy: every parameter's .grad
is a view into it, so there is no pack/unpack around the collective.  xGMI is point-to-point
(7 links per GPU) and these messages are small (G ~19 MB, D ~4 MB fp32), i.e. latency-bound; a single
large all-reduce per network is the shape RCCL handles best there.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _state


# development: run the gradient collectives even in a one-rank process group (exercises RCCL between graph segments on one GPU)
_FORCE_COLLECTIVES = __import__('os').environ.get('WC_FORCE_COLLECTIVES', '0') == '1'


class FlatGradBucket:
    """All gradients of one network in one contiguous buffer; .grad tensors are views into it.
    `flat=False` (what the trainer picks for a single process): no buffer -- zero() just drops the gradients, so autograd
    hands each parameter its gradient tensor instead of adding it into a view (one small kernel per parameter and
    backward pass saved; nothing is all-reduced anyway)."""

    def __init__(self, params, process_group=None, flat=True):
        self.params = [p for p in params if p.requires_grad]
        self.group = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.flat = None
        if not flat:
            return
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        if len({p.dtype for p in self.params}) != 1:
            raise ValueError("FlatGradBucket: the parameters of one network share one dtype")
        self.flat = torch.zeros(n, dtype=self.params[0].dtype, device=dev)      # (float32 everywhere but in float64 tests)
        off = 0
        for p in self.params:
            seg = self.flat[off:off + p.numel()]
            if p.dim() == 4 and not p.is_contiguous() and p.is_contiguous(memory_format=torch.channels_last):
                o, i, kh, kw = p.shape                      # same strides as the channels_last weight
                p.grad = seg.view(o, kh, kw, i).permute(0, 3, 1, 2)
            else:
                p.grad = seg.view_as(p)
            off += p.numel()

    def zero(self):
        if self.flat is None:
            for p in self.params:
                p.grad = None
        else:
            self.flat.zero_()

    def allreduce_mean(self):
        if (self.world > 1 or _FORCE_COLLECTIVES) and self.flat is not None:
            tm = self.timer
            if tm is not None:
                tm.begin(self.flat)
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
            if tm is not None:
                tm.end(self.flat)
            self.flat.mul_(1.0 / self.world)

    timer = None          # an AllreduceTimer while bench.py measures the collectives' share of a step (diagnostics only)


class AllreduceTimer:
    """Time spent in the gradient all-reduces, for the N > 1 diagnostics of bench.py: HIP events on the launching stream
    around each collective (the NCCL/RCCL call makes that stream wait for its result), wall clock on the CPU (gloo)."""

    def __init__(self):
        self.pairs, self.cpu_s, self.calls = [], 0.0, 0

    def begin(self, t):
        self.calls += 1
        if t.is_cuda:
            e0 = torch.cuda.Event(enable_timing=True); e0.record()
            self._e0 = e0
        else:
            import time
            self._t0 = time.perf_counter()

    def end(self, t):
        if t.is_cuda:
            e1 = torch.cuda.Event(enable_timing=True); e1.record()
            self.pairs.append((self._e0, e1))
        else:
            import time
            self.cpu_s += time.perf_counter() - self._t0

    def total_ms(self):
        if self.pairs:
            torch.cuda.synchronize()
            return sum(a.elapsed_time(b) for a, b in self.pairs)
        return self.cpu_s * 1e3


def broadcast_state(module, src=0, group=None):
    """Rank 0's parameters and buffers (incl. moving_mean / moving_cov) to every replica at start-up."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    for t in list(module.parameters()) + list(module.buffers()):
        dist.broadcast(t.data, src=src, group=group)


def _bump_versions(params):
    """torch's fused Adam updates the weights without moving their version counters; everything that caches per
    `tensor._version` (the eval-mode WC plan keys on the coloring weights) must still see the update."""
    inc = getattr(torch.autograd.graph, 'increment_version', None)
    if inc is not None:
        for p in params:
            inc(p)


class GanTrainer:
    def __init__(self, generator, discriminator, batch_size=64, generator_batch_multiple=2, training_ratio=5,
                 lr=2e-4, beta1=0.0, beta2=0.9, noise_dim=128, number_of_classes=10, conditional=False,
                 process_group=None, seed=1234, flat_buckets=None, objective='hinge', gradient_penalty_weight=0.0,
                 lr_decay_schedule=None, number_of_epochs=None, schedule_iters=None, generator_lr=None, discriminator_lr=None,
                 optimizer=None, gan_type=None, class_loss_weight_discriminator=1.0, class_loss_weight_generator=1.0):
        if gan_type not in (None, 'AC_GAN'):
            raise ValueError(f"gan_type {gan_type!r}: None or 'AC_GAN' (a PROJECTIVE recipe is `conditional=True` with a PROJECTIVE critic)")
        # 'AC_GAN' (scripts/cifar10_resnet_wgan_cond*.sh, run.py --gan_type AC_GAN): the critic's class head is trained with a cross entropy
        # beside the adversarial loss, and the generator is asked for samples the head assigns to the classes it drew.  gan/ac_gan.py is not
        # in the reference tree, so THESE CONVENTIONS ARE OURS AND UNPINNED: the critic's class loss is
        # w_d (mean ce(real) + mean ce(generated)) -- both halves --, the generator's w_g mean ce(generated), both weights 1.  The critic
        # takes no label input (`conditional` stays False) and the gradient penalty stays on the adversarial head.
        self.gan_type = gan_type
        self.w_cls_d, self.w_cls_g = float(class_loss_weight_discriminator), float(class_loss_weight_generator)
        self.last_class_losses = [None, None, None]     # device scalars: mean ce of the real half, of the generated half, of the generator's batch
        if gan_type == 'AC_GAN':
            if getattr(discriminator, 'type', None) != 'AC_GAN':
                raise ValueError("gan_type='AC_GAN' needs a critic with the class head (make_discriminator(type='AC_GAN'))")
            if conditional:
                raise ValueError("gan_type='AC_GAN': the critic takes no label input (conditional=False)")
        if objective not in ('hinge', 'wgan'):
            raise ValueError(f"objective {objective!r}: 'hinge' or 'wgan' (run.py --*_adversarial_objective)")
        # 'wgan' (scripts/cifar10_resnet_wgan_*.sh): the critic loss E D(fake) - E D(real), plus gradient_penalty_weight x the gradient
        # penalty at interpolates of the two batches (penalty.py: closed form, no second-order autograd)
        self.objective, self.gp_weight = objective, float(gradient_penalty_weight)
        self.last_penalty = self.last_grad_norms = None
        self.G, self.D = generator, discriminator
        self.batch_size, self.gbm, self.training_ratio = batch_size, generator_batch_multiple, training_ratio
        self.noise_dim, self.K, self.conditional = noise_dim, number_of_classes, conditional
        self.dev = next(generator.parameters()).device
        world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        flat = (world > 1) if flat_buckets is None else bool(flat_buckets)     # (True at world 1: the DP layout, for tests)
        self.g_bucket = FlatGradBucket(self.G.parameters(), process_group, flat=flat)
        self.d_bucket = FlatGradBucket(self.D.parameters(), process_group, flat=flat)
        # capturable: the step counters live on the device, so a whole G+D step can be recorded into one hipGraph
        cap = self.dev.type == 'cuda'
        # fused: one multi-tensor kernel per update instead of ~10 small launches per parameter (step counters on the
        # device either way)
        kw = dict(fused=True) if cap else dict()
        if optimizer not in (None, 'hip'):
            raise ValueError(f"optimizer {optimizer!r}: None (torch.optim.Adam) or 'hip' (optim.ScheduledAdam)")
        g_lr = lr if generator_lr is None else generator_lr                # run.py:252-253 --generator_lr / --discriminator_lr
        d_lr = lr if discriminator_lr is None else discriminator_lr
        if optimizer == 'hip' or lr_decay_schedule is not None:
            # run.py:100-101: the generator's schedule runs over 1000 x number_of_epochs of ITS updates, the critic's over training_ratio
            # times as many of its own (optim.py; each optimiser counts its updates on the device, so graph replays advance the rate)
            from .optim import ScheduledAdam
            total = schedule_iters if schedule_iters is not None else (None if number_of_epochs is None else 1000 * number_of_epochs)
            if lr_decay_schedule is not None and total is None:
                raise ValueError("lr_decay_schedule needs number_of_epochs (or schedule_iters, the generator's total directly)")
            d_total = None if total is None else total * training_ratio
            self.opt_g = ScheduledAdam(self.g_bucket.params, g_lr, (beta1, beta2), schedule=lr_decay_schedule, total_iters=total, ratio=1)
            self.opt_d = ScheduledAdam(self.d_bucket.params, d_lr, (beta1, beta2), schedule=lr_decay_schedule, total_iters=d_total,
                                       ratio=training_ratio)
        else:
            self.opt_g = torch.optim.Adam(self.g_bucket.params, lr=g_lr, betas=(beta1, beta2), capturable=cap, **kw)
            self.opt_d = torch.optim.Adam(self.d_bucket.params, lr=d_lr, betas=(beta1, beta2), capturable=cap, **kw)
        if cap:
            # the default device generator (its Philox offset is graph-safe); every replica draws its own noise
            rank = dist.get_rank(process_group) if (dist.is_available() and dist.is_initialized()) else 0
            torch.cuda.manual_seed(seed + rank)
        self._graph = None
        self._side = None
        self.overlap_g_forward = True
        self._boundary = None            # set while capture_segments() records: called where a gradient all-reduce goes
        self._side_pending = False

    def _sync_grads(self, bucket):
        """The gradient all-reduce of one network (a no-op for a single process) -- or, while capture_segments() records,
        the end of one graph segment and the start of the next."""
        if self._boundary is not None:
            self._boundary(bucket)
        else:
            bucket.allreduce_mean()

    def _noise(self, n):
        z = torch.randn(n, self.noise_dim, device=self.dev)
        cls = torch.randint(0, self.K, (n, 1), device=self.dev, dtype=torch.int32)
        return z, cls

    def _d(self, x, cls):
        out = self.D(x, cls if self.conditional else None)
        return out[0] if isinstance(out, tuple) else out

    def _adv_loss_d(self, out, n):
        if self.objective == 'wgan':
            return out[n:].mean() - out[:n].mean()
        return F.relu(1.0 - out[:n]).mean() + F.relu(1.0 + out[n:]).mean()

    def generate(self, rounds):
        """The `rounds` generated batches of one G+D step in ONE generator pass.  The generator's weights are fixed
        while the critic trains, so its `rounds` forward passes are independent; they run as a single batch of
        rounds x batch_size whose WC layers keep per-round statistics (layers.statistic_groups) -- the same numbers
        as separate passes, with the covariance / Cholesky problems of the rounds solved side by side."""
        from .layers import statistic_groups, supports_statistic_groups
        z, cls = self._noise(self.batch_size * rounds)
        if rounds > 1 and not supports_statistic_groups(self.G):
            # a norm layer without the grouped form (renorm, padded widths, plain batch norm): `rounds` real passes
            with torch.no_grad():
                fakes = [self.G(zz, cc) for zz, cc in zip(z.split(self.batch_size), cls.split(self.batch_size))]
            return fakes, cls.split(self.batch_size)
        with torch.no_grad(), statistic_groups(rounds):
            fake = self.G(z, cls)                      # train-mode WC forward (batch statistics), no graph
        return fake.split(self.batch_size), cls.split(self.batch_size)

    def d_step(self, real, real_cls=None, fake=None, cls=None, eps=None):
        """One critic update.  eps: the (N,) interpolation weights of the gradient penalty (drawn on the device when None)."""
        if fake is None:
            (fake,), (cls,) = self.generate(1)
        self.d_bucket.zero()
        # real and generated images go through the critic as ONE batch of 128: the critic has no batch-dependent
        # layer (discriminator_norm is 'n' in every recipe), so this equals two applications with shared weights,
        # with one spectral-norm power iteration per update and convolutions at twice the batch
        n = real.shape[0]
        if self.conditional:
            if real_cls is None:      # run.py:317 get_dataset(supervised=True): real images come with their labels
                raise ValueError("conditional critic: d_step needs the labels of the real batch (real_cls)")
            both_cls = torch.cat([real_cls.reshape(-1, 1).to(cls.dtype), cls], dim=0)
        else:
            both_cls = None
        if self.gan_type == 'AC_GAN':
            if real_cls is None:
                raise ValueError("gan_type='AC_GAN': d_step needs the labels of the real batch (real_cls)")
            labels = torch.cat([real_cls.reshape(-1).to(cls.dtype), cls.reshape(-1)], dim=0)
            out, _logits, ce = self.D(torch.cat([real, fake], dim=0), None, labels=labels)
            ce_real, ce_fake = ce[:n].mean(), ce[n:].mean()
            self.last_class_losses[0], self.last_class_losses[1] = ce_real.detach(), ce_fake.detach()
            loss = self._adv_loss_d(out, n) + self.w_cls_d * (ce_real + ce_fake)
        else:
            loss = self._adv_loss_d(self._d(torch.cat([real, fake], dim=0), both_cls), n)
        loss.backward()
        loss = loss.detach()
        if self.gp_weight != 0.0:
            # into the same .grad tensors (the flat bucket's views), ahead of the all-reduce
            from .penalty import gradient_penalty, interpolate
            x_hat = interpolate(real, fake, eps)
            hat_cls = both_cls[:n] if self.conditional else None        # a projection critic sees the interpolate under the real batch's labels
            self.last_penalty, self.last_grad_norms = gradient_penalty(self.D, x_hat, hat_cls, self.gp_weight)
            loss = loss + self.last_penalty
        self._sync_grads(self.d_bucket)
        self.opt_d.step()
        _bump_versions(self.d_bucket.params)
        return loss

    def g_step(self, generated=None):
        self.g_bucket.zero()
        if generated is None:
            z, cls = self._noise(self.batch_size * self.gbm)
            fake = self.G(z, cls)
        else:
            fake, cls = generated
        for p in self.d_bucket.params:
            p.requires_grad_(False)
        if self.gan_type == 'AC_GAN':
            out, _logits, ce = self.D(fake, None, labels=cls.reshape(-1))
            ce_g = ce.mean()
            self.last_class_losses[2] = ce_g.detach()
            loss = -out.mean() + self.w_cls_g * ce_g
        else:
            loss = -self._d(fake, cls).mean()
        loss.backward()
        for p in self.d_bucket.params:
            p.requires_grad_(True)
        self._sync_grads(self.g_bucket)
        self.opt_g.step()
        _bump_versions(self.g_bucket.params)
        return loss.detach()

    def step(self, real_batches, real_labels=None):
        """One G+D step: training_ratio critic updates, then one generator update.  `real_labels`: one int (64,) or
        (64, 1) tensor per real batch -- required by the conditional recipes (the projection critic must see true
        (image, label) pairs; run.py:317) and by gan_type='AC_GAN' (the class head learns from them)."""
        if self.conditional and real_labels is None:
            raise ValueError("conditional recipe: step() needs real_labels (one label tensor per real batch)")
        if self.gan_type == 'AC_GAN' and real_labels is None:
            raise ValueError("gan_type='AC_GAN': step() needs real_labels (one label tensor per real batch): the class head learns from them")
        fakes, clss = self.generate(self.training_ratio)
        generated = None
        if self.overlap_g_forward and self.dev.type == 'cuda':
            # The generator update's forward pass needs the generator's weights only, and those do not move while the
            # critic trains: it runs on a second stream next to the critic updates and fills the chip while their
            # narrow kernels (Cholesky, small GEMMs, spectral norm) run -- and the other way round.  Same numbers.
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream()
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                z, cls = self._noise(self.batch_size * self.gbm)
                generated = (self.G(z, cls), cls)
            self._side_pending = True
        for r in range(self.training_ratio):
            rl = real_labels[r % len(real_labels)] if real_labels is not None else None
            d_loss = self.d_step(real_batches[r % len(real_batches)], real_cls=rl, fake=fakes[r], cls=clss[r])
        if generated is not None:
            if self._side_pending:                   # (a graph segment that ended in between has joined it already)
                torch.cuda.current_stream().wait_stream(self._side)
                self._side_pending = False
            generated[0].record_stream(torch.cuda.current_stream())
            generated[1].record_stream(torch.cuda.current_stream())
        g_loss = self.g_step(generated)
        return d_loss, g_loss

    def trace_boundaries(self, real_batches, real_labels=None):
        """One eager step that also records where the gradient all-reduces sit: ['d', ..., 'd', 'g'] -- the cut points of
        capture_segments().  Every rank must report the same list (tests/test_dp_gloo.py, bench.py --dry-run)."""
        order = []

        def boundary(bucket):
            order.append('d' if bucket is self.d_bucket else 'g')
            bucket.allreduce_mean()

        self._boundary = boundary
        try:
            losses = self.step(real_batches, real_labels)
        finally:
            self._boundary = None
        return order, losses

    def capture(self, real_batches, real_labels=None, warmup=3):
        """Record one whole G+D step (~1700 kernel launches) into ONE hipGraph -- single process only: capturing an RCCL
        all-reduce aborts the process (tried with a one-rank group), so with gradient collectives use capture_segments().

        The C-ABI stages never synchronise or allocate and the gate of the fast path is a device flag, so the
        step is capturable as is; `real_batches` (and `real_labels`, for the conditional recipes) become the graph's
        static inputs: copy new data into them.  Returns a callable that replays the step.  Every replay draws fresh
        noise and updates the weights."""
        if (self.g_bucket.world > 1 or _FORCE_COLLECTIVES) and self.g_bucket.flat is not None:
            raise RuntimeError("capture(): gradient all-reduces cannot be captured; use capture_segments()")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step(real_batches, real_labels)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._static_losses = self.step(real_batches, real_labels)
        self._graph = graph

        def replay():
            graph.replay()
            _state.replays += 1                      # caches keyed by tensor versions: see _state.py
            return self._static_losses
        return replay

    def capture_segments(self, real_batches, real_labels=None, warmup=3):
        """The step as a CHAIN of hipGraphs cut at the gradient all-reduces, which stay ordinary RCCL calls between the
        replays: no collective is ever captured, yet the ~2000 kernel launches of a step leave the host loop -- the
        eager loop is at the edge of host-bound.  Segments:
        [generated batches + first critic pass] | [critic update + next pass] x (training_ratio - 1) |
        [critic update + generator pass] | [generator update]; the generator forward of the update still forks onto the
        second stream, but joins at the first cut (a captured graph must end with its branches joined).  The graphs share
        one memory pool and are replayed in capture order; autograd state crosses the cuts as ordinary tensors of that
        pool.  Returns a callable that replays the chain.

        If recording fails, the open capture is closed (the stream leaves capture mode), the partial graphs and their
        pool are dropped and the exception is re-raised: the caller can then run eagerly.  With several ranks the
        caller has to AGREE on the mode afterwards (bench.py all-reduces an ok flag): a rank that replays graphs while
        another runs eagerly would still issue the same collectives in the same order, but only by construction of
        step() -- do not rely on it."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.step(real_batches, real_labels)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        segments, cur = [], {}

        def begin():
            g = torch.cuda.CUDAGraph()
            # thread_local: calls of OTHER threads (the process group's watchdog polls its events) must not invalidate
            # a capture that contains none of their work
            ctx = torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local")
            ctx.__enter__()
            cur['g'], cur['ctx'] = g, ctx

        def end(bucket):
            if self._side_pending:                   # join the forked generator forward before the graph ends
                torch.cuda.current_stream().wait_stream(self._side)
                self._side_pending = False
            ctx = cur.pop('ctx')
            ctx.__exit__(None, None, None)
            segments.append((cur.pop('g'), bucket))

        def boundary(bucket):
            # no collective while recording: the captured kernels have not run, there is nothing to reduce -- and a rank
            # whose recording fails half-way must not leave its peers inside an all-reduce
            end(bucket)
            begin()

        self._boundary = boundary
        try:
            begin()
            losses = self.step(real_batches, real_labels)
            end(None)
        except BaseException as exc:
            ctx = cur.pop('ctx', None)
            if ctx is not None:                      # leave capture mode, as the context manager does on an error
                try:
                    ctx.__exit__(type(exc), exc, exc.__traceback__)
                except Exception:
                    pass
            self._side_pending = False
            segments.clear()
            cur.clear()
            del pool
            raise
        finally:
            self._boundary = None
        self._segments = segments

        def replay():
            for g, bucket in segments:
                g.replay()
                if bucket is not None:
                    bucket.allreduce_mean()
            _state.replays += 1                      # caches keyed by tensor versions: see _state.py
            return losses
        return replay


CIFAR10_UNCOND = dict(          # scripts/cifar10_resnet_sn_uncond.sh:4-7 + run.py:147-193
    generator=dict(block_sizes=(256, 256, 256), resamples=("UP", "UP", "UP"), first_block_shape=(4, 4, 256),
                   number_of_classes=10, block_norm='d', block_after_norm='uconv', last_norm='d',
                   last_after_norm='uconv', gan_type=None),
    discriminator=dict(input_image_shape=(32, 32, 3), block_sizes=(128, 128, 128, 128),
                       resamples=('DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=10, type=None, spectral=True,
                       sum_pool=True, conv_singular=False),
    image_shape=(32, 32, 3), conditional=False)

CIFAR10_COND = dict(            # scripts/cifar10_resnet_sn_cond.sh:5-8
    generator=dict(block_sizes=(128, 128, 128), resamples=("UP", "UP", "UP"), first_block_shape=(4, 4, 128),
                   number_of_classes=10, block_norm='d', block_after_norm='ucconv', last_norm='d',
                   last_after_norm='uconv', gan_type='PROJECTIVE'),
    discriminator=dict(input_image_shape=(32, 32, 3), block_sizes=(256, 256, 256, 256),
                       resamples=('DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=10, type='PROJECTIVE', spectral=True,
                       sum_pool=True, conv_singular=False),
    image_shape=(32, 32, 3), conditional=True)


# scripts/stl10_resnet_sn_uncond.sh:4-7 (generator_filters 256, discriminator_filters 128); run.py:152 first_block_w = 6,
# run.py:165-166 three UP blocks, run.py:333 images 48 x 48 x 3.  WC sites (N = 128): 6, 12, 12, 24, 24, 48, 48(final) at C = 256
STL10_UNCOND = dict(
    generator=dict(block_sizes=(256, 256, 256), resamples=("UP", "UP", "UP"), first_block_shape=(6, 6, 256),
                   number_of_classes=10, block_norm='d', block_after_norm='uconv', last_norm='d',
                   last_after_norm='uconv', gan_type=None),
    discriminator=dict(input_image_shape=(48, 48, 3), block_sizes=(128, 128, 128, 128),
                       resamples=('DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=10, type=None, spectral=True,
                       sum_pool=True, conv_singular=False),
    image_shape=(48, 48, 3), conditional=False)

# scripts/tinyimagenet_resnet_sn_cond_sa.sh:4-7 (generator_filters 128, discriminator_filters 1024, ufconv, filters_emb 15,
# PROJECTIVE); run.py:155-158 four UP blocks, run.py:172-173 200 classes, run.py:205-208 five critic blocks
# (filters/4, /2, 1, 1, 1; DOWN x3, SAME x2), run.py:335 images 64 x 64 x 3.  WC sites: 4, 8, 8, 16, 16, 32, 32, 64, 64(final)
# at C = 128; 200 classes > 64 samples per batch, so the block sites run per-sample coloring tables.
TINYIMAGENET_COND_SA = dict(
    generator=dict(block_sizes=(128, 128, 128, 128), resamples=("UP", "UP", "UP", "UP"), first_block_shape=(4, 4, 128),
                   number_of_classes=200, block_norm='d', block_after_norm='ufconv', filters_emb=15, last_norm='d',
                   last_after_norm='uconv', gan_type='PROJECTIVE'),
    discriminator=dict(input_image_shape=(64, 64, 3), block_sizes=(256, 512, 1024, 1024, 1024),
                       resamples=('DOWN', 'DOWN', 'DOWN', 'SAME', 'SAME'), number_of_classes=200, type='PROJECTIVE',
                       spectral=True, sum_pool=True, conv_singular=False, filters_emb=15),
    image_shape=(64, 64, 3), conditional=True)

# the four GPU configurations of BASELINE.json:configs, by the name bench.py --config takes
CONFIGS = {'cifar10_uncond': CIFAR10_UNCOND, 'cifar10_cond': CIFAR10_COND, 'stl10_uncond': STL10_UNCOND,
           'tinyimagenet_cond_sa': TINYIMAGENET_COND_SA}




def _dcgan(w, image, filters=512):
    """scripts/{cifar10,stl10}_dcgan_sn_uncond.sh (--arc dcgan, generator_filters = discriminator_filters = 512, norms d / uconv, SN critic,
    training_ratio 1, generator_batch_multiple 1) with the widths of run.py:167-171 (generator: F, F/2, F/4, three UP blocks from a
    (w, w, F) first block) and run.py:213-217 (critic: F/8, F/4, F/4, F/2, F/2, F, F; SAME and DOWN alternating)."""
    F_ = int(filters)
    return dict(
        generator=dict(block_sizes=(F_, F_ // 2, F_ // 4), resamples=("UP", "UP", "UP"), first_block_shape=(w, w, F_),
                       number_of_classes=10, block_norm='d', block_after_norm='uconv', last_norm='d', last_after_norm='uconv',
                       gan_type=None, arch='dcgan'),
        discriminator=dict(input_image_shape=image, block_sizes=(F_ // 8, F_ // 4, F_ // 4, F_ // 2, F_ // 2, F_, F_),
                           resamples=('SAME', 'DOWN', 'SAME', 'DOWN', 'SAME', 'DOWN', 'SAME'), number_of_classes=10, type=None,
                           spectral=True, sum_pool=True, conv_singular=False, arch='dcgan'),
        image_shape=image, conditional=False, training_ratio=1, generator_batch_multiple=1)


# the two DCGAN-SN recipes; NOT in CONFIGS (that is BASELINE.json's list, which bench.py takes by name)
DCGAN_CONFIGS = {'cifar10_dcgan_uncond': _dcgan(4, (32, 32, 3)), 'stl10_dcgan_uncond': _dcgan(6, (48, 48, 3))}

# scripts/cifar10_resnet_wgan_uncond.sh: --generator_adversarial_objective wgan --discriminator_adversarial_objective wgan
# --gradinet_penalty_weight 10, generator_filters = discriminator_filters = 128, norms d / uconv, no spectral normalisation, critic norm 'n'.
# NOT in CONFIGS either.  (The two conditional WGAN scripts: ACGAN_CONFIGS below.)
WGAN_CONFIGS = {'cifar10_wgan_uncond': dict(
    generator=dict(block_sizes=(128, 128, 128), resamples=("UP", "UP", "UP"), first_block_shape=(4, 4, 128),
                   number_of_classes=10, block_norm='d', block_after_norm='uconv', last_norm='d', last_after_norm='uconv', gan_type=None),
    discriminator=dict(input_image_shape=(32, 32, 3), block_sizes=(128, 128, 128, 128), resamples=('DOWN', 'DOWN', 'SAME', 'SAME'),
                       number_of_classes=10, type=None, spectral=False, sum_pool=True),
    image_shape=(32, 32, 3), conditional=False, objective='wgan', gradient_penalty_weight=10)}


def _wgan_cond(after_norm, filters_emb=None):
    """scripts/cifar10_resnet_wgan_cond.sh (ucconv) and scripts/cifar10_resnet_wgan_cond_sa.sh (ufconv, --filters_emb 4): --gan_type AC_GAN,
    wgan objectives, --gradinet_penalty_weight 10, generator_filters = discriminator_filters = 128, norms d / uconv at the last site, no
    spectral normalisation, critic norm 'n', --sum_pool 1.  The critic takes no label input (conditional=False): its class head is trained by
    GanTrainer(gan_type='AC_GAN') on the fused tail (tail.py)."""
    emb = {} if filters_emb is None else dict(filters_emb=filters_emb)
    return dict(
        generator=dict(block_sizes=(128, 128, 128), resamples=("UP", "UP", "UP"), first_block_shape=(4, 4, 128), number_of_classes=10,
                       block_norm='d', block_after_norm=after_norm, last_norm='d', last_after_norm='uconv', gan_type='AC_GAN', **emb),
        discriminator=dict(input_image_shape=(32, 32, 3), block_sizes=(128, 128, 128, 128), resamples=('DOWN', 'DOWN', 'SAME', 'SAME'),
                           number_of_classes=10, type='AC_GAN', spectral=False, sum_pool=True, fused_tail=True, **emb),
        image_shape=(32, 32, 3), conditional=False, objective='wgan', gradient_penalty_weight=10, gan_type='AC_GAN')


# the two conditional WGAN-GP recipes (the paper's cWC and cWC-sa rows); NOT in CONFIGS, and their schedules in a table of their own
ACGAN_CONFIGS = {'cifar10_wgan_cond': _wgan_cond('ucconv'), 'cifar10_wgan_cond_sa': _wgan_cond('ufconv', filters_emb=4)}
ACGAN_SCHEDULES = {
    'cifar10_wgan_cond': dict(lr_decay_schedule='linear', number_of_epochs=100),        # scripts/cifar10_resnet_wgan_cond.sh:7
    'cifar10_wgan_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=100),     # scripts/cifar10_resnet_wgan_cond_sa.sh:7
}


FUSED_PROJECTION_SHIPS = True       # profiles/projection_step.json: faster than torch's tail in every round at all three shapes


def _sn_cond(classes, after_norm, filters_emb=None):
    """scripts/cifar10_resnet_sn_cond_sa.sh (ufconv, --filters_emb 4), scripts/cifar100_resnet_sn_cond.sh (ucconv) and
    scripts/cifar100_resnet_sn_cond_sa.sh (ufconv, --filters_emb 10): CIFAR10_COND's networks -- hinge objectives, --gan_type PROJECTIVE,
    generator_filters 128, discriminator_filters 256, norms d / uconv at the last site, SN critic, --sum_pool 1 -- with the script's class
    count and block after-norm.  With 100 classes and 64 samples the generator's block sites run per-sample colouring tables.
    fused_projection: the critic's tail on tail.projection_tail, as profiles/projection_step.json decided."""
    emb = {} if filters_emb is None else dict(filters_emb=filters_emb)
    return dict(
        generator=dict(block_sizes=(128, 128, 128), resamples=("UP", "UP", "UP"), first_block_shape=(4, 4, 128), number_of_classes=classes,
                       block_norm='d', block_after_norm=after_norm, last_norm='d', last_after_norm='uconv', gan_type='PROJECTIVE', **emb),
        discriminator=dict(input_image_shape=(32, 32, 3), block_sizes=(256, 256, 256, 256), resamples=('DOWN', 'DOWN', 'SAME', 'SAME'),
                           number_of_classes=classes, type='PROJECTIVE', spectral=True, sum_pool=True, conv_singular=False,
                           fused_projection=FUSED_PROJECTION_SHIPS, **emb),
        image_shape=(32, 32, 3), conditional=True)


# the three further conditional SN recipes; NOT in CONFIGS (bench.py's names), their schedules in a table of their own
PROJECTION_CONFIGS = {'cifar10_cond_sa': _sn_cond(10, 'ufconv', filters_emb=4), 'cifar100_cond': _sn_cond(100, 'ucconv'),
                      'cifar100_cond_sa': _sn_cond(100, 'ufconv', filters_emb=10)}
PROJECTION_SCHEDULES = {
    'cifar10_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=50),           # scripts/cifar10_resnet_sn_cond_sa.sh:8
    'cifar100_cond': dict(lr_decay_schedule='linear', number_of_epochs=50),             # scripts/cifar100_resnet_sn_cond.sh:8
    'cifar100_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=50),          # scripts/cifar100_resnet_sn_cond_sa.sh:8
}


MNIST_RAGGED_SHIPS = True           # profiles/mnist_step.json: faster in every one of 7 rounds on both recipes


def _mnist(filters, after_norm, gan_type):
    """scripts/{mnist,fashionmnist}_resnet_sn_{uncond,cond}.sh with run.py:147-237 for a dataset whose name ends in 'mnist': one output
    channel, a (7, 7, F) first block (run.py:152) and two UP blocks of F filters (run.py:165-166) -- 28 x 28 x 1 images --, norms d / uconv at
    the last site, hinge objectives, the four-block critic of 128 filters with spectral normalisation and --sum_pool 1; the conditional
    scripts add --gan_type PROJECTIVE and the block after-norm ucconv.  At the recipes' batch of 64 the 7x7 grids have N*H*W = 3136 =
    24 * 128 + 64 (15680 in the five-round generation): the block kernels take them on a partial last tile where ragged_conv is on.
    fused_projection stays off: the tail has not been measured at (128, 49, 128, 10)."""
    conditional = gan_type is not None
    return dict(
        generator=dict(output_channels=1, block_sizes=(filters, filters), resamples=("UP", "UP"), first_block_shape=(7, 7, filters),
                       number_of_classes=10, block_norm='d', block_after_norm=after_norm, last_norm='d', last_after_norm='uconv',
                       gan_type=gan_type, ragged_conv=MNIST_RAGGED_SHIPS),
        discriminator=dict(input_image_shape=(28, 28, 1), block_sizes=(128, 128, 128, 128), resamples=('DOWN', 'DOWN', 'SAME', 'SAME'),
                           number_of_classes=10, type=gan_type, spectral=True, sum_pool=True, conv_singular=False,
                           ragged_conv=MNIST_RAGGED_SHIPS),
        image_shape=(28, 28, 1), conditional=conditional)


# the four MNIST-family recipes; NOT in CONFIGS (bench.py's names), their schedules in a table of their own
MNIST_CONFIGS = {'mnist_uncond': _mnist(256, 'uconv', None), 'mnist_cond': _mnist(128, 'ucconv', 'PROJECTIVE'),
                 'fashionmnist_uncond': _mnist(256, 'uconv', None), 'fashionmnist_cond': _mnist(128, 'ucconv', 'PROJECTIVE')}
MNIST_SCHEDULES = {
    'mnist_uncond': dict(lr_decay_schedule=None, number_of_epochs=5),                   # scripts/mnist_resnet_sn_uncond.sh:7 (no schedule given)
    'mnist_cond': dict(lr_decay_schedule=None, number_of_epochs=5),                     # scripts/mnist_resnet_sn_cond.sh:7
    'fashionmnist_uncond': dict(lr_decay_schedule='linear', number_of_epochs=20),       # scripts/fashionmnist_resnet_sn_uncond.sh:7
    'fashionmnist_cond': dict(lr_decay_schedule='linear', number_of_epochs=20),         # scripts/fashionmnist_resnet_sn_cond.sh:7
}


# profiles/imagenet_step.json (tools/imagenet_step.py: the captured G+D step at batch 64 with the generator's mark on against the same networks
# with it off, 7 alternating rounds): the marked step is faster in every round
IMAGENET_SLIM_SHIPS = True


# scripts/imagenet_resnet_sn_cond_sa.sh with run.py:147-237 for --dataset imagenet.  Generator: --generator_filters 128 (script line 6), a
# (4, 4, 128) first block (run.py:152-153), five UP blocks of F, F, F, F/2, F/4 filters (run.py:159-163), 1000 classes (run.py:172-173), norms
# d / ufconv in the blocks and d / uconv at the last site (script lines 5-6), --filters_emb 32 (line 8), --gan_type PROJECTIVE (line 7).
# Critic: --discriminator_filters 1024 (line 6), widths F/16, F/8, F/4, F/2, F, F (run.py:206-207), five DOWN blocks and a SAME one
# (run.py:208), 128 x 128 x 3 images (run.py:334), spectral normalisation (line 7), --sum_pool 1 (run.py:310, its default), hinge objectives
# (lines 4-5), batch 64 (line 8).  Its 128 -> 64 and 64 -> 32 generator blocks (64 x 64 and 128 x 128 pixels) run on the block kernels where
# slim_conv is on.  --shred_disc_batch 1 (line 8) is NOT reproduced: it lives in the reference's gan/ runtime,
# which is not part of the tree this project was built from.  NOT in CONFIGS (bench.py's names); the schedule in a table of its own.
IMAGENET_CONFIGS = {'imagenet_cond_sa': dict(
    generator=dict(block_sizes=(128, 128, 128, 64, 32), resamples=("UP", "UP", "UP", "UP", "UP"), first_block_shape=(4, 4, 128),
                   number_of_classes=1000, block_norm='d', block_after_norm='ufconv', filters_emb=32, last_norm='d',
                   last_after_norm='uconv', gan_type='PROJECTIVE', slim_conv=IMAGENET_SLIM_SHIPS),
    discriminator=dict(input_image_shape=(128, 128, 3), block_sizes=(64, 128, 256, 512, 1024, 1024),
                       resamples=('DOWN', 'DOWN', 'DOWN', 'DOWN', 'DOWN', 'SAME'), number_of_classes=1000, type='PROJECTIVE',
                       spectral=True, sum_pool=True, conv_singular=False, filters_emb=32),
    image_shape=(128, 128, 3), conditional=True)}
IMAGENET_SCHEDULES = {
    # scripts/imagenet_resnet_sn_cond_sa.sh:7 (linear, 450 epochs) and :8 (--generator_lr 5e-4 --discriminator_lr 5e-4)
    'imagenet_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=450, generator_lr=5e-4, discriminator_lr=5e-4),
}


def slim_config(config, on=True):
    """The same recipe with every convolution layer of the GENERATOR marked slim_conv (make_generator(slim_conv=True), DESIGN.md section
    4.22): the block kernels then take its 64- and 32-channel layers.  The critic is never touched: its mark is slim_blocks, a name and a
    helper of its own (slim_blocks_config).  A copy of any entry, the entry itself is left alone; on=False: the mark off."""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(slim_conv=bool(on))
    return out


# profiles/imagenet_critic_step.json (tools/imagenet_critic_step.py: the captured G+D step at batch 64 with the critic's mark on against the same
# networks with it off, the generator marked slim_conv in both, 7 alternating rounds): the marked step is faster in every round (DESIGN.md
# section 4.23)
IMAGENET_SLIM_BLOCKS_SHIPS = True


def slim_blocks_config(config, on=True):
    """The same recipe with every convolution layer of the CRITIC marked slim_blocks (make_discriminator(slim_blocks=True), DESIGN.md
    section 4.23): its 64-wide block layers run on the block kernels and the fused critic nodes, its image layers take their data gradient
    on the narrow-output kernel.  The generator is left alone.  A copy of any entry, the entry itself is left alone; on=False: the mark
    off.  The shipping form of the ImageNet recipe is
    narrow_last_config(slim_blocks_config(IMAGENET_CONFIGS['imagenet_cond_sa'], IMAGENET_SLIM_BLOCKS_SHIPS), IMAGENET_NARROW_LAST_SHIPS):
    this helper's copy with the generator's last layer marked by narrow_last_config below."""
    import copy
    out = copy.deepcopy(config)
    out['discriminator'].update(slim_blocks=bool(on))
    return out


# profiles/imagenet_last_step.json (tools/imagenet_last_step.py: the captured G+D step at batch 64 with Generator.Final marked narrow_last
# against the same networks with the mark off, both other marks on in both legs, 7 alternating rounds).  The rule of
# sections 4.22 / 4.23: True only if the marked step is faster in every round.
IMAGENET_NARROW_LAST_SHIPS = True


def narrow_last_config(config, on=True):
    """The same recipe with the GENERATOR's last layer, Generator.Final, marked narrow_last (make_generator(narrow_last=True), DESIGN.md
    section 4.24): its forward, weight gradient and data gradient run on the narrow kernels (conv._NarrowLastConv) instead of the GEMM + fold
    and convolution_backward.  No other layer and not the critic.  A copy of any entry, the entry itself is left alone; on=False: the mark
    off.  The shipping form of the ImageNet recipe is
    narrow_last_config(slim_blocks_config(IMAGENET_CONFIGS['imagenet_cond_sa'], IMAGENET_SLIM_BLOCKS_SHIPS), IMAGENET_NARROW_LAST_SHIPS)."""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(narrow_last=bool(on))
    return out


# --lr_decay_schedule / --number_of_epochs of each recipe's script: GanTrainer's arguments of the same names (the config tables above carry
# the networks alone and are left as they are).  build_trainer(CONFIGS[name], **RECIPE_SCHEDULES[name]) trains the recipe at its script's rates.
RECIPE_SCHEDULES = {
    'cifar10_uncond': dict(lr_decay_schedule='linear', number_of_epochs=50),            # scripts/cifar10_resnet_sn_uncond.sh:7
    'cifar10_cond': dict(lr_decay_schedule='dropat30', number_of_epochs=50),            # scripts/cifar10_resnet_sn_cond.sh:8
    'stl10_uncond': dict(lr_decay_schedule='linear', number_of_epochs=100),             # scripts/stl10_resnet_sn_uncond.sh:7
    'tinyimagenet_cond_sa': dict(lr_decay_schedule='linear', number_of_epochs=100),     # scripts/tinyimagenet_resnet_sn_cond_sa.sh:7
    'cifar10_dcgan_uncond': dict(lr_decay_schedule='linear', number_of_epochs=100),     # scripts/cifar10_dcgan_sn_uncond.sh:7
    'stl10_dcgan_uncond': dict(lr_decay_schedule='linear', number_of_epochs=200),       # scripts/stl10_dcgan_sn_uncond.sh:7
    'cifar10_wgan_uncond': dict(lr_decay_schedule='linear', number_of_epochs=100),      # scripts/cifar10_resnet_wgan_uncond.sh:7
}


def dcgan_sites(config, batch):
    """(name, N, H, W, C) of every WC site of a DC generator at batch size `batch`: one on each block's INPUT (generator.DCBlockUp is
    pre-activation), then the final site generator.py:154 -- len(blocks) + 1 in all."""
    g = config['generator']
    h, w, c = g['first_block_shape']
    sites = []
    for i, (bs, rs) in enumerate(zip(g['block_sizes'], g['resamples'])):
        sites.append((f'Generator.{i}.bn', batch, h, w, c))
        if rs == 'UP':
            h, w = 2 * h, 2 * w
        c = int(bs)
    sites.append(('Generator.BN.Final', batch, h, w, c))
    return sites


def baseline_config(config, after_norm='ucs', fused=True):
    """The batch-norm generator the reference sets WC against (run.py:277,285: norm 'b' is its default, after-norm 'ucs'; 'ccs' is the
    conditional batch norm of the cWC comparisons): a copy of a CONFIGS entry with both norms 'b', both after-norms `after_norm`, on
    the fused HIP route (fused=False: torch's BatchNorm2d and the coloring branches one by one).  The entry itself is left alone."""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(block_norm='b', last_norm='b', block_after_norm=after_norm, last_after_norm=after_norm,
                            fused_batch_norm=bool(fused))
    return out


def zca_config(config):
    """The same generator with ZCA whitening at every WC site (DecorelationNormalization(decomposition='zca'), the commented alternative of
    generator.py:24): a copy of a CONFIGS entry, the entry itself is left alone.  No shipped configuration uses it."""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(decomposition='zca')
    return out


def fused_projection_config(config):
    """The same recipe with the projection critic's tail on the HIP route (make_discriminator(fused_projection=True), DESIGN.md section
    4.20): a copy of any entry, the entry itself is left alone.  Without effect on a critic of another type."""
    import copy
    out = copy.deepcopy(config)
    out['discriminator'].update(fused_projection=True)
    return out


def ragged_config(config, on=True):
    """The same recipe with every convolution layer of both networks marked ragged_conv (make_generator / make_discriminator(ragged_conv=
    True)): the block kernels then take grids whose N*H*W is a multiple of 32 on a partial last tile.  A copy of any
    entry, the entry itself is left alone; on=False gives the copy with the mark off."""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(ragged_conv=bool(on))
    out['discriminator'].update(ragged_conv=bool(on))
    return out


def renorm_config(config):
    """The same generator with renorm whitening at every WC site (norm 'dr': DecorelationNormalization(renorm=True), generator.py:26):
    a copy of a CONFIGS entry, the entry itself is left alone.  No shipped configuration uses it.  (A renorm layer has no grouped
    form: GanTrainer.generate runs separate generator passes for such a generator.)"""
    import copy
    out = copy.deepcopy(config)
    out['generator'].update(block_norm='dr', last_norm='dr')
    return out


def wc_sites(config, batch):
    """(name, N, H, W, C) of every WC site of the config's generator at batch size `batch` (bn1 on the
    block input, bn2 after the upsampling conv1, then the final site generator.py:154)."""
    g = config['generator']
    h, w, c = g['first_block_shape']
    sites = []
    for i, (bs, rs) in enumerate(zip(g['block_sizes'], g['resamples'])):
        sites.append((f'Generator.{i}.bn1', batch, h, w, c))
        if rs == 'UP':
            h, w = 2 * h, 2 * w
        c = int(bs)
        sites.append((f'Generator.{i}.bn2', batch, h, w, c))
    sites.append(('Generator.BN.Final', batch, h, w, c))
    return sites


def build_trainer(config=CIFAR10_UNCOND, device='cuda', process_group=None, sync_wc=False, **kw):
    from .discriminator import make_discriminator
    from .generator import make_generator
    G = make_generator(process_group=process_group if sync_wc else None, **config['generator']).to(device)
    D = make_discriminator(**config['discriminator']).to(device)
    broadcast_state(G, group=process_group)
    broadcast_state(D, group=process_group)
    # a recipe's own schedule (DCGAN_CONFIGS) and objective (WGAN_CONFIGS), unless the caller overrides them
    for key in ('training_ratio', 'generator_batch_multiple', 'objective', 'gradient_penalty_weight', 'gan_type'):
        if key in config:
            kw.setdefault(key, config[key])
    return GanTrainer(G, D, number_of_classes=config['generator']['number_of_classes'],
                      conditional=config['conditional'], process_group=process_group, **kw)
