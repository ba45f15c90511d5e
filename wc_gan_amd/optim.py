"""Learning-rate schedules of the recipes (run.py:99-144, --lr_decay_schedule) and the Adam that runs them: one HIP pass over a network's
parameters per update (csrc/wc_adam.hip), with the update counter and the step's scalars on the device -- DESIGN.md section 4.18.

`it` is the number of updates ALREADY applied to the network, so the first update runs at multiplier 1.  The runtime that evaluates the
schedule upstream (`gan.gan`) is not part of the reference tree: this convention is ours.
"""
from __future__ import annotations

import ctypes

import torch

KINDS = {None: 0, 'linear': 1, 'half-linear': 2, 'linear-end': 3, 'dropat': 4}       # the `kind` of wc_adam_tick
CHUNK = 2048            # elements per workgroup of wc_adam_update_f32 (a multiple of 1024)
DECAY_AT = 0.828        # 'linear-end': run.py:117


def parse_schedule(kind):
    """'dropat30' -> ('dropat', 30); the other kinds -> (kind, None)."""
    if kind is None or kind in ('linear', 'half-linear', 'linear-end'):
        return kind, None
    if isinstance(kind, str) and kind.startswith('dropat') and kind[6:].isdigit():
        return 'dropat', int(kind[6:])
    raise ValueError(f"lr_decay_schedule {kind!r}: None, 'linear', 'half-linear', 'linear-end' or 'dropatN'")


def lr_multiplier(kind, it, total=None, ratio=1):
    """The factor on the learning rate of the update that follows `it` applied ones, in float64.  `total`: 1000 x number_of_epochs for the
    generator, times training_ratio for the critic.  `ratio` ('dropatN' alone): 1 for the generator, training_ratio for the critic --
    the drop is at N x 1000 x ratio updates."""
    base, n = parse_schedule(kind)
    if base is None:
        return 1.0
    if total is None or not total > 0:
        raise ValueError(f"schedule {kind!r} needs total > 0")
    it, total = float(it), float(total)
    lin = max(0.0, 1.0 - it / total)
    if base == 'linear':
        return lin
    if base == 'half-linear':
        return lin if it < 0.5 * total else 0.5
    if base == 'linear-end':
        return min(1.0, max(0.0, (total - it) / (total - DECAY_AT * total)))
    return (1.0 if it < n * 1000.0 * ratio else 0.1) * lin


def _pack(numels, chunk, capacity):
    """Which tensors go in which launch of wc_adam_update_f32, and each launch's chunk prefix sum: a list of (indices, chunk_start) with
    len(indices) <= capacity, chunk_start[0] = 0 and chunk_start[j + 1] - chunk_start[j] = ceil(numels[indices[j]] / chunk).  Tensors keep
    their order; every tensor is in exactly one launch."""
    if chunk < 1 or capacity < 1:
        raise ValueError("_pack: chunk and capacity are positive")
    launches = []
    for first in range(0, len(numels), capacity):
        idx = list(range(first, min(len(numels), first + capacity)))
        start = [0]
        for i in idx:
            if numels[i] < 1:
                raise ValueError("_pack: an empty tensor has no workgroup")
            start.append(start[-1] + (numels[i] + chunk - 1) // chunk)
        launches.append((idx, start))
    return launches


def _dense(t):
    """Dense and non-overlapping: the strides are a permutation of a contiguous tensor's."""
    dims = sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1)
    acc = 1
    for st, sz in dims:
        if st != acc:
            return False
        acc *= sz
    return True


class ScheduledAdam:
    """torch.optim.Adam's formula (no weight decay, no amsgrad) times a schedule's multiplier.  With schedule=None the same optimiser to
    rounding.

    * float32 parameters on the GPU: wc_adam_tick + wc_adam_update_f32, no synchronisation, no allocation after the first step,
      capturable.  Anything else (CPU, float64): the same maths in plain torch ops.
    * exp_avg and exp_avg_sq are two flat fp32 buffers (each parameter's segment padded to four elements); with beta1 == 0 exp_avg is the
      gradient and is not kept.  state[p] has views of them shaped like p, and 'step', the optimiser's ONE counter.
    * A parameter whose .grad is None at a step is skipped: its exp_avg_sq does not decay, and it shares the one counter (torch keeps a
      counter per parameter, so there a parameter that sat out k steps has a bias correction k steps younger).
    * `ratio`: see lr_multiplier ('dropatN')."""

    def __init__(self, params, lr, betas, eps=1e-8, schedule=None, total_iters=None, ratio=1):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("ScheduledAdam: no parameter to optimise")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        base, n = parse_schedule(schedule)
        if base is not None and not (total_iters is not None and total_iters > 0):
            raise ValueError(f"schedule {schedule!r} needs total_iters > 0")
        self.schedule, self.total_iters, self.ratio = schedule, (None if total_iters is None else float(total_iters)), ratio
        self._kind, self._drop_at = KINDS[base], (0.0 if n is None else n * 1000.0 * ratio)
        if not (self.lr >= 0.0 and 0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0 and self.eps >= 0.0):
            raise ValueError("ScheduledAdam: lr >= 0, 0 <= beta < 1, eps >= 0")
        dev, dtype = self.params[0].device, self.params[0].dtype
        for p in self.params:
            if p.device != dev or p.dtype != dtype:
                raise ValueError("ScheduledAdam: the parameters of one optimiser share one device and dtype")
            if not _dense(p):
                raise ValueError(f"ScheduledAdam: a parameter of shape {tuple(p.shape)} and strides {p.stride()} is not dense and non-overlapping")
            if p.numel() < 1 or p.numel() >= 2 ** 31 - 2 ** 20:
                raise ValueError("ScheduledAdam: 1 <= numel < 2^31 - 2^20 per parameter")
        self.hip = dev.type == 'cuda' and dtype == torch.float32
        self._offsets, off = [], 0
        for p in self.params:
            self._offsets.append(off)
            off += (p.numel() + 3) // 4 * 4
        self._moment_elems = off
        self.exp_avg_sq = torch.zeros(off, dtype=dtype, device=dev)
        self.exp_avg = torch.zeros(off, dtype=dtype, device=dev) if self.betas[0] != 0.0 else None
        self.counter = torch.zeros((), dtype=torch.int64, device=dev)
        self.record = torch.zeros(4, dtype=torch.float32, device=dev) if self.hip else None
        self.state = {}
        for p, o in zip(self.params, self._offsets):
            st = {'step': self.counter, 'exp_avg_sq': self.exp_avg_sq.as_strided(p.shape, p.stride(), o)}
            if self.exp_avg is not None:
                st['exp_avg'] = self.exp_avg.as_strided(p.shape, p.stride(), o)
            self.state[p] = st
        self._restrided = {}            # parameter index -> the buffer a gradient of other strides is copied into
        self._tables, self._key = [], None
        if self.hip:
            from . import _lib
            lib = _lib.load()
            if lib.wc_adam_capacity() != _lib.ADAM_CAPACITY:
                raise _lib.WcHipError("wc_adam_table: the library's capacity differs from the binding's; rebuild it")

    # -- gradients -------------------------------------------------------------------------------------------------------
    def _grads(self):
        """Each parameter's gradient in the parameter's own element order (None: skipped this step).  A gradient of other strides is
        copied into a buffer of the parameter's strides, allocated once."""
        out = []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is not None and g.shape != p.shape:
                raise ValueError(f"ScheduledAdam: a gradient of shape {tuple(g.shape)} for a parameter of shape {tuple(p.shape)}")
            if g is not None and any(sg != sp for sg, sp, n in zip(g.stride(), p.stride(), p.shape) if n != 1):
                buf = self._restrided.get(i)
                if buf is None:
                    buf = self._restrided[i] = torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device)
                buf.copy_(g)
                g = buf
            out.append(g)
        return out

    # -- the HIP route ---------------------------------------------------------------------------------------------------
    def _build_tables(self, grads):
        from . import _lib
        live = [i for i, g in enumerate(grads) if g is not None]
        tables = []
        for idx, start in _pack([self.params[i].numel() for i in live], CHUNK, _lib.ADAM_CAPACITY):
            t = _lib.AdamTable()
            for j, k in enumerate(idx):
                i = live[k]
                t.param[j], t.grad[j] = self.params[i].data_ptr(), grads[i].data_ptr()
                t.moment_off[j], t.numel[j] = self._offsets[i], self.params[i].numel()
            for j, s in enumerate(start):
                t.chunk_start[j] = s
            t.count, t.chunk = len(idx), CHUNK
            tables.append(t)
        return tables

    def _step_hip(self, grads):
        from . import _lib
        from .ops import _stream
        lib = _lib.load()
        for g in grads:
            if g is not None and (g.dtype != torch.float32 or g.device != self.params[0].device):
                raise TypeError("ScheduledAdam: a gradient's dtype or device differs from its parameter's")
        key = tuple(0 if g is None else g.data_ptr() for g in grads) + tuple(p.data_ptr() for p in self.params)
        if key != self._key:              # (the pointers of a captured step never change; eager autograd hands out new gradients)
            self._tables, self._key = self._build_tables(grads), key
        st = _stream()
        _lib.check(lib.wc_adam_tick(self.counter.data_ptr(), self.record.data_ptr(), self.lr, self.betas[0], self.betas[1], self._kind,
                                    self.total_iters or 0.0, self._drop_at, st), "wc_adam_tick")
        m = None if self.exp_avg is None else self.exp_avg.data_ptr()
        for t in self._tables:
            _lib.check(lib.wc_adam_update_f32(ctypes.byref(t), m, self.exp_avg_sq.data_ptr(), self._moment_elems, self.record.data_ptr(),
                                              self.betas[0], self.betas[1], self.eps, st), "wc_adam_update_f32")

    # -- the same maths in torch ops (CPU, float64) --------------------------------------------------------------------------
    def _scalars_torch(self):
        """(lr mult / bc1, 1 / sqrt(bc2)) as float64 0-d tensors on the parameters' device, from the counter; no synchronisation."""
        it = self.counter.to(torch.float64)
        base, _ = parse_schedule(self.schedule)
        one = torch.ones((), dtype=torch.float64, device=it.device)
        if base is None:
            mult = one
        else:
            total = self.total_iters
            lin = (1.0 - it / total).clamp_min(0.0)
            if base == 'linear':
                mult = lin
            elif base == 'half-linear':
                mult = torch.where(it < 0.5 * total, lin, 0.5 * one)
            elif base == 'linear-end':
                mult = ((total - it) / (total - DECAY_AT * total)).clamp(0.0, 1.0)
            else:
                mult = torch.where(it < self._drop_at, one, 0.1 * one) * lin
        step = it + 1.0
        b1, b2 = self.betas
        bc1 = 1.0 - b1 ** step
        bc2 = 1.0 - b2 ** step
        return self.lr * mult / bc1, 1.0 / torch.sqrt(bc2)

    @torch.no_grad()
    def _step_torch(self, grads):
        a, r = self._scalars_torch()
        dt = self.params[0].dtype
        a, r = a.to(dt), r.to(dt)
        b1, b2 = self.betas
        for p, g in zip(self.params, grads):
            if g is None:
                continue
            st = self.state[p]
            v = st['exp_avg_sq']
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            if self.exp_avg is not None:
                m = st['exp_avg']
                m.add_((g - m) * (1.0 - b1))
            else:
                m = g
            p.sub_(a * (m / (v.sqrt() * r + self.eps)))
        self.counter.add_(1)

    # -- torch.optim's surface -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self):
        grads = self._grads()
        if all(g is None for g in grads):
            self.counter.add_(1)          # (an update that moved nothing still counts: the schedule follows the trainer's calls)
            return
        if self.hip:
            self._step_hip(grads)
        else:
            self._step_torch(grads)

    def current_lr(self):
        """The rate of the NEXT update (lr x multiplier at the counter's value), for logging.  Synchronises."""
        return self.lr * lr_multiplier(self.schedule, int(self.counter.item()), self.total_iters, self.ratio)

    def state_dict(self):
        """The counter and both flat buffers (host copies), and the numels that fix the buffers' layout.  The rate, the betas and the
        schedule are the constructor's: a resumed run passes them again.  Synchronises."""
        return dict(step=int(self.counter.item()), exp_avg_sq=self.exp_avg_sq.detach().cpu().clone(),
                    exp_avg=None if self.exp_avg is None else self.exp_avg.detach().cpu().clone(),
                    numels=[p.numel() for p in self.params])

    def load_state_dict(self, sd):
        if list(sd['numels']) != [p.numel() for p in self.params]:
            raise ValueError("ScheduledAdam.load_state_dict: the state belongs to other parameters")
        if (sd['exp_avg'] is None) != (self.exp_avg is None):
            raise ValueError("ScheduledAdam.load_state_dict: the state was saved with another beta1 (exp_avg is kept only when beta1 != 0)")
        with torch.no_grad():
            self.exp_avg_sq.copy_(sd['exp_avg_sq'])
            if self.exp_avg is not None:
                self.exp_avg.copy_(sd['exp_avg'])
            self.counter.fill_(int(sd['step']))
