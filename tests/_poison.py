"""Poisoned, guard-banded device allocations for the GPU tests (not collected: no test_ prefix).

    with Poison(0x7B) as P:
        x = P.guarded(x_np)             # a test's own input, inside poisoned guard bands
        y = ops.apply(x, ...)           # every torch.empty / empty_like / new_empty / empty_strided of the call is poisoned
        P.check_guards()                # synchronises; every guard byte must still hold the pattern

While the context is open, every real CUDA tensor with numel() > 0 that torch.empty, torch.empty_like, torch.empty_strided or
Tensor.new_empty return is filled with one byte pattern:

    0x00   what fresh allocator memory usually holds
    0xFF   NaN in every float width, -1 / UINT_MAX as an integer
    0x7B   large but finite in every float width (f16 61280, f32 ~1.3e36, f64 ~1e289) and a large positive counter: catches the reads a
           NaN slips past (fmaxf, comparisons, a `>= target` wait)

A contiguous request comes back as a view into a larger buffer with GUARD bytes on both sides, filled with the same pattern; the offset
is a multiple of 512 bytes, so the allocator's alignment is kept.  A strided request (channels-last empty_like) gets the fill only.
Under graph capture the fills are captured too: every replay poisons its pool buffers again.  torch.zeros / torch.full / torch.ones are
left alone: those are the code's documented zero-initialisation contracts.  Meta and fake tensors (the register_fake kernels) are left
alone as well.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

PATTERNS = (0x00, 0xFF, 0x7B)
GUARD = 4096                    # bytes on each side; a multiple of 512
_PKG = os.sep + "wc_gan_amd" + os.sep
_HERE = os.path.abspath(__file__)


def _site():
    """The first wc_gan_amd/ frame of the allocating call stack (else the first frame outside this module)."""
    f = sys._getframe(2)
    first = None
    while f is not None:
        fn = f.f_code.co_filename
        if _PKG in fn:
            return f"{fn.split(_PKG)[-1]}:{f.f_lineno} ({f.f_code.co_name})"
        if first is None and os.path.abspath(fn) != _HERE and "torch" + os.sep not in fn:
            first = f"{os.path.basename(fn)}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return first or "?"


def _real_cuda(t):
    return type(t) is torch.Tensor and t.is_cuda and not t.is_meta and t.layout == torch.strided and t.numel() > 0 \
        and t.dtype not in (torch.bool,) and not t.is_complex()


def _row_major(shape):
    st, acc = [], 1
    for n in reversed(tuple(shape)):
        st.append(acc)
        acc *= n
    return tuple(reversed(st))


def bits(t):
    """A tensor's bytes on the host (bit-level comparison, NaN payloads included)."""
    t = t.detach()
    if t.is_cuda:
        t = t.cpu()
    return t.contiguous().view(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Poison:
    def __init__(self, pattern, guards=True):
        self.pattern = int(pattern) & 0xFF
        self.guards = guards
        self.records = []               # (buffer, nbytes of the payload, allocation site)
        self.filled = 0
        self._saved = None

    # -- allocation ------------------------------------------------------------------------------------------------------
    def _fill_storage(self, t):
        """Fill a dense (possibly strided) tensor's bytes with the pattern, whatever its dtype."""
        n = t.untyped_storage().nbytes()
        raw = self._orig_empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), 0, (n,))
        raw.fill_(self.pattern)
        self.filled += 1

    def _guarded_alloc(self, shape, dtype, device, requires_grad, site):
        """A contiguous tensor placed inside a poisoned guard-banded buffer."""
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.tensor([], dtype=dtype).element_size()
        buf = self._orig_empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        buf.fill_(self.pattern)
        self.filled += 1
        out = buf[GUARD:GUARD + nbytes].view(dtype).view(shape)
        self.records.append((buf, nbytes, site))
        if requires_grad:
            out = out.detach().requires_grad_(True)
        return out

    def _post(self, t, requires_grad=False, contiguous_request=True):
        if not _real_cuda(t):
            return t
        if self.guards and contiguous_request and t.stride() == _row_major(t.shape):     # (a channels-last 1x1 weight is "contiguous" too)
            return self._guarded_alloc(t.shape, t.dtype, t.device, requires_grad, _site())
        self._fill_storage(t)
        return t

    def __enter__(self):
        self._orig_empty = torch.empty
        self._orig_empty_like = torch.empty_like
        self._orig_empty_strided = torch.empty_strided
        self._orig_new_empty = torch.Tensor.new_empty
        P = self

        def empty(*args, **kw):
            if kw.get("out") is not None:
                return P._orig_empty(*args, **kw)
            mf = kw.get("memory_format", torch.contiguous_format)
            t = P._orig_empty(*args, **kw)
            return P._post(t, bool(kw.get("requires_grad", False)), mf == torch.contiguous_format)

        def empty_like(inp, *args, **kw):
            t = P._orig_empty_like(inp, *args, **kw)
            return P._post(t, bool(kw.get("requires_grad", False)), True)

        def empty_strided(*args, **kw):
            t = P._orig_empty_strided(*args, **kw)
            return P._post(t, False, False)         # the caller asked for these strides: fill only

        def new_empty(self_, *args, **kw):
            t = P._orig_new_empty(self_, *args, **kw)
            return P._post(t, bool(kw.get("requires_grad", False)), True)

        self._saved = (empty, empty_like, empty_strided, new_empty)
        torch.empty, torch.empty_like, torch.empty_strided = empty, empty_like, empty_strided
        torch.Tensor.new_empty = new_empty
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, torch.empty_strided = self._orig_empty, self._orig_empty_like, self._orig_empty_strided
        torch.Tensor.new_empty = self._orig_new_empty
        return False

    # -- test inputs -----------------------------------------------------------------------------------------------------
    def guarded(self, a, dtype=None):
        """A test input (numpy array or tensor) copied onto the device inside poisoned guard bands."""
        if isinstance(a, np.ndarray):
            src = torch.from_numpy(np.ascontiguousarray(a))
        else:
            src = a.detach()
        if dtype is not None:
            src = src.to(dtype)
        if src.numel() == 0:
            return src.to("cuda")
        out = self._guarded_alloc(src.shape, src.dtype, torch.device("cuda", torch.cuda.current_device()), False, "test input")
        out.copy_(src)
        return out

    # -- checks ----------------------------------------------------------------------------------------------------------
    def check_guards(self):
        """Synchronise and assert that every guard byte still holds the pattern; a failure names the allocation site."""
        torch.cuda.synchronize()
        if not self.records:
            return
        heads = torch.stack([b[:GUARD] for b, _, _ in self.records])
        tails = torch.stack([b[GUARD + n:GUARD + n + GUARD] for b, n, _ in self.records])
        bad = ((heads != self.pattern).any(1) | (tails != self.pattern).any(1)).nonzero().view(-1).tolist()
        if bad:
            lines = []
            for i in bad[:8]:
                b, n, site = self.records[i]
                h = int((b[:GUARD] != self.pattern).sum())
                t = int((b[GUARD + n:] != self.pattern).sum())
                lines.append(f"{site}: {n} bytes, {h} guard bytes changed in front, {t} behind")
            raise AssertionError(f"pattern 0x{self.pattern:02X}: {len(bad)} of {len(self.records)} guarded allocations were "
                                 "written outside their bounds:\n  " + "\n  ".join(lines))

    def release(self):
        self.records.clear()


def flatten(r):
    """Every tensor in a nest of tuples / lists / dicts, in order."""
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, dict):
        return [t for k in sorted(r) for t in flatten(r[k])]
    if isinstance(r, (list, tuple)):
        return [t for x in r for t in flatten(x)]
    return []


def run_patterns(fn, patterns=PATTERNS):
    """fn(P) -> a nest of tensors, under each pattern: asserts (a) bit-identical outputs across the patterns and (b) intact guards.
    Returns {pattern: host tensors} for the caller's oracle check.  A dict of tensors comes back as a dict (by name), anything else as a list."""
    outs = {}
    for p in patterns:
        with Poison(p) as P:
            r = fn(P)
            P.check_guards()
            if isinstance(r, dict):
                outs[p] = {k: v.detach().cpu().clone() for k, v in r.items()}
            else:
                outs[p] = [t.detach().cpu().clone() for t in flatten(r)]
            P.release()
    ref = outs[patterns[0]]
    for p in patterns[1:]:
        assert len(outs[p]) == len(ref)
        names = list(ref) if isinstance(ref, dict) else range(len(ref))
        diff = [i for i in names if not same_bits(ref[i], outs[p][i])]
        assert not diff, f"outputs {diff} differ in their bits between pattern 0x{patterns[0]:02X} and 0x{p:02X}"
    return outs
