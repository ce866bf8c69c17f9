"""Plumbing under every front-end: stream handle, pointers, scratch, cached constants, NHWC helpers, the pinned upload ring and the
gradient hand-over protocol between the heads and ``unet_ops``.  Depends on ``_cabi`` and torch only (module layers)."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import _cabi
from ._cabi import BF16, F16, F32, call

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The current HIP stream's handle.  Asked ~90 times per training step: `torch.cuda.current_stream().cuda_stream` builds a Python
    Stream object each time (9 us, 0.85 ms of host time per step -- the host is co-critical at this step time); the two raw
    bindings cost well under a microsecond."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _cabi.MisegError("miseg_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_LIB_FORK = True         # False: torch.cuda.Stream.wait_stream (system-scope events)


def wait_stream(waiter: "torch.cuda.Stream", producer: "torch.cuda.Stream") -> None:
    """``waiter.wait_stream(producer)`` through the library's device-scope-release events (``miseg_stream_wait_stream``): a torch event
    releases to system scope, which costs the PRODUCING stream ~5 us before its next kernel (scratch/fork_cost.py: 90.6 -> 88.2 us per
    kernel pair with a fork in between, 85.4 without) -- 22 weight-gradient forks per backward pass.  Under stream capture the torch
    call stays (the capture has to see the dependency)."""
    if waiter == producer:
        return
    if not _LIB_FORK or torch.cuda.is_current_stream_capturing():
        waiter.wait_stream(producer)
        return
    call("miseg_stream_wait_stream", waiter.cuda_stream, producer.cuda_stream)


def fill_zero(t: Tensor) -> Tensor:
    """``t.zero_()`` as a library launch (dense tensors; it is on the launch tape)."""
    assert t.is_cuda and (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last))
    call("miseg_fill_zero", _stream(), t.data_ptr(), t.numel() * t.element_size())
    return t


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_CONST_CACHE = {}


def cached_const(key, build):
    """Small static device tensors (window lists, gather indices) are built once per (shape, device)."""
    t = _CONST_CACHE.get(key)
    if t is None:
        t = _CONST_CACHE[key] = build()
    return t


def windows_tensor(windows, device) -> Tensor:
    key = ("win", str(device), tuple(tuple(int(v) for v in w) for w in windows))
    return cached_const(key, lambda: torch.tensor([list(w) for w in windows], dtype=torch.int32, device=device).view(len(windows), 4))


def arange_i32(start: int, stop: int, device) -> Tensor:
    """Cached int32 [start, stop) on the device; carries its bounds on the host (``_miseg_range``) so that a consumer that
    scatters into rows ``src`` (local_head's backward) knows which rows it will NOT write without reading the tensor back."""
    def build():
        t = torch.arange(start, stop, dtype=torch.int32, device=device)
        t._miseg_range = (int(start), int(stop))
        return t
    return cached_const(("arange", str(device), start, stop), build)


def flip_masks(decisions: Sequence[Sequence[bool]]) -> List[int]:
    """[[flip_h, flip_w], ...] -> bit masks (bit0 = H, bit1 = W), still on the host."""
    return [int(bool(fh)) | (int(bool(fw)) << 1) for fh, fw in decisions]


def flips_to_tensor(decisions: Sequence[Sequence[bool]], device) -> Tensor:
    """[[flip_h, flip_w], ...] -> int32 bit masks (bit0 = H, bit1 = W)."""
    return torch.tensor(flip_masks(decisions), dtype=torch.int32, device=device)


def as_nhwc(t: Tensor) -> Tensor:
    """[N,C,H,W]-shaped tensor whose memory is NHWC (channels_last); converts if needed."""
    if t.dim() != 4:
        raise ValueError(f"expected NCHW-shaped tensor, got {tuple(t.shape)}")
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def empty_nhwc(n, c, h, w, dtype, device) -> Tensor:
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)


def zeros_nhwc(n, c, h, w, dtype, device) -> Tensor:
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last).zero_()


def logits_nhwc(t: Tensor) -> Tensor:
    """fp32 NHWC logits for the pixel-wise kernels: read in place when they are that already, converted otherwise."""
    t = as_nhwc(t)
    return t if t.dtype == torch.float32 else t.float()


class PinnedRing:
    """``slots`` pinned host buffers of one shape used round-robin as the source of non-blocking host->device copies.  Every slot
    remembers an event recorded behind its last copy and waits for it before the slot is rewritten: free while the host is fewer than
    ``slots`` copies ahead of the copy engine, and a loop WITHOUT a per-iteration host synchronisation (a user loop, `bench.py
    --workload input`) can no longer overwrite a slot whose copy is still queued."""

    def __init__(self, shape, dtype, slots: int = 4):
        self.host = torch.empty((slots,) + tuple(shape), dtype=dtype).pin_memory()
        self.events = [None] * slots
        self.turn = 0

    def _send(self, fill, make_dst) -> Tensor:
        """Take the next slot, wait for its last copy, ``fill(slot)``, enqueue the copy into ``make_dst(slot)`` on the current stream
        and record the slot's event behind it."""
        self.turn = (self.turn + 1) % len(self.events)
        ev = self.events[self.turn]
        if ev is not None:
            ev.synchronize()
        slot = self.host[self.turn]
        fill(slot)
        dst = make_dst(slot)
        dst.copy_(slot, non_blocking=True)
        ev = self.events[self.turn] = ev or torch.cuda.Event()
        ev.record()
        return dst

    def upload(self, fill, device) -> Tensor:
        """``fill(host_slot)`` writes the payload; returns a fresh device tensor holding it (copy enqueued on the current stream)."""
        return self._send(fill, lambda slot: torch.empty(slot.shape, dtype=slot.dtype, device=device))

    def upload_into(self, fill, dst: Tensor) -> None:
        """The same into an existing device tensor (static buffers of a captured step)."""
        self._send(fill, lambda slot: dst)


class _GradJoin:
    """Hand-over of an input gradient between two consumers of ONE feature map, so that autograd has nothing to add.

    The last decoder block's output feeds DeConv_1x1 (the logits) and the local-MI head.  Autograd would add their two 100 MB input
    gradients with an elementwise kernel on the step's critical path (right after the IIC chain; 45 us alone, up to 150 us beside
    the next tap's backward).  Instead the consumer whose backward runs first (``conv1x1``: it has its gradient as soon as the
    supervised / consistency losses are differentiated) ``offer``s the tensor it wrote; the head's backward ``take``s it, makes its
    stream wait for the writer, ACCUMULATES into it in its kernel epilogue (``miseg_head_local_bwd_acc``), makes the writer's
    stream wait for that kernel, and returns no gradient of its own.  No offer (another tap, another order, an unsupported shape):
    the head returns its gradient as before.  The protocol is symmetric -- whoever runs first returns its tensor to autograd AND
    offers it, whoever runs second and can accumulate takes it and returns None: at the 32-channel tap the head runs first and
    ``up_conv``'s pooled data gradient (``miseg_conv3x3_fwd_sumpool_acc``) is the one that adds.

    OFF unless ``MISEG_GRAD_JOIN=1``: once the per-step host synchronisation was gone and same-box repeats agreed to 0.02 ms, three
    alternations read 7.32 / 7.30 / 7.33 ms without, 7.34 / 7.34 / 7.36 with the join at the 16-channel tap only, 7.44 / 7.43 / 7.44 at the
    32-channel tap only, 7.41 with both -- the cross-stream waits the hand-over adds cost more than the add kernels it removes."""
    enabled = os.environ.get("MISEG_GRAD_JOIN", "0") == "1"
    only = os.environ.get("MISEG_GRAD_JOIN_ONLY", "")      # "16" / "32": join at taps of that width only (the measurements below)
    _offers: dict = {}

    @classmethod
    def clear(cls) -> None:
        cls._offers.clear()

    @classmethod
    def offer(cls, feature: Tensor, grad: Tensor) -> None:
        """Only inside a backward pass; the offers die with it (a storage address may be another tensor's in the next pass)."""
        if cls.enabled and feature.is_cuda and grad.shape == feature.shape and grad.dtype == feature.dtype:
            if not cls._offers:
                try:
                    torch.autograd.Variable._execution_engine.queue_callback(cls.clear)
                except RuntimeError:      # not called from a backward pass: no hand-over
                    return
            ev = torch.cuda.Event()
            ev.record()
            cls._offers[(feature.data_ptr(), tuple(feature.shape))] = (grad, ev, torch.cuda.current_stream(feature.device))

    @classmethod
    def take(cls, feature: Tensor):
        return cls._offers.pop((feature.data_ptr(), tuple(feature.shape)), None) if cls.enabled else None
