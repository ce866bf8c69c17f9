"""Data-parallel gradient reduction: one process per GPU, RCCL over xGMI (torch.distributed backend "nccl").

The reference has no distributed code at all; this is the MI355X-native addition the
north star asks for.  Semantics: every rank draws its own labeled/unlabeled minibatch and runs
the full step locally -- BatchNorm statistics and the K x K joints stay per-rank, exactly what the reference
computes for one process with that batch -- then the gradients of all parameters are mean-all-reduced before
``Adam.step``.

Design for point-to-point xGMI rather than NVSwitch: the whole gradient is only 8.76 MB (2.19 M fp32), so ring
all-reduce is latency-bound, not bandwidth-bound.  Gradients live in ONE flat buffer (``miseg_amd.flat``), cut
into a few large contiguous buckets ordered by reverse execution (heads + decoder first).  A bucket's
all-reduce is issued asynchronously from the autograd hook of its last-arriving parameter, so it overlaps the
rest of the backward pass on RCCL's own stream; ``finish()`` waits, and averages.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.distributed as dist

from . import unet_ops
from ._rt import wait_stream
from .flat import FlatBuffers
from .tape import host_call


def init_from_env(backend: Optional[str] = None) -> bool:
    """Initialise torch.distributed from RANK / WORLD_SIZE / MASTER_* (torchrun); returns True if world_size > 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1 and os.environ.get("MISEG_FORCE_DDP", "0") != "1":  # FORCE: exercise the RCCL path with one rank
        return False
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29511")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    if not dist.is_initialized():
        backend = os.environ.get("MISEG_DDP_BACKEND") or backend     # e.g. gloo: several ranks on ONE GPU (tests), or CPU tensors
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(backend=backend)
    return True


class GradReducer:
    def __init__(self, flat: FlatBuffers, num_buckets: int = 3, process_group=None, broadcast_params: bool = True):
        assert dist.is_initialized(), "call ddp.init_from_env() first"
        self.flat = flat
        self.group = process_group
        self.world = dist.get_world_size(process_group)
        flat.ensure()
        self._avg_native = dist.get_backend(process_group) == "nccl"
        # contiguous buckets over the flat buffer, cut at parameter boundaries; bucket 0 = tail (ready first)
        n = len(flat.params)
        target = flat.total / float(num_buckets)
        bounds, acc = [n], 0.0
        for i in range(n - 1, -1, -1):
            acc += (flat.offsets[i + 1] if i + 1 < n else flat.total) - flat.offsets[i]
            if acc >= target and len(bounds) < num_buckets and i > 0:
                bounds.append(i)
                acc = 0.0
        bounds.append(0)
        self.buckets = []  # (first_param, last_param_exclusive, start, end)
        for hi, lo in zip(bounds[:-1], bounds[1:]):
            if lo < hi:
                end = flat.offsets[hi] if hi < n else flat.total
                self.buckets.append((lo, hi, flat.offsets[lo], end))
        self._bucket_of = [0] * n
        for b, (lo, hi, _, _) in enumerate(self.buckets):
            for i in range(lo, hi):
                self._bucket_of[i] = b
        self._pending: List[int] = []
        self.producer_streams: list = []   # extra streams that write gradients (see semi_seg.epocher IIC side stream)
        self._handles: List[Optional[object]] = []
        self._armed = False
        self.timing = False                 # bench.py: record an event pair around finish()'s waits
        self._wait_events: list = []
        # Gradient hooks.  The first armed backward pass runs one Python hook per parameter (~125) and learns which parameter of each
        # bucket gets its gradient LAST; from then on only those trigger parameters keep a hook (one per bucket instead of ~40: the hooks
        # alone cost a one-rank run 0.2-0.3 ms of host time per step on the thread that issues the backward launches).  A trigger that
        # fires while another parameter of its bucket has no gradient yet (the order changed) launches nothing; finish() flushes.
        self._last_in_bucket: List[Optional[int]] = [None] * len(self.buckets)
        self._triggers_only = False
        self._hook_handles = [p.register_post_accumulate_grad_hook(self._make_hook(i)) for i, p in enumerate(flat.params)]
        if broadcast_params:
            dist.broadcast(flat.flat_param, src=0, group=process_group)

    def _make_hook(self, index: int):
        def hook(_param):
            if not self._armed:
                return
            b = self._bucket_of[index]
            if self._triggers_only:
                lo, hi, _, _ = self.buckets[b]
                if self._handles[b] is None and all(p.grad is not None for p in self.flat.params[lo:hi]):
                    self._launch(b)
                return
            self._last_in_bucket[b] = index
            self._pending[b] -= 1
            if self._pending[b] == 0:
                self._launch(b)
        return hook

    def _keep_trigger_hooks(self) -> None:
        keep = set(i for i in self._last_in_bucket if i is not None)
        if len(keep) != len(self.buckets):
            return                  # some bucket saw no gradient at all in the learning pass: keep every hook
        for i, h in enumerate(self._hook_handles):
            if i not in keep:
                h.remove()
        self._triggers_only = True

    def _launch(self, b: int) -> None:
        lo, hi, start, end = self.buckets[b]
        op = dist.ReduceOp.AVG if self._avg_native else dist.ReduceOp.SUM
        if not self.flat.flat_grad.is_cuda:
            self.flat.collect(lo, hi)
            self._handles[b] = dist.all_reduce(self.flat.flat_grad[start:end], op=op, group=self.group, async_op=True)
            return
        # A bucket mixes gradients written on different HIP streams: the stream this hook runs on (BatchNorm / head parameters), the
        # weight-gradient stream, the IIC branch.  The collective is launched from the WEIGHT-GRADIENT stream, made to wait for the
        # others: the backward pass's own stream never waits for the weight gradients to drain in the middle of the pass, and no further
        # stream is created -- with RCCL's own that makes four, the number of hardware queues a process gets by default
        # (GPU_MAX_HW_QUEUES); a fifth stream shares a queue with one of the others and the step time became bimodal (6.95 / 7.4 ms).
        dev = self.flat.flat_grad.device
        cur = torch.cuda.current_stream(dev)
        rs = unet_ops.wgrad_stream(dev)
        for s in [cur] + [s for s in self.producer_streams if s != cur and s != rs]:
            wait_stream(rs, s)
        torch.cuda.set_stream(rs)       # (not the `with torch.cuda.stream` context: 15-20 us of host time per use)
        try:
            self.flat.collect(lo, hi)   # joins the weight-gradient stream into rs; gradients autograd parked elsewhere -> flat slice
        finally:
            torch.cuda.set_stream(cur)

        def allreduce():                # host call: under a launch tape it is repeated between two segments of every replay, from
            back = torch.cuda.current_stream(dev)      # the caller's thread -- so it sets (and restores) its own stream
            torch.cuda.set_stream(rs)
            try:
                self._handles[b] = dist.all_reduce(self.flat.flat_grad[start:end], op=op, group=self.group, async_op=True)
            finally:
                torch.cuda.set_stream(back)
        host_call(allreduce)

    def prepare(self) -> None:
        """Call after zero_grad(), before backward()."""
        self.flat.ensure()
        self._pending = [hi - lo for lo, hi, _, _ in self.buckets]
        self._handles = [None] * len(self.buckets)
        if self._triggers_only and any(p.grad is not None for p in self.flat.params):
            # trigger-only mode decides "bucket complete" from `grad is not None`: a gradient left over from an earlier pass (gradient
            # accumulation, a zero_grad that keeps the tensors) would let a trigger reduce a half-written bucket -> count arrivals again
            for h in self._hook_handles:
                h.remove()
            self._hook_handles = [p.register_post_accumulate_grad_hook(self._make_hook(i)) for i, p in enumerate(self.flat.params)]
            self._triggers_only = False
            self._stale_grads = True
        self._armed = True

    def finish(self) -> None:
        """Call after backward(), before optimizer.step(): flush unlaunched buckets, wait, average."""
        self._armed = False
        if not self._triggers_only and not getattr(self, "_stale_grads", False):
            self._keep_trigger_hooks()
        for b in range(len(self.buckets)):
            if self._handles[b] is None:  # some parameter of the bucket got no gradient this step (or its trigger fired early)
                self._launch(b)
        if self.flat.flat_grad.is_cuda:
            host_call(self._wait_all)     # (a replayed launch tape repeats it at this point of the iteration)
        else:
            self._wait_all()

    def _wait_all(self) -> None:
        timed = self.timing and self.flat.flat_grad.is_cuda
        if timed:       # from "this stream has nothing left but to wait for the collectives" to "they are done": the EXPOSED part
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for h in self._handles:
            h.wait()
        if timed:
            e1.record()
            self._wait_events.append((e0, e1))
        if not self._avg_native:
            self.flat.flat_grad.div_(self.world)

    def exposed_ms(self) -> Optional[float]:
        """Mean device time per step the gradient stream spent waiting for its all-reduces after the backward pass had finished
        (``timing`` must have been on; synchronises)."""
        if not self._wait_events:
            return None
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self._wait_events]
        self._wait_events = []
        return sum(ms) / len(ms)


def attach(trainer, num_buckets: int = 3) -> Optional[GradReducer]:
    """Give a SemiTrainer (after ``init()`` and after its parameters are on their device) a GradReducer."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return None
    optimizer = trainer._optimizer
    if not hasattr(optimizer, "flat"):
        raise RuntimeError("data-parallel training needs a flat-buffer fused optimiser (Optim.name: Adam, RAdam, AdaBound or AdaBoundW)")
    trainer.to(trainer._device)
    trainer._grad_reducer = GradReducer(optimizer.flat, num_buckets=num_buckets)
    teacher, updater = getattr(trainer, "_teacher_model", None), getattr(trainer, "_ema_updater", None)
    if teacher is not None and updater is not None:
        # Mean Teacher: rank 0's teacher everywhere (its flat mirror of the student's buffer: one broadcast).  The student is identical
        # on every rank after each all-reduce, so the EMA keeps the teachers identical with no communication; the teacher's BatchNorm
        # buffers stay rank-local like the student's.
        dist.broadcast(updater.flats(teacher, optimizer.flat).flat_param, src=0)
    return trainer._grad_reducer
