"""Record / replay harness on the library's launch tape (csrc/tape.hip), by the rules ``miseg_amd.tape.StepTape._record`` follows.

``record(fn)`` runs ``fn()`` eagerly while the library records its own calls: every allocation of that run (all threads) comes
from a private ``torch.cuda.MemPool``, an ATen watch (``miseg_amd.tape.ForeignOps``) notes device work the library did not see,
and the tape is sealed whatever ``fn`` does.  The ``Recording`` keeps the pool and whatever ``fn`` returned referenced until
``close()`` has freed the tape: a replay writes to the recorded addresses, so nothing a recorded call points at may go back
to the general allocator while the tape can still run.

``assert_replay_equals_eager(case)`` is the per-call check: eager results, then poisoned outputs and restored state, then a
replay, bit for bit.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence

import torch
from torch import Tensor

from miseg_amd import _cabi
from miseg_amd.tape import ForeignOps

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def last_error() -> str:
    msg = _cabi.lib().miseg_last_error()
    return msg.decode() if msg else ""


def nbytes(t: Tensor) -> int:
    return t.numel() * t.element_size()


def bits(t: Tensor) -> Tensor:
    """The tensor's elements as integers of the same width (NaNs compare, -0.0 differs from 0.0)."""
    return t.view(_INT_VIEW[t.element_size()]) if t.dtype != torch.bool else t.view(torch.uint8)


def poison(t: Tensor) -> None:
    """Every byte of the tensor's elements 0xFF."""
    v = bits(t)
    v.fill_(255 if v.dtype == torch.uint8 else -1)


class Recording:
    """A sealed tape with what keeps its pointers valid.  Use as a context manager, or call ``close()``."""

    def __init__(self, handle: int, pool, seen: List[str], result: Any, keep: list):
        self.handle, self.pool, self.seen, self.result, self.keep = handle, pool, seen, result, keep
        self.slots: List[str] = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self) -> None:
        """Drain the device, free the tape, and only then let go of the pool and the tensors."""
        if self.handle:
            try:
                torch.cuda.synchronize()
            finally:
                _cabi.lib().miseg_tape_free(self.handle)
                self.handle = 0
        self.result, self.keep, self.pool = None, [], None

    def __len__(self) -> int:
        return int(_cabi.lib().miseg_tape_len(self.handle))

    def names(self) -> List[str]:
        lib = _cabi.lib()
        return [lib.miseg_tape_op_name(self.handle, i).decode() for i in range(len(self))]

    def segments(self) -> int:
        return int(_cabi.lib().miseg_tape_segments(self.handle))

    def bind(self, base: int, span: int) -> int:
        slot = int(_cabi.lib().miseg_tape_bind(self.handle, base, span))
        if slot < 0:
            raise _cabi.MisegError(f"miseg_tape_bind failed ({slot}): {last_error()}")
        return slot

    def bind_tensor(self, t: Tensor) -> int:
        return self.bind(t.data_ptr(), nbytes(t))

    def uses(self, slot: int) -> int:
        return int(_cabi.lib().miseg_tape_bind_uses(self.handle, slot))

    def replay_status(self, values: Sequence[Optional[int]] = (), segment: int = 0) -> int:
        arr = (ctypes.c_void_p * max(len(values), 1))(*values)
        return int(_cabi.lib().miseg_tape_replay(self.handle, segment, arr, len(values)))

    def replay(self, values: Sequence[Optional[int]] = ()) -> None:
        """All segments, in order; the bindings' values are applied by segment 0."""
        for seg in range(self.segments()):
            rc = self.replay_status(values, seg)
            if rc != 0:
                raise _cabi.MisegError(f"miseg_tape_replay failed ({rc}): {last_error()}")


def record(fn: Callable[[], Any], keep: Sequence[Any] = ()) -> Recording:
    """Run ``fn()`` with the library recording.  Raises what ``fn`` raises, after the tape has been ended and freed."""
    lib = _cabi.lib()
    idx = torch.cuda.current_device()
    pool = torch.cuda.MemPool()
    guard = ForeignOps()
    handle = int(lib.miseg_tape_begin())
    if not handle:
        raise _cabi.MisegError("miseg_tape_begin: another tape is being recorded")
    ok = False
    result = None
    try:
        torch._C._cuda_beginAllocateToPool(idx, pool.id)
        try:
            with guard:
                result = fn()
        finally:
            torch._C._cuda_endAllocateToPool(idx, pool.id)
            torch._C._cuda_releasePool(idx, pool.id)
        ok = lib.miseg_tape_end(handle) == 0
        if not ok:
            raise _cabi.MisegError(f"miseg_tape_end failed: {last_error()}")
    finally:
        if not ok:
            torch.cuda.synchronize()
            lib.miseg_tape_free(handle)      # (also stops the recording if it was never ended)
    return Recording(handle, pool, list(guard.seen), result, list(keep))


@dataclass
class Case:
    """One taped call (or a short chain of them) with everything it points at.

    ``call(T)`` issues the library calls on the tensors of ``T`` (inputs, inout and outputs under their names) and may return a
    dict of further outputs that it allocated itself.  ``inout`` is state the call updates in place or needs zeroed on entry;
    it is restored before the replay.  ``rebind`` names the input a trainer would bind, ``alt`` is a second tensor for it."""
    call: Callable[[Dict[str, Tensor]], Optional[Dict[str, Tensor]]]
    inputs: Dict[str, Tensor] = field(default_factory=dict)
    inout: Dict[str, Tensor] = field(default_factory=dict)
    outputs: Dict[str, Tensor] = field(default_factory=dict)
    rebind: Optional[str] = None
    alt: Optional[Tensor] = None
    order_dependent: bool = False
    reason: str = ""
    close: Optional[Callable[[str, Tensor, Tensor], None]] = None     # order-dependent cases: raises if got is too far from want
    loose: Sequence[str] = ()                                          # ... the tensors it applies to; every other one stays bit-compared
    expect: Sequence[str] = ()                                         # op names that must be on the tape

    def tensors(self) -> Dict[str, Tensor]:
        return {**self.inputs, **self.inout, **self.outputs}


class ReplayMismatch(AssertionError):
    pass


def _compare(case: Case, want: Dict[str, Tensor], got: Dict[str, Tensor], what: str, exact: bool = False) -> None:
    assert set(want) == set(got), (what, sorted(want), sorted(got))
    for k in sorted(want):
        w, g = want[k], got[k]
        if w.shape != g.shape or w.dtype != g.dtype:
            raise ReplayMismatch(f"{what}: {k} is {tuple(g.shape)} {g.dtype}, eager gave {tuple(w.shape)} {w.dtype}")
        if case.order_dependent and not exact and k in case.loose:
            case.close(k, w, g)
        elif not torch.equal(bits(w), bits(g)):
            n = int((bits(w) != bits(g)).sum())
            raise ReplayMismatch(f"{what}: {k} differs from the eager result in {n} of {w.numel()} elements")


def _reset(case: Case, snap: Dict[str, Tensor], outs: Dict[str, Tensor]) -> None:
    for k, t in case.inout.items():
        t.copy_(snap[k])
    for t in outs.values():
        poison(t)


def assert_replay_equals_eager(case: Case, replayer: Optional[Callable[[Recording], None]] = None) -> List[str]:
    """Snapshot, run eagerly while recording, poison, replay, compare bit for bit; then the same with ``rebind`` re-based.
    Returns the op names of the tape.  ``replayer`` replaces the replay (the harness's own test replays nothing)."""
    if case.order_dependent:
        assert case.reason and case.close is not None and case.loose, "an order-dependent case states its reason, its bound and the tensors it is for"
        assert not set(case.loose) - set(case.inout) - set(case.outputs), "the bound is for tensors the call writes"
    T = case.tensors()
    snap_in = {k: t.clone() for k, t in case.inputs.items()}
    snap = {k: t.clone() for k, t in case.inout.items()}
    torch.cuda.synchronize()
    with record(lambda: case.call(T), keep=[case]) as rec:
        torch.cuda.synchronize()
        if rec.seen:
            raise AssertionError(f"not tape-clean, device work outside the library: {sorted(set(rec.seen))}")
        names = rec.names()
        assert names, "the call recorded nothing"
        missing = sorted(set(case.expect) - set(names))
        assert not missing, f"expected on the tape, not recorded: {missing} (recorded {sorted(set(names))})"
        outs = {**case.outputs, **(rec.result or {})}
        assert outs or case.inout, "a case needs something to compare"
        state = {**case.inout, **outs}
        eager = {k: t.clone() for k, t in state.items()}
        _reset(case, snap, outs)
        torch.cuda.synchronize()
        (replayer or Recording.replay)(rec)
        torch.cuda.synchronize()
        _compare(case, eager, state, "replay")
        _compare(case, snap_in, case.inputs, "replay (inputs must be left alone)", exact=True)
        if case.rebind is not None:
            orig, alt = case.inputs[case.rebind], case.alt
            assert alt is not None and alt.shape == orig.shape and alt.dtype == orig.dtype and alt.stride() == orig.stride()
            assert not torch.equal(bits(alt), bits(orig)), "the second tensor must differ from the recorded one"
            alt_snap = alt.clone()
            slot = rec.bind_tensor(orig)
            assert rec.uses(slot) >= 1, f"{case.rebind} is not a pointer argument of any recorded call"
            _reset(case, snap, outs)
            poison(orig)                        # a replay that still read the recorded tensor would show
            torch.cuda.synchronize()
            rec.replay([alt.data_ptr()])
            torch.cuda.synchronize()
            rebound = {k: t.clone() for k, t in state.items()}
            assert torch.equal(bits(alt), bits(alt_snap)), "replay wrote the re-bound input"
            orig.copy_(snap_in[case.rebind])
            # the plain, unrecorded eager call on the second tensor (into the same buffers: the tape is not replayed again)
            _reset(case, snap, outs)
            T2 = dict(T)
            T2[case.rebind] = alt
            res2 = case.call(T2)
            torch.cuda.synchronize()
            plain = {**case.inout, **case.outputs, **(res2 or {})}
            _compare(case, {k: plain[k] for k in rebound}, rebound, f"replay with {case.rebind} re-bound")
    return names
