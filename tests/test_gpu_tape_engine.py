"""The launch tape's own contract (csrc/tape.h, csrc/tape.hip; header section "Launch tape"), on the C ABI.

The ops are the byte movers -- ``miseg_fill_zero``, ``miseg_copy``, ``miseg_axpy`` -- on buffers of a few KB: their effect is
checked exactly, and every buffer carries sentinels around and inside what an op may write.  All buffers are allocated before a
tape records and are held until it has been freed.  The one refused op on a tape is an ARGUMENT refusal (a misaligned pointer,
refused before any launch); nothing here launches a kernel with wrong sizes or pointers.
"""
import contextlib
import ctypes
import math
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 256                      # floats an op moves (1 KB)
GUARD = 64                   # sentinel floats on either side


def _lib():
    from miseg_amd import _cabi
    return _cabi.lib()


def _H():
    import tape_harness
    return tape_harness


def _st():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """N floats between two guards; ``mid`` is what ops may touch."""

    def __init__(self, seed: int, n: int = N):
        g = torch.Generator().manual_seed(seed)
        self.n = n
        self.init = (torch.randint(1, 1000, (n + 2 * GUARD,), generator=g).float() + seed * 1000).to(DEV)
        self.t = self.init.clone()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + GUARD * 4

    @property
    def mid(self):
        return self.t[GUARD:GUARD + self.n]

    @property
    def mid0(self):
        return self.init[GUARD:GUARD + self.n]

    def reset(self):
        self.t.copy_(self.init)

    def guards_intact(self) -> bool:
        return torch.equal(self.t[:GUARD], self.init[:GUARD]) and torch.equal(self.t[GUARD + self.n:], self.init[GUARD + self.n:])

    def untouched(self) -> bool:
        return torch.equal(self.t, self.init)


def fill_zero(b: Buf, off: int = 0, n: int = None) -> int:
    return _lib().miseg_fill_zero(_st(), b.ptr + off * 4, (b.n - off if n is None else n) * 4)


def copy(dst: Buf, src: Buf, off: int = 0, n: int = None, dst_shift: int = 0) -> int:
    return _lib().miseg_copy(_st(), dst.ptr + off * 4 + dst_shift, src.ptr + off * 4, (src.n - off if n is None else n) * 4)


def axpy(dst: Buf, src: Buf) -> int:
    return _lib().miseg_axpy(_st(), 0, src.ptr, dst.ptr, src.n)


@contextlib.contextmanager
def recording():
    """A tape that records now; freed (which also stops the recording) whatever the test does."""
    lib = _lib()
    h = lib.miseg_tape_begin()
    assert h, "another tape is being recorded"
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        lib.miseg_tape_free(h)


def sealed(h) -> int:
    assert _lib().miseg_tape_end(h) == 0
    return h


def names(h):
    lib = _lib()
    return [lib.miseg_tape_op_name(h, i).decode() for i in range(lib.miseg_tape_len(h))]


def values(*ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs), len(ptrs)


def replay(h, *ptrs, segment: int = 0) -> int:
    arr, n = values(*ptrs)
    return _lib().miseg_tape_replay(h, segment, arr, n)


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- handles
def test_second_begin_while_recording_returns_zero():
    lib = _lib()
    with recording() as h:
        assert lib.miseg_tape_begin() == 0
        a = Buf(1)
        assert fill_zero(a) == 0
        assert lib.miseg_tape_len(h) == 1            # ... and the first tape still records


def test_end_with_a_foreign_or_zero_handle_fails_and_recording_continues():
    lib = _lib()
    a = Buf(1)
    with recording() as h:
        sealed(h)
        with recording() as h2:
            assert lib.miseg_tape_end(h) != 0        # a sealed tape that is not the one recording
            assert lib.miseg_tape_end(0) != 0
            assert b"not the one being recorded" in lib.miseg_last_error()
            assert fill_zero(a) == 0
            assert lib.miseg_tape_len(h2) == 1 and lib.miseg_tape_len(h) == 0
            assert lib.miseg_tape_end(h2) == 0


def test_free_of_zero_is_ok_and_null_handles_answer_minus_one():
    lib = _lib()
    assert lib.miseg_tape_free(0) == 0
    assert lib.miseg_tape_mark(0) == -1 and lib.miseg_tape_len(0) == -1 and lib.miseg_tape_segments(0) == -1
    assert lib.miseg_tape_bind_uses(0, 0) == -1 and lib.miseg_tape_op_stream(0, 0) == -1
    assert lib.miseg_tape_op_name(0, 0) == b""
    assert lib.miseg_tape_timed_ms(0, 0, (ctypes.c_float * 1)(), 1) == -1
    assert replay(0) != 0 and lib.miseg_tape_time_op(0, 0) != 0 and lib.miseg_tape_bind(0, 16, 16) < 0


def test_freeing_the_recording_tape_stops_recording():
    lib = _lib()
    a = Buf(1)
    h = lib.miseg_tape_begin()
    assert h
    assert lib.miseg_tape_free(h) == 0
    assert fill_zero(a) == 0                         # lands on no tape (there is none), and still executes
    sync()
    assert float(a.mid.abs().sum()) == 0.0 and a.guards_intact()
    with recording() as h2:                          # a new begin succeeds
        assert lib.miseg_tape_len(h2) == 0


def test_recording_does_not_suppress_execution():
    a, b = Buf(1), Buf(2)
    with recording() as h:
        assert copy(b, a) == 0 and axpy(b, a) == 0
        sync()
        assert torch.equal(b.mid, a.mid0 + a.mid0) and b.guards_intact() and a.untouched()
        assert names(h) == ["miseg_copy", "miseg_axpy"]


# ---------------------------------------------------------------------------------------------------------------- outermost call only
def test_entry_points_that_forward_to_others_record_once():
    """The fp32 `_heads` forms loop over the per-head entry points (csrc/mi_local.hip): one op each, under the outer name, on the
    stream passed in; and the replay of that one op reproduces all S sub-heads."""
    from miseg_amd import _cabi
    H = _H()
    s, ub, k, h, w, pad, P = 3, 1, 5, 12, 10, 2, 1
    t = 2 * pad + 1
    g = torch.Generator().manual_seed(3)
    probs = torch.softmax(torch.randn(s, 2 * ub, k, h, w, generator=g), 2).to(DEV)
    win = torch.tensor([[0, h, 0, w]], dtype=torch.int32, device=DEV)
    raw = torch.empty(s, P, t, t, k, k, device=DEV)
    graw = torch.randn(s, P, t, t, k, k, generator=g).to(DEV)
    scale = (torch.rand(s, P, generator=g) + 0.5).to(DEV)
    gprob = torch.empty_like(probs)
    jws = torch.empty(max(_cabi.query("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, P * s), _cabi.query("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, P)),
                      dtype=torch.uint8, device=DEV)
    bws = torch.empty(_cabi.query("miseg_iic_local_bwd_ws_bytes", k, pad, P * s), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def run():
        st = side.cuda_stream
        _cabi.call("miseg_iic_local_joint_fwd_heads", st, probs.data_ptr(), s, ub, k, h, w, pad, win.data_ptr(), P, raw.data_ptr(), jws.data_ptr(), jws.numel(), 0)
        _cabi.call("miseg_iic_local_bwd_heads", st, probs.data_ptr(), s, ub, k, h, w, pad, win.data_ptr(), P, graw.data_ptr(), scale.data_ptr(), gprob.data_ptr(),
                   0, 0, bws.data_ptr(), bws.numel())

    with H.record(run, keep=[probs, win, raw, graw, scale, gprob, jws, bws, side]) as rec:
        sync()
        assert rec.names() == ["miseg_iic_local_joint_fwd_heads", "miseg_iic_local_bwd_heads"]
        lib = _lib()
        assert lib.miseg_tape_op_stream(rec.handle, 0) == side.cuda_stream and lib.miseg_tape_op_stream(rec.handle, 1) == side.cuda_stream
        assert side.cuda_stream != _st()
        eager_raw, eager_g = raw.clone(), gprob.clone()
        assert float(eager_raw[s - 1].abs().sum()) > 0 and float(eager_g[s - 1].abs().sum()) > 0       # the last sub-head ran too
        H.poison(raw)
        H.poison(gprob)
        sync()
        rec.replay()
        sync()
        assert torch.equal(H.bits(raw), H.bits(eager_raw))
        assert torch.equal(H.bits(gprob), H.bits(eager_g))          # K = 5: plain read-modify-write col2im, no float atomics


# ---------------------------------------------------------------------------------------------------------------- threads
def test_calls_from_a_second_thread_are_recorded_in_call_order():
    a, b, c = Buf(1), Buf(2), Buf(3)
    st = _st()
    rcs = []

    def other():
        torch.cuda.set_device(0)
        lib = _lib()
        rcs.append(lib.miseg_copy(st, b.ptr, a.ptr, N * 4))
        rcs.append(lib.miseg_axpy(st, 0, a.ptr, b.ptr, N))

    with recording() as h:
        assert fill_zero(c) == 0
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert fill_zero(a, off=N // 2) == 0
        assert rcs == [0, 0]
        assert names(h) == ["miseg_fill_zero", "miseg_copy", "miseg_axpy", "miseg_fill_zero"]
        sealed(h)
        sync()
        want_b = a.mid0 * 2
        assert torch.equal(b.mid, want_b)
        for x in (a, b, c):
            x.reset()
        assert replay(h) == 0
        sync()
        assert torch.equal(b.mid, want_b) and float(c.mid.abs().sum()) == 0.0
        assert torch.equal(a.mid[:N // 2], a.mid0[:N // 2]) and float(a.mid[N // 2:].abs().sum()) == 0.0
        assert a.guards_intact() and b.guards_intact() and c.guards_intact()


def test_a_replay_while_another_tape_records_appends_nothing():
    lib = _lib()
    a, b, c = Buf(1), Buf(2), Buf(3)
    with recording() as ha:
        assert copy(b, a) == 0
        sealed(ha)
        with recording() as hb:
            assert replay(ha) == 0                               # on the recording thread
            rcs = []
            th = threading.Thread(target=lambda: (torch.cuda.set_device(0), rcs.append(replay(ha))))
            th.start()
            th.join()
            assert rcs == [0]
            assert lib.miseg_tape_len(hb) == 0
            assert fill_zero(c) == 0                             # a direct call afterwards is appended
            assert names(hb) == ["miseg_fill_zero"]
            assert lib.miseg_tape_len(ha) == 1
            sync()


# ---------------------------------------------------------------------------------------------------------------- bind
def test_bind_needs_a_sealed_tape_and_bad_slots_answer_minus_one():
    lib = _lib()
    a = Buf(1)
    with recording() as h:
        assert fill_zero(a) == 0
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) < 0
        assert b"still being recorded" in lib.miseg_last_error()
        sealed(h)
        assert lib.miseg_tape_bind_uses(h, 0) == -1              # no slot yet
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) == 0
        assert lib.miseg_tape_bind_uses(h, 0) == 1
        assert lib.miseg_tape_bind_uses(h, 1) == -1 and lib.miseg_tape_bind_uses(h, -1) == -1


def test_slots_count_up_and_bind_uses_counts_matches():
    lib = _lib()
    a, b, c, unused = Buf(1), Buf(2), Buf(3), Buf(4)
    with recording() as h:
        assert copy(b, a) == 0 and axpy(b, a) == 0 and fill_zero(c) == 0
        sealed(h)
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) == 0
        assert lib.miseg_tape_bind(h, unused.ptr, N * 4) == 1    # matches nothing: still a slot
        assert lib.miseg_tape_bind(h, b.ptr, N * 4) == 2
        assert lib.miseg_tape_bind(h, c.ptr, N * 4) == 3
        assert [lib.miseg_tape_bind_uses(h, s) for s in range(4)] == [2, 0, 2, 1]
        # the value of a binding without uses is ignored, NULL included
        a2, b2, c2 = Buf(5), Buf(6), Buf(7)
        for x in (a, b, c):
            x.reset()
        assert replay(h, a2.ptr, None, b2.ptr, c2.ptr) == 0
        sync()
        assert torch.equal(b2.mid, a2.mid0 * 2) and float(c2.mid.abs().sum()) == 0.0
        assert a.untouched() and b.untouched() and c.untouched() and unused.untouched() and a2.untouched()
        assert b2.guards_intact() and c2.guards_intact()


def test_interior_pointers_keep_their_offset_and_the_span_is_half_open():
    lib = _lib()
    a, b = Buf(1), Buf(2)
    x, y = Buf(3), Buf(4)
    off = 64                                                     # floats: base + 256 bytes
    with recording() as h:
        assert copy(b, a, off=off, n=32) == 0                    # dst = b + 256, src = a + 256
        assert fill_zero(b, off=N - 4, n=4) == 0                 # dst = b + span - 16
        sealed(h)
        # a span that ends exactly at the interior pointer does not contain it; one byte more does
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr, off * 4)) == 0
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr, off * 4 + 1)) == 1
        s_b = lib.miseg_tape_bind(h, b.ptr, N * 4)
        assert lib.miseg_tape_bind_uses(h, s_b) == 2
        for t in (a, b):
            t.reset()
        assert replay(h, x.ptr, x.ptr, y.ptr) == 0
        sync()
        want = y.init.clone()
        want[GUARD + off:GUARD + off + 32] = x.mid0[off:off + 32]
        want[GUARD + N - 4:GUARD + N] = 0
        assert torch.equal(y.t, want)
        assert a.untouched() and b.untouched() and x.untouched()


def test_span_end_pointer_is_not_bound_and_a_span_below_one_behaves_as_one():
    lib = _lib()
    a, b, c = Buf(1), Buf(2), Buf(3)
    with recording() as h:
        assert fill_zero(a, off=0, n=4) == 0                     # pointer = a
        assert fill_zero(a, off=4, n=4) == 0                     # pointer = a + 16
        sealed(h)
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr, 16)) == 1        # base + span is outside
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr + 1, 16)) == 1    # base + span - 1 is inside
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr, 0)) == 1         # span <= 0: the base alone
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr + 16, -5)) == 1
        assert lib.miseg_tape_bind_uses(h, lib.miseg_tape_bind(h, a.ptr + 15, -5)) == 0
        a.reset()
        # later bindings win (they are applied in slot order): slot 2 re-bases the first op to b, slot 3 the second to c + 16
        assert replay(h, a.ptr, a.ptr + 1, b.ptr, c.ptr + 16, None) == 0
        sync()
        assert a.untouched()
        assert float(b.mid[:4].abs().sum()) == 0.0 and torch.equal(b.t[GUARD + 4:], b.init[GUARD + 4:]) and b.guards_intact()
        assert float(c.mid[4:8].abs().sum()) == 0.0 and torch.equal(c.mid[:4], c.mid0[:4]) and torch.equal(c.t[GUARD + 8:], c.init[GUARD + 8:])


# ---------------------------------------------------------------------------------------------------------------- replay arguments
def test_bad_replay_arguments_run_nothing():
    lib = _lib()
    a, b = Buf(1), Buf(2)
    with recording() as h:
        assert copy(b, a) == 0
        sync()
        b.reset()
        assert replay(h) != 0                                    # unsealed
        assert b"not a sealed tape" in lib.miseg_last_error()
        sealed(h)
        assert replay(h, segment=1) != 0 and replay(h, segment=-1) != 0
        assert b"segment" in lib.miseg_last_error()
        assert replay(h, a.ptr) != 0                             # one value, no binding
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) == 0
        assert replay(h) != 0 and replay(h, a.ptr, a.ptr) != 0   # none / two values, one binding
        assert b"values for 1 bindings" in lib.miseg_last_error()
        sync()
        assert b.untouched() and a.untouched()
        assert replay(h, a.ptr) == 0
        sync()
        assert torch.equal(b.mid, a.mid0)


# ---------------------------------------------------------------------------------------------------------------- segments
def test_marks_cut_segments_and_each_replays_its_own_ops():
    lib = _lib()
    a, b, c = Buf(1), Buf(2), Buf(3)
    with recording() as h:
        assert lib.miseg_tape_segments(h) == 1
        assert lib.miseg_tape_mark(h) == 1                       # at the start: segment 0 is empty
        assert copy(b, a) == 0
        assert lib.miseg_tape_mark(h) == 2
        assert lib.miseg_tape_mark(h) == 3                       # segment 2 is empty
        assert fill_zero(c) == 0 and axpy(b, a) == 0
        assert lib.miseg_tape_mark(h) == 4                       # at the end: segment 4 is empty
        sealed(h)
        assert lib.miseg_tape_mark(h) == -1                      # no mark after end
        assert lib.miseg_tape_segments(h) == 5 and lib.miseg_tape_len(h) == 3
        sync()
        for seg, check in ((0, lambda: b.untouched() and c.untouched()),
                           (1, lambda: torch.equal(b.mid, a.mid0) and c.untouched()),
                           (2, lambda: b.untouched() and c.untouched()),
                           (3, lambda: torch.equal(b.mid, b.mid0 + a.mid0) and float(c.mid.abs().sum()) == 0.0),
                           (4, lambda: b.untouched() and c.untouched())):
            for x in (a, b, c):
                x.reset()
            assert replay(h, segment=seg) == 0
            sync()
            assert check(), seg
            assert a.untouched() and b.guards_intact() and c.guards_intact()
        assert replay(h, segment=5) != 0


def test_values_are_applied_at_segment_zero_only():
    """Replaying segment 1 with other values does not re-base: it still writes where segment 0's values pointed."""
    lib = _lib()
    a, b = Buf(1), Buf(2)
    A, B = Buf(3), Buf(4)
    with recording() as h:
        assert fill_zero(a, n=8) == 0
        assert lib.miseg_tape_mark(h) == 1
        assert copy(a, b, off=16, n=8) == 0
        sealed(h)
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) == 0
        sync()
        a.reset()
        assert replay(h, A.ptr, segment=0) == 0
        assert replay(h, B.ptr, segment=1) == 0
        sync()
        want = A.init.clone()
        want[GUARD:GUARD + 8] = 0
        want[GUARD + 16:GUARD + 24] = b.mid0[16:24]
        assert torch.equal(A.t, want)
        assert B.untouched() and a.untouched() and b.untouched()


def test_rebasing_does_not_drift():
    lib = _lib()
    a, src = Buf(1), Buf(2)
    X, Y = Buf(3), Buf(4)
    off = 64
    with recording() as h:
        assert copy(a, src, off=off, n=16) == 0
        sealed(h)
        assert lib.miseg_tape_bind(h, a.ptr, N * 4) == 0
        sync()
        a.reset()
        for target in (X, Y, a, X):
            for t in (a, X, Y):
                t.reset()
            assert replay(h, target.ptr) == 0
            sync()
            want = target.init.clone()
            want[GUARD + off:GUARD + off + 16] = src.mid0[off:off + 16]
            assert torch.equal(target.t, want)
            assert all(t.untouched() for t in (a, X, Y) if t is not target) and src.untouched()


# ---------------------------------------------------------------------------------------------------------------- a refused op
def test_a_refused_op_is_recorded_and_fails_every_replay_at_that_op():
    """good, refused, good: the refused call (a destination that is not 16-byte aligned: refused before any launch) is on the
    tape like any other; a replay runs the ops before it, returns its status and names it, and runs nothing after it."""
    lib = _lib()
    a, b, c = Buf(1), Buf(2), Buf(3)
    with recording() as h:
        assert copy(b, a) == 0
        assert copy(c, a, dst_shift=4) == -1                     # MISEG_E_INVALID
        assert fill_zero(c) == 0
        sealed(h)
        assert names(h) == ["miseg_copy", "miseg_copy", "miseg_fill_zero"]
        sync()
        for _ in range(2):
            for x in (a, b, c):
                x.reset()
            assert replay(h) == -1
            msg = lib.miseg_last_error().decode()
            assert "op 1" in msg and "miseg_copy" in msg and "16-byte aligned" in msg, msg
            sync()
            assert torch.equal(b.mid, a.mid0) and b.guards_intact()
            assert c.untouched() and a.untouched()


# ---------------------------------------------------------------------------------------------------------------- timing
def test_time_op_and_timed_ms():
    """``miseg_tape_timed_ms`` hands out the oldest ``cap`` samples and DROPS the rest: the read empties the store whatever
    ``cap`` was, so the next read returns 0."""
    lib = _lib()
    a, b = Buf(1), Buf(2)
    buf = (ctypes.c_float * 8)(*([-1.0] * 8))
    with recording() as h:
        assert copy(b, a) == 0 and axpy(b, a) == 0
        sealed(h)
        assert lib.miseg_tape_time_op(h, 2) != 0 and lib.miseg_tape_time_op(h, -1) != 0
        assert lib.miseg_tape_time_op(h, 1) == 0 and lib.miseg_tape_time_op(h, 1) == 0           # idempotent
        assert lib.miseg_tape_timed_ms(h, 1, buf, 8) == 0                                        # no replay yet
        assert lib.miseg_tape_timed_ms(h, 0, buf, 8) == 0                                        # op 0 is not timed
        for _ in range(3):
            assert replay(h) == 0
        assert lib.miseg_tape_timed_ms(h, 1, buf, 8) == 3
        assert all(math.isfinite(buf[i]) and buf[i] >= 0.0 for i in range(3)) and buf[3] == -1.0
        assert lib.miseg_tape_timed_ms(h, 1, buf, 8) == 0
        for _ in range(3):
            assert replay(h) == 0
        small = (ctypes.c_float * 4)(*([-1.0] * 4))
        assert lib.miseg_tape_timed_ms(h, 1, small, 2) == 2
        assert small[0] >= 0.0 and small[1] >= 0.0 and small[2] == -1.0 and small[3] == -1.0
        assert lib.miseg_tape_timed_ms(h, 1, small, 4) == 0                                      # the third sample is gone
        assert replay(h) == 0
        assert lib.miseg_tape_timed_ms(h, 1, small, 4) == 1                                      # ... and timing goes on
        sync()


# ---------------------------------------------------------------------------------------------------------------- upload, download, events
def _pinned(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 255, (max(n, 16),), dtype=torch.uint8, generator=g).pin_memory()


@pytest.mark.parametrize("n", [0, 16, 4096, 4100])
def test_upload_is_bit_equal(n):
    """16 and 4096 bytes go through the kernel that reads the pinned block over the bus, 4100 (no multiple of 16) through the copy;
    0 is a no-op."""
    lib = _lib()
    src = _pinned(n, 7)
    dst = torch.full((n + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    ev = lib.miseg_event_create()
    assert ev
    try:
        assert lib.miseg_upload(_st(), dst.data_ptr() + 64, src.data_ptr(), n) == 0
        assert lib.miseg_event_record(_st(), ev) == 0
        assert lib.miseg_event_synchronize(ev) == 0
        assert lib.miseg_event_query(ev) == 1
        got = dst.cpu()
        assert torch.equal(got[64:64 + n], src[:n])
        assert bool((got[:64] == 0xAB).all()) and bool((got[64 + n:] == 0xAB).all())
    finally:
        sync()
        lib.miseg_event_destroy(ev)


def test_recorded_upload_download_event_replay_with_a_second_staging_set():
    """The production pattern (StepTape._record): the pinned source, the pinned destination and the event are bound, and a replay
    goes through another set of them."""
    lib = _lib()
    n = 4096
    src_a, src_b = _pinned(n, 1), _pinned(n, 2)
    dst_a, dst_b = torch.zeros(n, dtype=torch.uint8).pin_memory(), torch.zeros(n, dtype=torch.uint8).pin_memory()
    dev = torch.full((n + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    ev_a, ev_b = lib.miseg_event_create(), lib.miseg_event_create()
    assert ev_a and ev_b
    try:
        with recording() as h:
            assert lib.miseg_upload(_st(), dev.data_ptr() + 64, src_a.data_ptr(), n) == 0
            assert lib.miseg_download(_st(), dst_a.data_ptr(), dev.data_ptr() + 64, n) == 0
            assert lib.miseg_event_record(_st(), ev_a) == 0
            sealed(h)
            assert names(h) == ["miseg_upload", "miseg_download", "miseg_event_record"]
            assert lib.miseg_event_synchronize(ev_a) == 0
            assert torch.equal(dst_a, src_a)
            slots = [lib.miseg_tape_bind(h, src_a.data_ptr(), n), lib.miseg_tape_bind(h, ev_a, 1), lib.miseg_tape_bind(h, dst_a.data_ptr(), n)]
            assert slots == [0, 1, 2] and [lib.miseg_tape_bind_uses(h, s) for s in slots] == [1, 1, 1]
            sync()
            dst_a.fill_(0xEE)
            assert replay(h, src_b.data_ptr(), ev_b, dst_b.data_ptr()) == 0
            assert lib.miseg_event_synchronize(ev_b) == 0
            assert lib.miseg_event_query(ev_b) == 1
            assert torch.equal(dst_b, src_b) and bool((dst_a == 0xEE).all())
            got = dev.cpu()
            assert torch.equal(got[64:64 + n], src_b) and bool((got[:64] == 0xAB).all()) and bool((got[64 + n:] == 0xAB).all())
    finally:
        sync()
        lib.miseg_event_destroy(ev_a)
        lib.miseg_event_destroy(ev_b)


def test_upload_from_pageable_memory_takes_the_fallback_and_leaves_no_stale_error():
    lib = _lib()
    n = 4096
    src = torch.arange(n, dtype=torch.int32).to(torch.uint8)     # ordinary host memory
    assert not src.is_pinned()
    dst = torch.full((n + 128,), 0xAB, dtype=torch.uint8, device=DEV)
    z = Buf(1)
    assert lib.miseg_upload(_st(), dst.data_ptr() + 64, src.data_ptr(), n) == 0
    assert fill_zero(z) == 0                                     # its launch check would report an error left behind
    sync()
    got = dst.cpu()
    assert torch.equal(got[64:64 + n], src) and bool((got[:64] == 0xAB).all()) and bool((got[64 + n:] == 0xAB).all())
    assert float(z.mid.abs().sum()) == 0.0 and z.guards_intact()


# ---------------------------------------------------------------------------------------------------------------- miseg_flip
def test_flip_keeps_its_own_copy_of_the_host_stride_arrays():
    lib = _lib()
    H = _H()
    g = torch.Generator().manual_seed(5)
    shape = (2, 3, 5, 7)
    x = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    x2 = torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    assert x.stride() == out.stride() == (105, 1, 21, 3)
    flips = torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    flips2 = torch.tensor([3, 0], dtype=torch.int32, device=DEV)
    ist, ost = (ctypes.c_int64 * 4)(*x.stride()), (ctypes.c_int64 * 4)(*out.stride())

    def ref(t, decisions):
        return torch.stack([t[i].flip([d for d, bit in ((1, 1), (2, 2)) if f & bit]) for i, f in enumerate(decisions)])

    with recording() as h:
        assert lib.miseg_flip(_st(), x.data_ptr(), out.data_ptr(), *shape, ist, ost, 4, flips.data_ptr()) == 0
        sealed(h)
        assert names(h) == ["miseg_flip"] and lib.miseg_tape_op_stream(h, 0) == _st()
        sync()
        eager = out.clone()
        assert torch.equal(eager, ref(x, [1, 2]))
        for i in range(4):                                       # the caller's arrays go away (all-zero strides stay inside the tensors)
            ist[i] = 0
            ost[i] = 0
        H.poison(out)
        assert replay(h) == 0
        sync()
        assert torch.equal(H.bits(out), H.bits(eager))
        slots = [lib.miseg_tape_bind(h, x.data_ptr(), H.nbytes(x)), lib.miseg_tape_bind(h, out.data_ptr(), H.nbytes(out)),
                 lib.miseg_tape_bind(h, flips.data_ptr(), 8)]
        assert slots == [0, 1, 2] and [lib.miseg_tape_bind_uses(h, s) for s in slots] == [1, 1, 1]
        H.poison(out)
        H.poison(out2)
        assert replay(h, x2.data_ptr(), out2.data_ptr(), flips2.data_ptr()) == 0
        sync()
        assert torch.equal(out2, ref(x2, [3, 0]))
        assert bool((H.bits(out) == -1).all())


# ---------------------------------------------------------------------------------------------------------------- the harness itself
def _copy_case():
    H = _H()
    from miseg_amd import _cabi
    g = torch.Generator().manual_seed(9)
    src, alt = torch.randn(N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    acc0 = torch.randn(N, generator=g).to(DEV)

    def call(T):
        _cabi.call("miseg_copy", _st(), T["dst"].data_ptr(), T["src"].data_ptr(), N * 4)
        _cabi.call("miseg_axpy", _st(), 0, T["src"].data_ptr(), T["acc"].data_ptr(), N)

    return H.Case(call=call, inputs={"src": src}, inout={"acc": acc0}, outputs={"dst": torch.empty(N, device=DEV)}, rebind="src", alt=alt,
                  expect=("miseg_copy", "miseg_axpy"))


def test_harness_passes_a_correct_replay():
    assert _H().assert_replay_equals_eager(_copy_case()) == ["miseg_copy", "miseg_axpy"]


def test_harness_detects_a_missing_replay():
    """The comparison after replaying nothing: the outputs are still poison and the in-place state is the restored snapshot, so it
    must raise -- the harness cannot pass vacuously."""
    H = _H()
    with pytest.raises(H.ReplayMismatch):
        H.assert_replay_equals_eager(_copy_case(), replayer=lambda rec: None)
    h = _lib().miseg_tape_begin()
    assert h, "the failed comparison left a tape recording"
    _lib().miseg_tape_free(h)


def test_harness_reports_device_work_outside_the_library():
    H = _H()
    case = _copy_case()
    inner = case.call

    def call(T):
        inner(T)
        T["dst"].add_(1.0)                                       # an ATen launch the tape cannot replay

    case.call = call
    with pytest.raises(AssertionError, match="not tape-clean"):
        H.assert_replay_equals_eager(case)


def test_record_frees_the_tape_when_the_call_raises():
    H = _H()

    def boom():
        raise RuntimeError("boom")

    with pytest.raises(RuntimeError, match="boom"):
        H.record(boom)
    h = _lib().miseg_tape_begin()
    assert h
    _lib().miseg_tape_free(h)
