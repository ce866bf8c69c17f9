"""GPU: the uncertainty-aware Mean Teacher (``Trainer.name=uamt``) -- its three kernels (csrc/uamt.hip:
``miseg_noise_add``, ``miseg_softmax_accum``, ``miseg_softmax_umse``) against torch's fp32 expression (the noise, bit for bit) and the
float64 restatement of tests/uamt_ref.py (checked on the CPU by test_cpu_uamt.py), their refusals, their launch-tape replay, the
step under the tape, the step against its unfused twin, and the CLI.

Accumulator and masked loss: every entry of ``pixel_ref.LOSS_CASES`` (all class counts x logit scales, a short block, exactly one
block, the grid-stride shape) with T = 3 passes from ``uamt_ref.pass_logits``, ``(a, b) = pixel_ref.case_inputs("mse", name)``, the
accumulator of the loss tests the float64 sum rounded to float32, and the threshold ``uamt_ref.case_threshold``: the middle of the
widest gap of the case's uncertainties (half-gap >= 1e-4 for every case: test_cpu_uamt.py), so that the kernel's mask must be the
reference's at every pixel -- the count is compared exactly, the gradient must be +0.0 at every masked-out pixel.  Bounds: the
accumulator 1e-6 * T absolute; loss and statistics 1e-5 relative, the gradient 1e-5 of max|ref| (pixel_ref's).

Worst measured error per kernel over every case compared with a reference, as a fraction of the bound (run with -s: every case
prints its figures, test_zz_worst_errors the worst ones):
  kernel   value: error / bound                         gradient: max error / bound
  accum    0.120  (c4_s30: 3.6e-07 of 3e-06)            --
  umse     0.013  (stride_c2, thr = 2 ln C: 3.5e-08 of 0.2603)  0.140  (c16_s2: 1.5e-10, max|ref| 1.1e-04)
(MI355X, library 418.)  No case needed a bound of its own.  The statistics agree to 2e-7 relative.  The module takes about 28 s,
19 s of them the CLI test's four processes; no other test takes 2 s.

Launch tape: this module registers the replay cases of the three entry points in ``test_gpu_tape_entry_points.CASES`` when it is
imported (no GPU needed for that), replays them itself -- the noise with another seed, the loss with another threshold re-bound --
and adds the recorded names to ``RECORDED``; it sorts before test_gpu_tape_entry_points.py, so its cases have run when that
module's last test counts.  Both therefore need the whole ``tests`` directory collected.
"""
import functools
import math
import os
import shutil
import zlib

import numpy as np
import pytest
import torch

import pixel_ref as P
import test_gpu_tape_entry_points as T
import trainer_harness as th
import uamt_ref as R
from trainer_harness import FEATURES

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
NEW = ("miseg_noise_add", "miseg_softmax_accum", "miseg_softmax_umse")
WORST = {}
SENTINEL = -12345.0
ACCUM_BOUND = 1e-6 * R.PASSES          # each term a probability <= 1 with a few-ulp fp32 error, plus T roundings of a sum <= T
STATS_REL = 1e-5


# ---------------------------------------------------------------------------------------------------------------- tape cases (import time)
@T.case("miseg_noise_add")
def _case_noise_add(v):
    c = T.abi_case("miseg_noise_add", dict(x=T.rn(3, 1, 6, 10), M=180, passes=2, seed=T.ints([1234567, 5]), sigma=0.1, clip=0.2, out=T.out(2, 180)),
                   rebind="seed")
    c.alt = T.ints([7654321, 9])          # a replay with the seed words re-bound draws another noise
    return c


@T.case("miseg_softmax_accum")
def _case_softmax_accum(v):
    n, h, w = T.LOSS
    return T.abi_case("miseg_softmax_accum", dict(logits=T.rn(n, h, w, 4, scale=3.0), N=n, H=h, W=w, C=4, first=0, acc=T.ru(n, h, w, 4)),
                      inout=("acc",), rebind="logits")


@T.case("miseg_softmax_umse")
def _case_softmax_umse(v):
    n, h, w = T.LOSS
    need = T.q("miseg_softmax_umse_ws_bytes", n, h, w)
    c = T.abi_case("miseg_softmax_umse", dict(a=T.rn(n, h, w, 5, scale=3.0), b=T.rn(n, h, w, 5, scale=3.0), acc=T.simplex(n, h, w, 5, dim=3) * 3.0,
                                              N=n, H=h, W=w, C=5, inv_passes=1.0 / 3.0, thr=T.ints([1.0], dtype=T.F32), upstream=T.ru(1), loss=T.out(1),
                                              ga=T.out(n, h, w, 5), kept=T.out(1, dtype=T.I64), stats=T.out(2), ws=T.ws(need), ws_bytes=need),
                   rebind="thr")
    c.alt = T.ints([1.25], dtype=T.F32)   # a replay with the threshold word re-bound keeps other pixels
    return c


# ---------------------------------------------------------------------------------------------------------------- helpers
def ops():
    from miseg_amd import ops as _ops
    return _ops


def cabi():
    from miseg_amd import _cabi
    return _cabi


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def dev_cl(x):
    return x.to(DEV).contiguous(memory_format=CL)


def seed_words(seed64):
    lo, hi = seed64 & 0xFFFFFFFF, (seed64 >> 32) & 0xFFFFFFFF
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in (lo, hi)], dtype=torch.int32, device=DEV)


def thr_dev(thr):
    return torch.tensor([thr], dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. the noise
def _unaligned(numel, fill=None):
    """A float32 device view of ``numel`` elements that starts 4 bytes behind a 16-byte boundary."""
    buf = torch.empty(numel + 4, device=DEV) if fill is None else torch.full((numel + 4,), fill, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[1:1 + numel]


def torch_noise(x, seed64, passes, sigma, clip):
    """The fp32 torch expression on the generator's normals: [passes, M]."""
    m = x.numel()
    rows = []
    for p in range(passes):
        z = ops().normal_fill(torch.empty(m, device=DEV), seed64, p * m)
        rows.append(R.noise(x.reshape(-1), z, sigma, clip))
    return torch.stack(rows)


def raw_noise(x, words, passes, sigma, clip, out=None):
    m = x.numel()
    out = torch.full((passes, m), float("nan"), device=DEV) if out is None else out
    cabi().call("miseg_noise_add", stream(), ptr(x), m, passes, ptr(words), sigma, clip, ptr(out))
    torch.cuda.synchronize()
    return out


NOISE_SHAPES = {"scalar_3x1x19x23": ((3, 1, 19, 23), False), "vector_2x1x64x64": ((2, 1, 64, 64), False),
                "unaligned_3x1x19x23": ((3, 1, 19, 23), True), "unaligned_2x1x64x64": ((2, 1, 64, 64), True)}
SEEDS = (1234567, (5 << 32) | 0x80000001)        # what the epocher draws, and one with a high word and a set sign bit


@pytest.mark.parametrize("seed64", SEEDS)
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("tag", list(NOISE_SHAPES))
def test_noise_add_equals_the_torch_expression_bit_for_bit(tag, passes, seed64):
    shape, unaligned = NOISE_SHAPES[tag]
    x = P.logits(f"uamt/noise/{tag}", *shape).to(DEV)
    m = x.numel()
    out = None
    if unaligned:
        flat = _unaligned(m)
        flat.copy_(x.reshape(-1))
        x, out = flat, _unaligned(passes * m, float("nan")).view(passes, m)
        assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    got = raw_noise(x, seed_words(seed64), passes, 0.1, 0.2, out)
    want = torch_noise(x, seed64, passes, 0.1, 0.2)
    assert torch.equal(P.bits(got), P.bits(want))
    delta = (got - x.reshape(1, -1)).abs()
    assert float(delta.max()) <= 0.2 + 1e-6 and float(delta.max()) > 0.19 and bool(torch.isfinite(got).all())      # the clip bites (2 sigma)
    if passes > 1:
        assert not torch.equal(got[0], got[1])
    if not unaligned:
        wrapped = ops().noise_add(x, seed_words(seed64), passes, 0.1, 0.2)
        assert wrapped.shape == (passes,) + tuple(shape) and torch.equal(P.bits(wrapped.reshape(passes, -1)), P.bits(got))


def test_noise_add_sigma_zero_returns_the_input_and_two_seeds_differ():
    x = P.bit_payload("uamt/noise/payload", (3, 1, 19, 23)).to(DEV)          # NaN payloads, -0.0, denormals
    got = raw_noise(x, seed_words(SEEDS[0]), 2, 0.0, 0.2)
    normal = (torch.isfinite(x.reshape(-1)) & (x.reshape(-1).abs() >= 2.0 ** -126)).cpu()
    assert int(normal.sum()) > 0.8 * x.numel()
    for p in range(2):       # x + 0.0: the bits of every normal value (a NaN may lose its payload, -0.0 its sign, a denormal may be flushed)
        assert torch.equal(P.bits(got[p])[normal], P.bits(x.reshape(-1))[normal])
    y = P.logits("uamt/noise/two", 2, 1, 64, 64).to(DEV)
    same = raw_noise(y, seed_words(SEEDS[0]), 1, 0.0, 0.2)
    assert torch.equal(P.bits(same[0]), P.bits(y.reshape(-1)))
    a, b = raw_noise(y, seed_words(SEEDS[0]), 1, 0.1, 0.2), raw_noise(y, seed_words(SEEDS[0] + 1), 1, 0.1, 0.2)
    hi = raw_noise(y, seed_words(SEEDS[0] | (1 << 32)), 1, 0.1, 0.2)
    assert not torch.equal(a, b) and not torch.equal(a, hi) and torch.equal(a, raw_noise(y, seed_words(SEEDS[0]), 1, 0.1, 0.2))
    assert float((a != b).float().mean()) > 0.99


# ---------------------------------------------------------------------------------------------------------------- 2. the accumulator
def _worst(kernel, tag, ev, bv, eg=0.0, bg=1.0):
    w = WORST.setdefault(kernel, [0.0, "", 0.0, ""])
    if ev / bv > w[0]:
        w[0], w[1] = ev / bv, tag
    if eg / bg > w[2]:
        w[2], w[3] = eg / bg, tag


@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_softmax_accum_vs_float64(name):
    acc = None
    for p in range(R.PASSES):
        acc = ops().softmax_accum(dev_cl(R.pass_logits(name, p)), acc)
    err = float((acc.cpu().to(R.F64) - R.case_acc(name)).abs().max())
    print(f"\nUAMT accum {name:14s} max|acc - ref| = {err:.3e} (bound {ACCUM_BOUND:.1e})")
    _worst("accum", name, err, ACCUM_BOUND)
    assert acc.is_contiguous(memory_format=CL) and bool(torch.isfinite(acc).all())
    assert err <= ACCUM_BOUND


def test_softmax_accum_first_overwrites_and_layouts_agree():
    name = "c3_s2"
    n, h, w, c, _ = P.LOSS_CASES[name]
    z = [R.pass_logits(name, p) for p in range(2)]
    acc = torch.full((n, h, w, c), SENTINEL, device=DEV)
    z0 = dev_cl(z[0])
    cabi().call("miseg_softmax_accum", stream(), ptr(z0), n, h, w, c, 1, ptr(acc))
    torch.cuda.synchronize()
    first = ops().softmax_accum(z0)
    assert torch.equal(P.bits(acc), P.bits(first.permute(0, 2, 3, 1)))
    assert float((acc.cpu().to(R.F64) - R.accumulate(z[:1]).permute(0, 2, 3, 1)).abs().max()) <= 1e-6
    # contiguous NCHW goes through the wrapper's conversion, channels-last does not; C = 3 so that the two layouts differ
    plain = ops().softmax_accum(z[1].to(DEV).contiguous(), ops().softmax_accum(z[0].to(DEV).contiguous()))
    cl = ops().softmax_accum(dev_cl(z[1]), ops().softmax_accum(dev_cl(z[0])))
    assert torch.equal(P.bits(plain), P.bits(cl))
    # the order of the calls is the order of the additions: the same calls give the same bits
    again = ops().softmax_accum(dev_cl(z[1]), ops().softmax_accum(dev_cl(z[0])))
    assert torch.equal(P.bits(again), P.bits(cl))


# ---------------------------------------------------------------------------------------------------------------- 3. the masked loss
@functools.lru_cache(maxsize=None)
def acc32(name):
    """The float64 accumulator of a case rounded to float32, NCHW-shaped on the CPU.  Shared: read-only."""
    return R.case_acc(name).float()


def wrapper_run(name, thr, layout=dev_cl, scale=None):
    """(loss, gradient, kept, stats) through the ops wrapper."""
    a, b = P.case_inputs("mse", name)
    a = layout(a).detach().clone().requires_grad_(True)
    loss, kept, stats = ops().softmax_umse(a, layout(b), layout(acc32(name)), thr_dev(thr), R.PASSES)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), a.grad, kept, stats


def raw_umse(name, thr, upstream=None, want=("ga", "kept", "stats")):
    """One C-ABI call: (loss [1], grad NCHW-shaped or None, kept or None, stats or None), all on the device."""
    a, b = P.case_inputs("mse", name)
    n, c, h, w = a.shape
    need = cabi().query("miseg_softmax_umse_ws_bytes", n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    grad = torch.full((n, c, h, w), float("nan"), device=DEV).contiguous(memory_format=CL) if "ga" in want else None
    kept = torch.full((1,), -7, dtype=torch.int64, device=DEV) if "kept" in want else None
    stats = torch.full((2,), float("nan"), device=DEV) if "stats" in want else None
    a_d, b_d, acc_d = dev_cl(a), dev_cl(b), dev_cl(acc32(name))
    cabi().call("miseg_softmax_umse", stream(), ptr(a_d), ptr(b_d), ptr(acc_d), n, h, w, c, 1.0 / R.PASSES, ptr(thr_dev(thr)), ptr(upstream),
                ptr(loss), ptr(grad), ptr(kept), ptr(stats), ptr(ws), need)
    torch.cuda.synchronize()
    return loss, grad, kept, stats


def check(tag, loss, grad, ref_loss, ref_grad, gscale=1.0, kernel="umse"):
    el, bl = P.loss_error(float(loss), float(ref_loss))
    eg, bg = P.grad_error(grad, ref_grad * gscale)
    print(f"\nUAMT {kernel} {tag:30s} loss={float(loss):.9g} ref={float(ref_loss):.9g} err={el:.3e} (bound {bl:.3e})  "
          f"grad err={eg:.3e} (bound {bg:.3e}, max|ref|={float(ref_grad.abs().max()) * abs(gscale):.3e})")
    _worst(kernel, tag, el, bl, eg, bg)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    assert el <= bl, (tag, "loss", el, bl)
    assert eg <= bg, (tag, "grad", eg, bg)


def check_mask(tag, grad, kept, stats, k, mask, unc, zero_bits=True):
    """The count exactly, exactly zero at every masked-out pixel -- +0.0 as the kernel writes it (``zero_bits``; autograd's own product
    with a negative upstream turns it into -0.0) --, the two statistics at 1e-5 relative."""
    assert int(kept) == k, (tag, int(kept), k)
    out = ~mask.unsqueeze(1).expand(-1, grad.shape[1], -1, -1)
    assert bool((grad.cpu()[out] == 0).all()), tag
    assert not zero_bits or bool((P.bits(grad)[out] == 0).all()), tag
    want = (k / mask.numel(), float(unc.mean()))
    for got, ref, what in zip(stats.tolist(), want, ("certain", "uncertainty")):
        print(f"\nUAMT umse {tag:30s} {what} {got:.9g} ref {ref:.9g}")
        assert abs(got - ref) <= STATS_REL * abs(ref), (tag, what, got, ref)


@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_softmax_umse_vs_float64(name):
    thr, half = R.case_threshold(name)
    assert half >= R.MIN_HALF_GAP
    ref_loss, ref_grad, hand, k, mask, unc = R.case_reference(name, thr)
    loss, grad, kept, stats = wrapper_run(name, thr)
    check(name, loss, grad, ref_loss, ref_grad)
    check_mask(name, grad, kept, stats, k, mask, unc)
    assert 0 < k < mask.numel()


@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_every_pixel_certain_is_the_plain_mse(name):
    c = P.LOSS_CASES[name][3]
    ref_loss, ref_grad = P.case_reference("mse", name)
    loss, grad, kept, stats = wrapper_run(name, R.f32(2.0 * math.log(c)))
    n, h, w = P.LOSS_CASES[name][:3]
    assert int(kept) == n * h * w and float(stats[0]) == 1.0
    check(f"{name} thr=2lnC", loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("name", ["c4_s2", "c3_s12", "short_c16", "stride_c2"])
def test_no_pixel_certain_is_zero_never_nan(name):
    for run in (lambda: wrapper_run(name, 0.0), lambda: raw_umse(name, 0.0, upstream=torch.tensor([-3.0], device=DEV))):
        loss, grad, kept, stats = run()
        assert int(P.bits(loss).reshape(-1)[0]) == 0 and int(kept) == 0 and float(stats[0]) == 0.0
        assert bool((P.bits(grad) == 0).all())
        assert math.isfinite(float(stats[1])) and float(stats[1]) > 0


def test_plain_nchw_and_channels_last_inputs_agree_bit_for_bit():
    """Contiguous NCHW goes through the wrapper's conversion, channels-last does not; C = 3 so that the two layouts differ."""
    thr, _ = R.case_threshold("c3_s2")
    l0, g0, k0, s0 = wrapper_run("c3_s2", thr, layout=lambda x: x.to(DEV).contiguous())
    l1, g1, k1, s1 = wrapper_run("c3_s2", thr)
    assert torch.equal(P.bits(l0), P.bits(l1)) and torch.equal(P.bits(g0), P.bits(g1)) and int(k0) == int(k1) and torch.equal(P.bits(s0), P.bits(s1))
    ref_loss, ref_grad, *_ = R.case_reference("c3_s2", thr)
    check("c3_s2 nchw", l0, g0, ref_loss, ref_grad)


def test_upstream_through_autograd_and_through_the_device_pointer():
    name = "c5_s2"
    thr, _ = R.case_threshold(name)
    ref_loss, ref_grad, _, k, mask, unc = R.case_reference(name, thr)
    loss, grad, kept, stats = wrapper_run(name, thr, scale=-2.5)
    check(f"{name} autograd x -2.5", loss, grad, ref_loss, ref_grad, gscale=-2.5)
    check_mask(name, grad, kept, stats, k, mask, unc, zero_bits=False)
    loss, grad, kept, stats = raw_umse(name, thr, upstream=torch.tensor([0.375], device=DEV))
    check(f"{name} upstream 0.375", loss, grad, ref_loss, ref_grad, gscale=0.375)
    check_mask(name, grad, kept, stats, k, mask, unc)
    # the loss scale of the fp16 mode arrives the same way: a large upstream
    loss, grad, *_ = raw_umse(name, thr, upstream=torch.tensor([65536.0], device=DEV))
    check(f"{name} upstream 65536", loss, grad, ref_loss, ref_grad, gscale=65536.0)


@pytest.mark.parametrize("name", ["c4_s2", "c3_s12"])
def test_null_outputs_and_two_calls_give_the_same_bits(name):
    thr, _ = R.case_threshold(name)
    l0, g0, k0, s0 = raw_umse(name, thr)
    l1, g1, k1, s1 = raw_umse(name, thr)
    assert torch.equal(P.bits(l0), P.bits(l1)) and torch.equal(P.bits(g0), P.bits(g1)) and int(k0) == int(k1) and torch.equal(P.bits(s0), P.bits(s1))
    for want in ((), ("ga",), ("kept",), ("stats",)):
        l2, g2, k2, s2 = raw_umse(name, thr, want=want)
        assert torch.equal(P.bits(l0), P.bits(l2))
        assert (g2 is None) == ("ga" not in want) and (k2 is None) == ("kept" not in want) and (s2 is None) == ("stats" not in want)
        assert g2 is None or torch.equal(P.bits(g0), P.bits(g2))
        assert k2 is None or int(k2) == int(k0)
        assert s2 is None or torch.equal(P.bits(s0), P.bits(s2))
    ref_loss, ref_grad, *_ = R.case_reference(name, thr)
    check(f"{name} raw", l0, g0, ref_loss, ref_grad)


def test_outputs_live_in_the_step_block_inside_an_iteration():
    """``kept`` is two adjacent counters of the step block (8-byte aligned), ``loss`` and ``stats`` come from the scalar arena."""
    from miseg_amd import stepio
    name = "c4_s2"
    thr, _ = R.case_threshold(name)
    _, _, _, k, _, _ = R.case_reference(name, thr)
    io = stepio.StepIO(torch.device(DEV, torch.cuda.current_device()))
    io.begin([0, 0, 0], [[0.0] * 4])
    io.counter()                                    # an odd number of counters taken before: the pair must skip one
    stepio.CURRENT = io
    try:
        a, b = P.case_inputs("mse", name)
        dev = io.device
        loss, kept, stats = ops().softmax_umse(a.to(dev).contiguous(memory_format=CL), b.to(dev).contiguous(memory_format=CL),
                                               acc32(name).to(dev).contiguous(memory_format=CL), thr_dev(thr).to(dev), R.PASSES)
    finally:
        stepio.CURRENT = None
    torch.cuda.synchronize()
    assert kept.dtype == torch.int64 and kept.data_ptr() % 8 == 0 and int(kept) == k
    base = io.counters_base()
    assert base.data_ptr() <= kept.data_ptr() < base.data_ptr() + 4 * base.numel()
    assert io.arena_offset(loss) is not None and io.arena_offset(stats) is not None and io.arena_offset(stats[0]) is not None


def test_zz_worst_errors():
    for kernel, (wl, tl, wg, tg) in sorted(WORST.items()):
        print(f"\nUAMT WORST {kernel:7s} value {wl:.3f} of its bound ({tl})   gradient {wg:.3f} of its bound ({tg})")
    assert set(WORST) == {"accum", "umse"} or not WORST


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing_and_write_nothing():
    from miseg_amd._cabi import MisegError
    n, h, w, c = 3, 19, 23, 4
    need = cabi().query("miseg_softmax_umse_ws_bytes", n, h, w)
    a, b, acc = torch.randn(n, h, w, c, device=DEV), torch.randn(n, h, w, c, device=DEV), torch.rand(n, h, w, c, device=DEV)
    thr = thr_dev(1.0)
    loss, ga = torch.full((1,), SENTINEL, device=DEV), torch.full((n, h, w, 16), SENTINEL, device=DEV)
    kept, stats = torch.full((1,), 77, dtype=torch.int64, device=DEV), torch.full((2,), SENTINEL, device=DEV)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    big = torch.full((n, h, w, 32), SENTINEL, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((loss == SENTINEL).all()) and bool((ga == SENTINEL).all()) and int(kept) == 77 and bool((stats == SENTINEL).all()) and \
            bool((ws == 0x5A).all()) and bool((big == SENTINEL).all())

    good = dict(a=a, b=b, acc=acc, thr=thr, N=n, H=h, W=w, C=c, ws=ws, ws_bytes=need, loss=loss)
    refusals = [dict(C=k) for k in P.REFUSED_CLASS_COUNTS] + [dict(N=0), dict(H=0), dict(W=0), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                                                              dict(a=None), dict(b=None), dict(acc=None), dict(thr=None), dict(loss=None), dict(ws=None)]
    for change in refusals:
        k = {**good, **change}
        with pytest.raises(MisegError):
            cabi().call("miseg_softmax_umse", stream(), ptr(k["a"]), ptr(k["b"]), ptr(k["acc"]), k["N"], k["H"], k["W"], k["C"], 1.0 / 3.0, ptr(k["thr"]),
                        None, ptr(k["loss"]), ptr(ga), ptr(kept), ptr(stats), ptr(k["ws"]), k["ws_bytes"])
        assert untouched(), change
    good = dict(logits=a, acc=big, N=n, H=h, W=w, C=c)
    for change in [dict(C=k) for k in P.REFUSED_CLASS_COUNTS] + [dict(N=0), dict(H=0), dict(W=0), dict(logits=None), dict(acc=None)]:
        k = {**good, **change}
        for first in (0, 1):
            with pytest.raises(MisegError):
                cabi().call("miseg_softmax_accum", stream(), ptr(k["logits"]), k["N"], k["H"], k["W"], k["C"], first, ptr(k["acc"]))
        assert untouched(), change
    m = 3 * 19 * 23
    x, out, words = torch.randn(m, device=DEV), torch.full((2 * m,), SENTINEL, device=DEV), seed_words(5)
    good = dict(x=x, M=m, passes=2, seed=words, out=out)
    for change in (dict(M=0), dict(M=-4), dict(passes=0), dict(passes=-1), dict(x=None), dict(seed=None), dict(out=None)):
        k = {**good, **change}
        with pytest.raises(MisegError):
            cabi().call("miseg_noise_add", stream(), ptr(k["x"]), k["M"], k["passes"], ptr(k["seed"]), 0.1, 0.2, ptr(k["out"]))
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), change
    keep = out.clone()
    for alias in (out, out[m:], out[m - 1:]):       # in place, x the second copy, x straddling the two
        with pytest.raises(MisegError):
            cabi().call("miseg_noise_add", stream(), ptr(alias), m if alias.numel() >= m else alias.numel(), 2, ptr(words), 0.1, 0.2, ptr(out))
    torch.cuda.synchronize()
    assert torch.equal(out, keep)


# ---------------------------------------------------------------------------------------------------------------- 5. tape, entry points
@pytest.mark.parametrize("name", NEW)
def test_replay_equals_eager(name):
    import tape_harness
    T._G.manual_seed(zlib.crc32(f"{name}/call".encode()))
    c = T.CASES[name](None)
    torch.cuda.synchronize()
    try:
        names = tape_harness.assert_replay_equals_eager(c)
    finally:
        torch.cuda.synchronize()
    assert name in names
    T.RECORDED.update(names)


# ---------------------------------------------------------------------------------------------------------------- 6. tape, step
UAMT = dict(H=64, LB=2, UB=3, lr=1e-3, wd=1e-5, weight=0.1, alpha=0.99, ema_wd=1e-6, passes=2, sigma=0.1, clip=0.2)


def build(dtype="float32", num_batches=3, k_total=7):
    """Student and teacher from different seeded states, the trainer's optimiser / updater, synthetic device loaders."""
    from deepclustering2.loss import KL_div
    from deepclustering2.models import ema_updater
    from deepclustering2.optim import Adam
    from semi_seg.epocher import UAMTEpocher
    from semi_seg.synthetic import SyntheticPairs
    model, teacher = th.unet(dtype, 31), th.unet(dtype, 32)
    for p in teacher.parameters():
        p.detach_().requires_grad_(False)
    opt = Adam(model.parameters(), lr=UAMT["lr"], weight_decay=UAMT["wd"])
    upd = ema_updater(alpha=UAMT["alpha"], justify_alpha=True, weight_decay=UAMT["ema_wd"])
    lab = SyntheticPairs(UAMT["LB"], UAMT["H"], 4, seed=0, device=DEV)
    unl = SyntheticPairs(UAMT["UB"], UAMT["H"], 4, seed=1, device=DEV)
    ep = UAMTEpocher(model, teacher, opt, iter(lab), iter(unl), KL_div(verbose=False), torch.nn.MSELoss(), UAMT["weight"], num_batches, 0, DEV,
                     feature_position=FEATURES, feature_importance=th.IMPORTANCE, ema_updater=upd, passes=UAMT["passes"],
                     noise_sigma=UAMT["sigma"], noise_clip=UAMT["clip"], k_total=k_total)
    return ep, model, teacher, opt, upd


def _teacher_state(built):
    ep, model, teacher, opt, upd = built
    return {"teacher": upd._mirror.flat_param.detach().clone(), "teacher_bn": [b.detach().clone() for b in teacher.buffers()]}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_uamt_tape_replay_equals_eager_steps(dtype):
    """7 iterations, the seed drawn anew and the threshold ramping in every one: 2 eager + 1 recorded + 4 replayed iterations give
    the student, Adam's moments, the teacher's flat buffer and BatchNorm buffers and the meters of 7 eager iterations, bit for bit."""
    def run(tape):
        return th.run_steps(lambda: build(dtype, num_batches=7), 7, tape, mi_precision="fp32" if dtype == "float32" else "f16f8",
                            extra_state=_teacher_state)
    got, info = run(True)
    ref, _ = run(False)
    th.assert_replayed(info, 4)
    names = info.op_names
    assert names.count("miseg_noise_add") == 1 and names.count("miseg_softmax_accum") == UAMT["passes"], names
    assert names.count("miseg_softmax_umse") == 1 and names.count("miseg_ema_update") == 1, names
    assert "miseg_softmax_mse" not in names and "miseg_normal_fill" not in names
    assert "threshold" in got["meters"] and "certain" in got["meters"] and "uncertainty" in got["meters"]
    th.assert_same_state(got, ref, ("param", "m", "v", "teacher", "teacher_bn", "meters"))


# ---------------------------------------------------------------------------------------------------------------- 7. step vs the unfused twin
TWIN_SEEDS = (4242, 777, 31337)


def _torch_twins(monkeypatch, seen):
    """The three kernels as materialised torch expressions on the device, the noise on the generator's own normals."""
    from miseg_amd import ops as O
    normal_fill = O.normal_fill

    def noise_add(x, words, passes, sigma, clip):
        lo, hi = (int(w) & 0xFFFFFFFF for w in words.tolist())
        m = x.numel()
        rows = [R.noise(x, normal_fill(torch.empty(m, device=x.device), (hi << 32) | lo, p * m).view_as(x), sigma, clip) for p in range(passes)]
        return torch.stack(rows)

    def softmax_accum(logits, acc=None):
        p = logits.detach().float().softmax(1)
        return p if acc is None else acc + p

    def softmax_umse(a, b, acc, thr, passes):
        m = acc / passes
        unc = -(m * torch.log(m + 1e-6)).sum(1)
        seen.append(unc.detach().cpu().to(R.F64))
        mask = unc < thr[0]
        k = mask.sum()
        d = a.float().softmax(1) - b.detach().float().softmax(1)
        loss = (mask.unsqueeze(1) * d * d).sum() / (a.shape[1] * k.double() + 1e-16).float()
        stats = torch.stack([(k.double() / mask.numel()).float(), (unc.double().mean()).float()])
        return loss, k.view(1), stats

    monkeypatch.setattr(O, "noise_add", noise_add)
    monkeypatch.setattr(O, "softmax_accum", softmax_accum)
    monkeypatch.setattr(O, "softmax_umse", softmax_umse)


def _first_iteration(seed, monkeypatch, twin, thr=None):
    from semi_seg import epocher as E
    seen = []
    with monkeypatch.context() as mp:
        th.replay_seeds(mp, [seed])
        if thr is not None:
            mp.setattr(E, "uamt_threshold", lambda *a: thr)
        if twin:
            _torch_twins(mp, seen)
        with th.adam_gradients(mp) as grads:
            ep, model, teacher, opt, upd = build("float32", num_batches=1)
            ep._TAPE_DEFAULT = False
            per_step = th.keep_records(ep)
            ep.run()
        torch.cuda.synchronize()
        named = {n: (opt.flat.offset_of(p), p.numel()) for n, p in model.named_parameters()}
        return per_step[0], grads[0].cpu(), named, [b.detach().clone() for b in teacher.buffers()], seen


def test_first_iteration_matches_the_unfused_twin(monkeypatch):
    """fp32, 64 x 64, LB = 2, UB = 3, two passes: the iteration with the three kernels against the same iteration with torch
    expressions in their place (same U-Net kernels, same teacher, same noise bits), both at the threshold ``gap_threshold`` finds in
    the uncertainties of a dry twin run from the same state -- so the count of certain pixels is the same number -- at the step-1
    bounds of test_gpu_ict.py's twin.  Then the teacher's BatchNorm buffers: those of one tracked pass on x[0]."""
    for seed in TWIN_SEEDS:
        *_, seen = _first_iteration(seed, monkeypatch, twin=True)
        thr, half = R.gap_threshold(seen[0])
        thr = R.f32(thr)
        print(f"\nUAMT twin seed {seed}: threshold {thr:.6f}, half-gap {half:.3e}, uncertainties in [{float(seen[0].min()):.4f}, {float(seen[0].max()):.4f}]")
        if half >= R.MIN_HALF_GAP:
            break
    else:
        raise AssertionError("no seed leaves a half-gap of 1e-4 around the threshold")
    got, grad, named, bn, _ = _first_iteration(seed, monkeypatch, twin=False, thr=thr)
    ref, grad_ref, named_ref, bn_ref, seen = _first_iteration(seed, monkeypatch, twin=True, thr=thr)
    assert named == named_ref
    assert got["certain"] == ref["certain"] == float(np.float32(float((seen[0] < thr).sum()) / seen[0].numel())) and 0.1 <= got["certain"] <= 0.9
    np.testing.assert_allclose(got["sup_loss"], ref["sup_loss"], rtol=2e-5)
    np.testing.assert_allclose(got["reg_loss"], ref["reg_loss"], rtol=2e-4)
    np.testing.assert_allclose(got["uncertainty"], ref["uncertainty"], rtol=2e-5)
    assert ref["reg_loss"] > 0
    worst = {}
    for n, (off, numel) in named.items():
        x, y = th.sampled(grad, off, numel, f"uamt/grad/{n}"), th.sampled(grad_ref, off, numel, f"uamt/grad/{n}")
        worst[n] = float(np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-30))
    print(f"\nUAMT twin: sup {got['sup_loss']:.9g} / {ref['sup_loss']:.9g}, reg {got['reg_loss']:.9g} / {ref['reg_loss']:.9g}, certain {got['certain']:.6f}, "
          f"uncertainty {got['uncertainty']:.9g} / {ref['uncertainty']:.9g}, worst gradient rel L2 {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
    tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
    assert tail[len(tail) // 2] < 5e-3 and tail[-1] < 1.5e-2, tail
    assert max(worst.values()) < 3e-2, worst
    # the T passes moved nothing: the running statistics are those of a meanteacher-style single tracked pass on x[0]
    assert all(torch.equal(x, y) for x, y in zip(bn, bn_ref))
    from semi_seg.epocher import TrainEpocher
    from semi_seg.synthetic import SyntheticPairs
    _, _, teacher, _, _ = build("float32", num_batches=1)
    unlabeled, *_ = TrainEpocher._unzip_data(next(iter(SyntheticPairs(UAMT["UB"], UAMT["H"], 4, seed=1, device=DEV))), DEV)
    x0 = ops().noise_add(unlabeled.contiguous(), seed_words(seed), 1, UAMT["sigma"], UAMT["clip"])[0]
    teacher.train()
    with torch.no_grad():
        teacher(x0)
    torch.cuda.synchronize()
    single = [b.detach().clone() for b in teacher.buffers()]
    assert len(single) == len(bn) and all(torch.equal(x, y) for x, y in zip(bn, single))
    assert any(int(b) == 1 for b in bn if b.dtype == torch.int64 and b.numel() == 1)          # num_batches_tracked: one pass, not 1 + T


# ---------------------------------------------------------------------------------------------------------------- 8. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.num_batches=2", "Data.size=64", "Data.name=synthetic", "LabeledData.batch_size=2",
         "UnlabeledData.batch_size=3", "UAMTParameters.passes=2"]


def test_main_cli_trains_resumes_and_infers_with_the_teacher(golden):
    save = f"pytest_cli_uamt_{os.getpid()}"
    run_dir = th.run_dir(save)
    dirs = [run_dir, th.run_dir(save + "_resume"), th.run_dir(save + "_inf")]
    for d in dirs:
        shutil.rmtree(d, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=uamt", f"Trainer.save_dir={save}", "Trainer.max_epoch=2"] + _TINY)
        header = open(os.path.join(run_dir, "storage.csv")).read().splitlines()[0].split(",")
        for column in ("tra_uncertainty", "tra_certain", "tra_threshold"):
            assert any(h.startswith(column) for h in header), (column, header)
        ref = sorted(str(x) for x in golden("trainer_io")["partial/tree_last_pth"])
        own = ("_reg_criterion", "_teacher_model/", "_ema_updater/", "_storage/tra_reg_weight", "_storage/tra_uncertainty", "_storage/tra_certain",
               "_storage/tra_threshold")
        for name in ("last.pth", "best.pth"):
            lines = th.checkpoint_tree(os.path.join(run_dir, name))
            # the meanteacher tree: the partial trainer's, the consistency criterion, the teacher (a second _model), the updater, the
            # reg_weight history -- and the histories of the three new meters
            mine = th.own_lines_removed(lines, own)
            if name == "last.pth":        # (best.pth may be the first epoch's: a shorter history)
                assert mine == ref, (sorted(set(mine) - set(ref))[:12], sorted(set(ref) - set(mine))[:12])
            assert {l.split("/")[0].split(" ")[0] for l in mine} == {l.split("/")[0].split(" ")[0] for l in ref}, name
            assert sorted(l.replace("_teacher_model/", "_model/", 1) for l in lines if l.startswith("_teacher_model/")) == \
                sorted(l for l in lines if l.startswith("_model/"))
            assert any(l.startswith("_ema_updater/") for l in lines) and any(l.startswith("_storage/tra_reg_weight") for l in lines)
        sd = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert sd["_ema_updater"]["global_step"] == 4 and sd["_buffers"]["_cur_epoch"] == 1
        assert any(not torch.equal(sd["_teacher_model"][k], sd["_model"][k]) for k in sd["_model"] if "weight" in k)
        assert all(int(v) == 4 for k, v in sd["_teacher_model"].items() if k.endswith("num_batches_tracked"))       # one tracked pass per iteration
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["UAMTParameters"] == {"passes": 2}
        # a resume continues: one more epoch, the updater's call count goes on
        th.run_main(["Trainer.name=uamt", f"Trainer.save_dir={save}_resume", "Trainer.max_epoch=3", f"Checkpoint={run_dir}/last.pth"] + _TINY)
        sd2 = torch.load(os.path.join(dirs[1], "last.pth"), map_location="cpu", weights_only=False)
        assert sd2["_ema_updater"]["global_step"] == 6 and sd2["_buffers"]["_cur_epoch"] == 2
        # inference evaluates the teacher: a checkpoint whose student is scrambled scores the same
        score = th.run_inference(["Trainer.name=uamt", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "last.pth"))
        assert 0.0 <= score <= 1.0
        scrambled = dict(sd, _model={k: (torch.randn_like(v) if v.is_floating_point() else v) for k, v in sd["_model"].items()})
        torch.save(scrambled, os.path.join(run_dir, "scrambled.pth"))
        assert th.run_inference(["Trainer.name=uamt", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "scrambled.pth")) == score
    finally:
        for d in dirs:
            shutil.rmtree(d, ignore_errors=True)
