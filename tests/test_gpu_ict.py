"""GPU: the ICT trainer (``Trainer.name=ict``) -- its three kernels (csrc/ict.hip: ``miseg_cat_mixed``,
``miseg_softmax_mix_mse``, ``miseg_softmax_mix_klcons``) against the float64 restatement of tests/ict_ref.py (checked on the CPU by
test_cpu_ict.py), their refusals and bad indices, their launch-tape replay, the step under the tape, the step against its unfused
twin, and the CLI.

Losses: every entry of ``pixel_ref.LOSS_CASES`` (all class counts x logit scales, a short block, exactly one block, the grid-stride
shape) with ``(a, b) = pixel_ref.case_inputs("mse", name)``, the rotation ``i -> (i + 1) mod N`` and lam = 0.3; 3 x 19 x 23, C = 4
with a fixed point and a 3-cycle at lam 0, 1, 0.25.  Bounds are pixel_ref's: |loss - ref| <= 1e-5 |ref|, max|grad - ref| <= 1e-5
max|ref|.  ``cat_mixed``: the ``a`` rows bit for bit, mixed rows within 3 * 2^-24 * (|c0 x| + |c1 y|).

Worst measured error per kernel over every case compared with a reference, as a fraction of the bound (run with -s: every case
prints its figures, test_zz_worst_errors the worst ones):
  kernel   loss: error / bound                          gradient: max error / bound
  mse      0.016  (c4_s30: 4.5e-08 of 0.2823)           0.108  (c16_s2: 1.8e-11, max|ref| 1.7e-05)
  klcons   0.019  (c3_s12: 1.8e-06 of 9.442)            0.054  (c8_s12: 4.1e-10, max|ref| 7.6e-04)
(MI355X, library 417.)  ``cat_mixed``: at most 0.63 of its bound (648 x 650 images, lam = 0.3).  No case needed a bound of its own.
The kernel tests take about 4 s together, the three tape runs 6 s, the two twin runs 6 s.

Launch tape: tests/test_cpu_tape_table.py and tests/test_gpu_tape_entry_points.py want a replay case in the latter's ``CASES`` for
every taped entry point and its name in ``RECORDED``.  This module registers the three new cases there when it is imported (no GPU
needed for that), replays them itself and adds the recorded names; it sorts before test_gpu_tape_entry_points.py, so its cases have run
when that module's last test counts.  Both therefore need the whole ``tests`` directory collected.
"""
import functools
import math
import os
import shutil
import zlib

import numpy as np
import pytest
import torch

import ict_ref as R
import pixel_ref as P
import test_gpu_tape_entry_points as T
import trainer_harness as th
from trainer_harness import FEATURES

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
NEW = ("miseg_cat_mixed", "miseg_softmax_mix_mse", "miseg_softmax_mix_klcons")
ENTRY = {"mse": "miseg_softmax_mix_mse", "klcons": "miseg_softmax_mix_klcons"}
WORST = {}
SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------------------------------- tape cases (import time)
@T.case("miseg_cat_mixed")
def _case_cat_mixed(v):
    na, nb, c, h, w = 2, 3, 2, 6, 10
    return T.abi_case("miseg_cat_mixed", dict(a=T.rn(na, c, h, w), Na=na, b=T.rn(nb, c, h, w), Nb=nb, C=c, H=h, W=w, perm=T.ints([1, 2, 0]),
                                              coef=T.ints([0.3, 0.7], dtype=T.F32), out=T.out(na + nb, c, h, w), bad=T.zeros(1, dtype=T.I32)),
                      inout=("bad",), rebind="b")


def _mix_loss_case(name, c, perm):
    n, h, w = T.LOSS
    return T.abi_case(name, dict(a=T.rn(n, h, w, c, scale=3.0), b=T.rn(n, h, w, c, scale=3.0), perm=T.ints(perm), coef=T.ints([0.3, 0.7], dtype=T.F32),
                                 ga=T.out(n, h, w, c), bad=T.zeros(1, dtype=T.I32), **T._loss_common(c)), inout=("bad",), rebind="b")


@T.case("miseg_softmax_mix_mse")
def _case_mix_mse(v):
    return _mix_loss_case("miseg_softmax_mix_mse", 4, [2, 0, 5])       # one index out of range: `bad` is written, and replayed


@T.case("miseg_softmax_mix_klcons")
def _case_mix_klcons(v):
    return _mix_loss_case("miseg_softmax_mix_klcons", 5, [1, 2, 0])


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


def perm_dev(perm):
    return torch.tensor(list(perm), dtype=torch.int32, device=DEV)


def coef_dev(lam):
    return torch.tensor(R.coefficients(lam), dtype=torch.float32, device=DEV)


def rotation(n):
    return [(i + 1) % n for i in range(n)]


def wrapper_run(kernel, a, b, perm, lam, scale=None):
    """(loss, gradient) through the ops wrapper; ``a`` a device tensor in the layout under test."""
    a = a.detach().clone().requires_grad_(True)
    fn = ops().softmax_mix_mse if kernel == "mse" else ops().softmax_mix_kl_consistency
    loss = fn(a, b, perm_dev(perm), coef_dev(lam))
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), a.grad


def raw_loss(kernel, a, b, perm, coef, upstream=None, want_grad=True, want_bad=True):
    """One C-ABI call on NCHW-shaped CPU logits: (loss [1], grad NCHW-shaped or None, bad [1] or None), all on the device."""
    n, c, h, w = a.shape
    a_d, b_d = dev_cl(a), dev_cl(b)
    need = cabi().query("miseg_loss_ws_bytes", n, h, w)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    grad = torch.full((n, c, h, w), float("nan"), device=DEV).contiguous(memory_format=CL) if want_grad else None
    bad = torch.zeros(1, dtype=torch.int32, device=DEV) if want_bad else None
    cabi().call(ENTRY[kernel], stream(), ptr(a_d), ptr(b_d), ptr(perm), ptr(coef), n, h, w, c, ptr(upstream), ptr(loss), ptr(grad), ptr(bad),
                ptr(ws), need)
    torch.cuda.synchronize()
    return loss, grad, bad


def raw_cat(a, b, perm, coef, want_bad=True):
    """``miseg_cat_mixed`` on CPU tensors (a may be None: Na = 0, null pointer): (out, bad) on the device."""
    na = 0 if a is None else a.shape[0]
    nb, c, h, w = b.shape
    a_d, b_d = None if a is None else a.to(DEV).contiguous(), b.to(DEV).contiguous()
    out = torch.full((na + nb, c, h, w), float("nan"), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV) if want_bad else None
    cabi().call("miseg_cat_mixed", stream(), ptr(a_d), na, ptr(b_d), nb, c, h, w, ptr(perm), ptr(coef), ptr(out), ptr(bad))
    torch.cuda.synchronize()
    return out, bad


@functools.lru_cache(maxsize=None)
def reference(kernel, name, perm, lam):
    a, b = P.case_inputs("mse", name)
    c0, c1 = R.coefficients(lam)
    return R.loss_and_grad(kernel, a, b, list(perm), c0, c1)


def check(kernel, tag, loss, grad, ref_loss, ref_grad, gscale=1.0):
    el, bl = P.loss_error(float(loss), float(ref_loss))
    eg, bg = P.grad_error(grad, ref_grad * gscale)
    print(f"\nICT {kernel:7s} {tag:30s} loss={float(loss):.9g} ref={float(ref_loss):.9g} err={el:.3e} (bound {bl:.3e})  "
          f"grad err={eg:.3e} (bound {bg:.3e}, max|ref|={float(ref_grad.abs().max()) * abs(gscale):.3e})")
    w = WORST.setdefault(kernel, [0.0, "", 0.0, ""])
    if el / bl > w[0]:
        w[0], w[1] = el / bl, tag
    if eg / bg > w[2]:
        w[2], w[3] = eg / bg, tag
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    assert el <= bl, (kernel, tag, "loss", el, bl)
    assert eg <= bg, (kernel, tag, "grad", eg, bg)


# ---------------------------------------------------------------------------------------------------------------- 1. the losses
@pytest.mark.parametrize("kernel", ["mse", "klcons"])
@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_mix_losses_vs_float64(name, kernel):
    a, b = P.case_inputs("mse", name)
    perm = rotation(a.shape[0])
    ref_loss, ref_grad = reference(kernel, name, tuple(perm), 0.3)
    loss, grad = wrapper_run(kernel, dev_cl(a), dev_cl(b), perm, 0.3)
    check(kernel, name, loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
@pytest.mark.parametrize("lam", [0.0, 1.0, 0.25])
@pytest.mark.parametrize("perm", [(0, 2, 1), (1, 2, 0)])
def test_fixed_point_and_cycle_vs_float64(perm, lam, kernel):
    a, b = P.case_inputs("mse", "c4_s2")          # 3 x 19 x 23, C = 4
    ref_loss, ref_grad = reference(kernel, "c4_s2", perm, lam)
    loss, grad = wrapper_run(kernel, dev_cl(a), dev_cl(b), perm, lam)
    check(kernel, f"c4_s2 perm={perm} lam={lam}", loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
def test_the_mix_is_a_gather_not_a_scatter(kernel):
    """perm = [1, 2, 0] read as a scatter is the gather of its inverse [2, 0, 1]: the two losses lie more than 100 bounds apart."""
    a, b = P.case_inputs("mse", "c4_s2")
    got, _ = wrapper_run(kernel, dev_cl(a), dev_cl(b), (1, 2, 0), 0.25)
    inverse, _ = wrapper_run(kernel, dev_cl(a), dev_cl(b), (2, 0, 1), 0.25)
    ref, _ = reference(kernel, "c4_s2", (1, 2, 0), 0.25)
    _, bound = P.loss_error(float(got), float(ref))
    print(f"\nICT {kernel} gather {float(got):.9g} vs inverse permutation {float(inverse):.9g} (bound {bound:.3e})")
    assert abs(float(got) - float(inverse)) > 100 * bound


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
def test_plain_nchw_and_channels_last_inputs_agree_bit_for_bit(kernel):
    """Contiguous NCHW goes through the wrapper's conversion, channels-last does not; C = 3 so that the two layouts differ."""
    a, b = P.case_inputs("mse", "c3_s2")
    l0, g0 = wrapper_run(kernel, a.to(DEV).contiguous(), b.to(DEV).contiguous(), (1, 2, 0), 0.3)
    l1, g1 = wrapper_run(kernel, dev_cl(a), dev_cl(b), (1, 2, 0), 0.3)
    assert torch.equal(P.bits(l0), P.bits(l1)) and torch.equal(P.bits(g0), P.bits(g1))
    ref_loss, ref_grad = reference(kernel, "c3_s2", (1, 2, 0), 0.3)
    check(kernel, "c3_s2 nchw", l0, g0, ref_loss, ref_grad)


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
def test_upstream_through_autograd_and_through_the_device_pointer(kernel):
    a, b = P.case_inputs("mse", "c5_s2")
    perm, lam = (1, 2, 0), 0.3
    ref_loss, ref_grad = reference(kernel, "c5_s2", perm, lam)
    loss, grad = wrapper_run(kernel, dev_cl(a), dev_cl(b), perm, lam, scale=-2.5)
    check(kernel, "c5_s2 autograd x -2.5", loss, grad, ref_loss, ref_grad, gscale=-2.5)
    up = torch.tensor([0.375], device=DEV)
    loss, grad, bad = raw_loss(kernel, a, b, perm_dev(perm), coef_dev(lam), upstream=up)
    check(kernel, "c5_s2 upstream 0.375", loss, grad, ref_loss, ref_grad, gscale=0.375)
    assert int(bad) == 0


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
@pytest.mark.parametrize("name", ["c4_s2", "c3_s12"])
def test_null_gradient_and_two_calls_give_the_same_bits(name, kernel):
    a, b = P.case_inputs("mse", name)
    perm, coef = perm_dev((1, 2, 0)), coef_dev(0.3)
    l0, g0, _ = raw_loss(kernel, a, b, perm, coef)
    l1, g1, _ = raw_loss(kernel, a, b, perm, coef)
    l2, g2, b2 = raw_loss(kernel, a, b, perm, coef, want_grad=False, want_bad=False)
    assert torch.equal(P.bits(l0), P.bits(l1)) and torch.equal(P.bits(g0), P.bits(g1))
    assert g2 is None and b2 is None and torch.equal(P.bits(l0), P.bits(l2))
    ref_loss, ref_grad = reference(kernel, name, (1, 2, 0), 0.3)
    check(kernel, f"{name} raw", l0, g0, ref_loss, ref_grad)


def test_zz_worst_errors():
    for kernel, (wl, tl, wg, tg) in sorted(WORST.items()):
        print(f"\nICT WORST {kernel:7s} loss {wl:.3f} of its bound ({tl})   gradient {wg:.3f} of its bound ({tg})")
    assert set(WORST) == {"mse", "klcons"} or not WORST


# ---------------------------------------------------------------------------------------------------------------- 2. cat_mixed
# (Na, Nb, C, H, W): a scalar shape (C*H*W odd), a 16-byte one, and one of each that makes the threads loop (> 2048 * 256 units)
CAT_SHAPES = {"2+3x1x19x23": (2, 3, 1, 19, 23), "1+2x3x8x5": (1, 2, 3, 8, 5), "scalar_loop": (1, 3, 1, 419, 419), "vector_loop": (1, 4, 1, 648, 650)}


def _cat_inputs(tag, shape):
    na, nb, c, h, w = shape
    a = P.bit_payload(f"ict/cat/{tag}/a", (na, c, h, w))           # NaN payloads, -0.0, denormals: the copy is of bits
    b = P.logits(f"ict/cat/{tag}/b", nb, c, h, w, 1.0)
    return a, b


@pytest.mark.parametrize("lam", [0.3, 0.0, 1.0])
@pytest.mark.parametrize("tag", list(CAT_SHAPES))
def test_cat_mixed_vs_float64(tag, lam):
    shape = CAT_SHAPES[tag]
    na, nb = shape[:2]
    a, b = _cat_inputs(tag, shape)
    perm = rotation(nb)
    c0, c1 = R.coefficients(lam)
    out, bad = raw_cat(a, b, perm_dev(perm), coef_dev(lam))
    out = out.cpu()
    assert int(bad) == 0
    assert torch.equal(P.bits(out[:na]), P.bits(a))
    err = (out[na:].to(R.F64) - R.mix_rows(b, perm, c0, c1)).abs()
    bound = R.cat_mixed_bound(b, perm, c0, c1)
    print(f"\nICT cat_mixed {tag} lam={lam}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    if lam == 0.0:
        assert torch.equal(P.bits(out[na:]), P.bits(b[torch.tensor(perm)]))      # the plain gather
    if lam == 1.0:
        assert torch.equal(P.bits(out[na:]), P.bits(b))                          # the plain copy
    wrapped = ops().cat_mixed(a.to(DEV), b.to(DEV), perm_dev(perm), coef_dev(lam)).cpu()
    assert torch.equal(P.bits(wrapped), P.bits(out))


def test_cat_mixed_without_labeled_rows():
    for tag in ("2+3x1x19x23", "1+2x3x8x5"):
        _, nb, c, h, w = CAT_SHAPES[tag]
        _, b = _cat_inputs(tag, CAT_SHAPES[tag])
        perm = rotation(nb)
        out, bad = raw_cat(None, b, perm_dev(perm), coef_dev(0.3), want_bad=False)
        with_a, _ = raw_cat(*_cat_inputs(tag, CAT_SHAPES[tag]), perm_dev(perm), coef_dev(0.3))
        assert bad is None and torch.equal(P.bits(out), P.bits(with_a[CAT_SHAPES[tag][0]:]))


# ---------------------------------------------------------------------------------------------------------------- 3. bad indices
def test_bad_indices_count_as_their_own_and_are_reported():
    from miseg_amd import checks
    a, b = P.case_inputs("mse", "c4_s2")
    bad_perm, own = perm_dev([0, 7, -1]), perm_dev([0, 1, 2])
    coef = coef_dev(0.3)
    for kernel in ("mse", "klcons"):
        l0, g0, f0 = raw_loss(kernel, a, b, own, coef)
        l1, g1, f1 = raw_loss(kernel, a, b, bad_perm, coef)
        assert torch.equal(P.bits(l0), P.bits(l1)) and torch.equal(P.bits(g0), P.bits(g1))
        assert int(f0) == 0 and int(f1) == 2
    imgs = _cat_inputs("2+3x1x19x23", CAT_SHAPES["2+3x1x19x23"])
    o0, f0 = raw_cat(*imgs, own, coef)
    o1, f1 = raw_cat(*imgs, bad_perm, coef)
    assert torch.equal(P.bits(o0), P.bits(o1)) and int(f0) == 0 and int(f1) == 2
    # through the wrappers: raised now ...
    o = ops()
    calls = {"cat_mixed": lambda: o.cat_mixed(imgs[0].to(DEV), imgs[1].to(DEV), bad_perm, coef),
             "softmax_mix_mse": lambda: o.softmax_mix_mse(dev_cl(a), dev_cl(b), bad_perm, coef),
             "softmax_mix_kl_consistency": lambda: o.softmax_mix_kl_consistency(dev_cl(a), dev_cl(b), bad_perm, coef)}
    for name, fn in calls.items():
        with pytest.raises(IndexError, match=name):
            fn()
        # ... and inside a deferred block at the fetch
        items = []
        with checks.deferred(items):
            fn()
        assert len(items) == 1
        flags = [float(checks.flag_tensor(it)) for it in items]
        assert flags == [2.0]
        with pytest.raises(IndexError, match=name):
            checks.raise_failed(items, flags)
    items = []
    with checks.deferred(items):
        o.softmax_mix_mse(dev_cl(a), dev_cl(b), own, coef)
    checks.raise_failed(items, [float(checks.flag_tensor(it)) for it in items])


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing_and_write_nothing():
    from miseg_amd._cabi import MisegError
    n, h, w, c = 3, 19, 23, 4
    need = cabi().query("miseg_loss_ws_bytes", n, h, w)
    a, b = torch.randn(n, h, w, c, device=DEV), torch.randn(n, h, w, c, device=DEV)
    perm, coef = perm_dev([1, 2, 0]), coef_dev(0.3)
    loss, ga = torch.full((1,), SENTINEL, device=DEV), torch.full((n, h, w, 16), SENTINEL, device=DEV)
    bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ws = torch.full((max(need, 16),), 0x5A, dtype=torch.uint8, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((loss == SENTINEL).all()) and bool((ga == SENTINEL).all()) and int(bad) == 77 and bool((ws == 0x5A).all())

    good = dict(a=a, b=b, perm=perm, coef=coef, N=n, H=h, W=w, C=c, ws_bytes=need)
    refusals = [dict(C=k) for k in P.REFUSED_CLASS_COUNTS] + [dict(N=0), dict(H=0), dict(ws_bytes=need - 1), dict(perm=None), dict(coef=None),
                                                              dict(a=None), dict(b=None)]
    for entry in ENTRY.values():
        for change in refusals:
            k = {**good, **change}
            with pytest.raises(MisegError):
                cabi().call(entry, stream(), ptr(k["a"]), ptr(k["b"]), ptr(k["perm"]), ptr(k["coef"]), k["N"], k["H"], k["W"], k["C"], None,
                            ptr(loss), ptr(ga), ptr(bad), ptr(ws), k["ws_bytes"])
            assert untouched(), (entry, change)
    na, nb, ch = 2, 3, 1
    x, y = torch.randn(na, ch, h, w, device=DEV), torch.randn(nb, ch, h, w, device=DEV)
    out = torch.full((na + nb, ch, h, w), SENTINEL, device=DEV)
    good = dict(a=x, Na=na, b=y, Nb=nb, C=ch, H=h, W=w, perm=perm, coef=coef)
    for change in (dict(Nb=0), dict(Na=-1), dict(C=0), dict(H=0), dict(W=0), dict(perm=None), dict(coef=None), dict(b=None), dict(a=None)):
        k = {**good, **change}
        with pytest.raises(MisegError):
            cabi().call("miseg_cat_mixed", stream(), ptr(k["a"]), k["Na"], ptr(k["b"]), k["Nb"], k["C"], k["H"], k["W"], ptr(k["perm"]),
                        ptr(k["coef"]), ptr(out), ptr(bad))
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and int(bad) == 77, change
    with pytest.raises(MisegError):       # in place
        cabi().call("miseg_cat_mixed", stream(), None, 0, ptr(y), nb, ch, h, w, ptr(perm), ptr(coef), ptr(y), ptr(bad))


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
ICT = dict(H=64, LB=2, UB=3, lr=1e-3, wd=1e-5, weight=10.0, alpha=0.999, ema_wd=1e-6, mix_alpha=0.5)


def build(dtype="float32", num_batches=3, reg="mse"):
    """Student and teacher from different seeded states, the trainer's optimiser / updater, synthetic device loaders."""
    from deepclustering2.loss import KL_div
    from deepclustering2.models import ema_updater
    from deepclustering2.optim import Adam
    from semi_seg.epocher import ICTEpocher
    from semi_seg.synthetic import SyntheticPairs
    model, teacher = th.unet(dtype, 31), th.unet(dtype, 32)
    for p in teacher.parameters():
        p.detach_().requires_grad_(False)
    opt = Adam(model.parameters(), lr=ICT["lr"], weight_decay=ICT["wd"])
    upd = ema_updater(alpha=ICT["alpha"], justify_alpha=True, weight_decay=ICT["ema_wd"])
    lab = SyntheticPairs(ICT["LB"], ICT["H"], 4, seed=0, device=DEV)
    unl = SyntheticPairs(ICT["UB"], ICT["H"], 4, seed=1, device=DEV)
    crit = torch.nn.MSELoss() if reg == "mse" else KL_div(verbose=False)
    ep = ICTEpocher(model, teacher, opt, iter(lab), iter(unl), KL_div(verbose=False), crit, ICT["weight"], num_batches, 0, DEV,
                    feature_position=FEATURES, feature_importance=th.IMPORTANCE, ema_updater=upd, mix_alpha=ICT["mix_alpha"])
    return ep, model, teacher, opt, upd


def _teacher_state(built):
    ep, model, teacher, opt, upd = built
    return {"teacher": upd._mirror.flat_param.detach().clone(), "teacher_bn": [b.detach().clone() for b in teacher.buffers()]}


@pytest.mark.parametrize("dtype,reg", [("float32", "mse"), ("bfloat16", "mse"), ("float32", "kl")])
def test_ict_tape_replay_equals_eager_steps(dtype, reg):
    """7 iterations, lam and perm drawn anew in every one: 2 eager + 1 recorded + 4 replayed iterations give the student, Adam's
    moments, the teacher's flat buffer and BatchNorm buffers and the meters of 7 eager iterations, bit for bit."""
    def run(tape):
        return th.run_steps(lambda: build(dtype, reg=reg), 7, tape, mi_precision="fp32" if dtype == "float32" else "f16f8",
                            extra_state=_teacher_state)
    got, info = run(True)
    ref, _ = run(False)
    th.assert_replayed(info, 4)
    names = info.op_names
    loss = ENTRY["mse" if reg == "mse" else "klcons"]
    other = ENTRY["klcons" if reg == "mse" else "mse"]
    assert names.count("miseg_cat_mixed") == 1 and names.count("miseg_ema_update") == 1 and names.count(loss) == 1, names
    assert names.count(other) == 0 and not [n for n in names if n.startswith("miseg_cat_flip")], names
    assert "miseg_softmax_mse" not in names and "miseg_softmax_klcons" not in names
    th.assert_same_state(got, ref, ("param", "m", "v", "teacher", "teacher_bn", "meters"))


# ---------------------------------------------------------------------------------------------------------------- 7. step vs the unfused twin
def _cycle_seed(ub, mix_alpha):
    """The first seed whose draw is a 3-cycle (a permutation that is not its own inverse) with lam well inside (0, 1)."""
    for seed in range(1000):
        lam, perm = R.draws(seed, ub, mix_alpha)
        if perm in ([1, 2, 0], [2, 0, 1]) and 0.2 < lam < 0.8:
            return seed, lam, perm
    raise AssertionError("no such seed")


def _torch_twins(monkeypatch):
    """The three kernels as materialised torch expressions on the device."""
    from miseg_amd import ops as O

    def cat_mixed(a, b, perm, coef, check_perm=True):
        return torch.cat([a, coef[0] * b + coef[1] * b[perm.long()]])

    def target(b, perm, coef):
        t = b.detach().float().softmax(1)
        return coef[0] * t + coef[1] * t[perm.long()]

    def mix_mse(a, b, perm, coef, check_perm=True):
        return ((a.float().softmax(1) - target(b, perm, coef)) ** 2).mean()

    def mix_kl(a, b, perm, coef, check_perm=True):
        p, q = a.float().softmax(1), target(b, perm, coef)
        return (-q * torch.log((p + 1e-16) / (q + 1e-16))).sum(1).mean()

    monkeypatch.setattr(O, "cat_mixed", cat_mixed)
    monkeypatch.setattr(O, "softmax_mix_mse", mix_mse)
    monkeypatch.setattr(O, "softmax_mix_kl_consistency", mix_kl)


def _first_iteration(reg, seed, monkeypatch, twin):
    with monkeypatch.context() as mp:
        th.replay_seeds(mp, [seed])
        if twin:
            _torch_twins(mp)
        with th.adam_gradients(mp) as grads:
            ep, model, teacher, opt, upd = build("float32", num_batches=1, reg=reg)
            ep._TAPE_DEFAULT = False
            per_step = th.keep_records(ep)
            ep.run()
        torch.cuda.synchronize()
        named = {n: (opt.flat.offset_of(p), p.numel()) for n, p in model.named_parameters()}
        return per_step[0], grads[0].cpu(), named, ep._mix


@pytest.mark.parametrize("reg", ["mse", "kl"])
def test_first_iteration_matches_the_unfused_twin(reg, monkeypatch):
    """fp32, 64 x 64, LB = 2, UB = 3, a 3-cycle: the iteration with the three kernels against the same iteration with torch
    expressions in their place (same U-Net kernels, same teacher), at the step-1 bounds of
    test_gpu_meanteacher.py::test_epocher_matches_the_reference_run."""
    seed, lam, perm = _cycle_seed(ICT["UB"], ICT["mix_alpha"])
    got, grad, named, mix = _first_iteration(reg, seed, monkeypatch, twin=False)
    ref, grad_ref, named_ref, mix_ref = _first_iteration(reg, seed, monkeypatch, twin=True)
    assert mix == mix_ref == (lam, 1.0 - lam) and named == named_ref
    np.testing.assert_allclose(got["sup_loss"], ref["sup_loss"], rtol=2e-5)
    np.testing.assert_allclose(got["reg_loss"], ref["reg_loss"], rtol=2e-4)
    assert ref["reg_loss"] > 0
    worst = {}
    for n, (off, numel) in named.items():
        x, y = th.sampled(grad, off, numel, f"ict/grad/{n}"), th.sampled(grad_ref, off, numel, f"ict/grad/{n}")
        worst[n] = float(np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-30))
    print(f"\nICT twin {reg}: sup {got['sup_loss']:.9g} / {ref['sup_loss']:.9g}, reg {got['reg_loss']:.9g} / {ref['reg_loss']:.9g}, "
          f"worst gradient rel L2 {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
    assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
    tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
    assert tail[len(tail) // 2] < 5e-3 and tail[-1] < 1.5e-2, tail
    assert max(worst.values()) < 3e-2, worst


# ---------------------------------------------------------------------------------------------------------------- 8. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.num_batches=2", "Data.size=64", "Data.name=synthetic", "LabeledData.batch_size=2",
         "UnlabeledData.batch_size=3", "ICTParameters.mix_alpha=0.5"]


def test_main_cli_trains_resumes_and_infers_with_the_teacher(golden):
    save = f"pytest_cli_ict_{os.getpid()}"
    run_dir = th.run_dir(save)
    dirs = [run_dir, th.run_dir(save + "_resume"), th.run_dir(save + "_inf")]
    for d in dirs:
        shutil.rmtree(d, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=ict", f"Trainer.save_dir={save}", "Trainer.max_epoch=2"] + _TINY)
        ref = sorted(str(x) for x in golden("trainer_io")["partial/tree_last_pth"])
        for name in ("last.pth", "best.pth"):
            lines = th.checkpoint_tree(os.path.join(run_dir, name))
            # the meanteacher tree: the partial trainer's, the consistency criterion, the teacher (a second _model), the updater and the
            # reg_weight history
            mine = th.own_lines_removed(lines, ("_reg_criterion", "_teacher_model/", "_ema_updater/", "_storage/tra_reg_weight"))
            if name == "last.pth":        # (best.pth may be the first epoch's: a shorter history)
                assert mine == ref, (sorted(set(mine) - set(ref))[:12], sorted(set(ref) - set(mine))[:12])
            assert {l.split("/")[0].split(" ")[0] for l in mine} == {l.split("/")[0].split(" ")[0] for l in ref}, name
            assert sorted(l.replace("_teacher_model/", "_model/", 1) for l in lines if l.startswith("_teacher_model/")) == \
                sorted(l for l in lines if l.startswith("_model/"))
            assert any(l.startswith("_ema_updater/") for l in lines) and any(l.startswith("_storage/tra_reg_weight") for l in lines)
            assert any(l.startswith("_reg_criterion") for l in lines)
        sd = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert sd["_ema_updater"]["global_step"] == 4 and sd["_buffers"]["_cur_epoch"] == 1
        assert any(not torch.equal(sd["_teacher_model"][k], sd["_model"][k]) for k in sd["_model"] if "weight" in k)
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["ICTParameters"] == {"mix_alpha": 0.5}
        # a resume continues: one more epoch, the updater's call count goes on
        th.run_main(["Trainer.name=ict", f"Trainer.save_dir={save}_resume", "Trainer.max_epoch=3", f"Checkpoint={run_dir}/last.pth"] + _TINY)
        sd2 = torch.load(os.path.join(dirs[1], "last.pth"), map_location="cpu", weights_only=False)
        assert sd2["_ema_updater"]["global_step"] == 6 and sd2["_buffers"]["_cur_epoch"] == 2
        # inference evaluates the teacher: a checkpoint whose student is scrambled scores the same
        score = th.run_inference(["Trainer.name=ict", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "last.pth"))
        assert 0.0 <= score <= 1.0
        scrambled = dict(sd, _model={k: (torch.randn_like(v) if v.is_floating_point() else v) for k, v in sd["_model"].items()})
        torch.save(scrambled, os.path.join(run_dir, "scrambled.pth"))
        assert th.run_inference(["Trainer.name=ict", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "scrambled.pth")) == score
    finally:
        for d in dirs:
            shutil.rmtree(d, ignore_errors=True)
