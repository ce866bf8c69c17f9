"""GPU: the cross pseudo supervision trainer (``Trainer.name=cps``) -- its kernel (csrc/cps.hip:
``miseg_softmax_cross_pseudo``) against the float64 restatement of tests/cps_ref.py (checked on the CPU by test_cpu_cps.py), its tie
rule, its optional arguments, its refusals, its launch-tape replay, the step under the tape, the step against its unfused twin, the
CLI and two data-parallel ranks.

Kernel: every entry of ``pixel_ref.LOSS_CASES`` (all class counts x logit scales, a short block, exactly one block, the grid-stride
shape) with ``(a, b) = pixel_ref.case_inputs("mse", name)``.  Bounds are pixel_ref's, for both losses and both gradients:
|loss - ref| <= 1e-5 |ref|, max|grad - ref| <= 1e-5 max|ref|; ``agree`` is compared exactly (test_cpu_cps.py shows that no pixel of
these cases is a tie).  Ties: ``pixel_ref.tie_logits``, 3 x 19 x 23, C = 3, 4, 16.

Worst measured error over every case compared with a reference, as a fraction of the bound (run with -s: every case prints its
figures, test_zz_worst_errors the worst ones and, with MISEG_ERROR_DUMP, writes them):
  loss: error / bound                        gradient: max error / bound
  0.012  (short_c16, cps_b: 4.8e-07 of 4.115)  0.032  (c16_s12, gb: 2.5e-10, max|ref| 7.6e-04)
(MI355X, library 419.)  No case needed a bound of its own.

Launch tape: this module registers the replay case of the new entry point in ``test_gpu_tape_entry_points.CASES`` when it is imported
(no GPU needed for that), replays it itself and adds the recorded name; it sorts before test_gpu_tape_entry_points.py, as
test_gpu_ict.py does and for the same reason.
"""
import functools
import math
import os
import shutil
import subprocess
import sys
import zlib
from itertools import chain

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cps_ref as R
import pixel_ref as P
import test_gpu_tape_entry_points as T
import trainer_harness as th
from trainer_harness import FEATURES, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
ENTRY = "miseg_softmax_cross_pseudo"
WORST = {"loss": [0.0, ""], "grad": [0.0, ""]}
SENTINEL = -12345.0


# ---------------------------------------------------------------------------------------------------------------- tape case (import time)
@T.case(ENTRY)
def _case_cross_pseudo(v):
    n, h, w = T.LOSS
    need = T.q("miseg_softmax_cross_pseudo_ws_bytes", n, h, w)
    return T.abi_case(ENTRY, dict(a=T.rn(n, h, w, 5, scale=3.0), b=T.rn(n, h, w, 5, scale=3.0), N=n, H=h, W=w, C=5, upstream=T.ru(1),
                                  loss=T.out(2), ga=T.out(n, h, w, 5), gb=T.out(n, h, w, 5), agree=T.out(1, dtype=T.I64), ws=T.ws(need),
                                  ws_bytes=need), rebind="b")


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


def wrapper_run(a, b, scales=(1.0, 1.0)):
    """(loss [2], grad of a, grad of b, agree) through the ops wrapper, the backward seeded with ``scales``; ``a`` and ``b`` device
    tensors in the layout under test."""
    a, b = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    loss, agree = ops().softmax_cross_pseudo(a, b)
    (scales[0] * loss[0] + scales[1] * loss[1]).backward()
    return loss.detach(), a.grad, b.grad, agree


def raw(a, b, upstream=None, want=("ga", "gb", "agree")):
    """One C-ABI call on NCHW-shaped CPU logits: (loss [2], ga, gb NCHW-shaped or None, agree [1] or None), all on the device."""
    n, c, h, w = a.shape
    a_d, b_d = dev_cl(a), dev_cl(b)
    need = cabi().query("miseg_softmax_cross_pseudo_ws_bytes", n, h, w)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    loss = torch.full((2,), float("nan"), device=DEV)
    ga, gb = (torch.full((n, c, h, w), float("nan"), device=DEV).contiguous(memory_format=CL) if k in want else None for k in ("ga", "gb"))
    agree = torch.full((1,), -7, dtype=torch.int64, device=DEV) if "agree" in want else None
    cabi().call(ENTRY, stream(), ptr(a_d), ptr(b_d), n, h, w, c, ptr(upstream), ptr(loss), ptr(ga), ptr(gb), ptr(agree), ptr(ws), need)
    torch.cuda.synchronize()
    return loss, ga, gb, agree


@functools.lru_cache(maxsize=None)
def reference(name):
    """((cps_a, cps_b), (ga, gb), agree) of a LOSS_CASES entry in float64; computed once, handed out as is."""
    return R.loss_grads_agree(*P.case_inputs("mse", name))


def check(tag, loss, grads, agree, ref, gscales=(1.0, 1.0)):
    (ref_a, ref_b), ref_grads, ref_agree = ref
    for side, got, want in (("a", float(loss[0]), float(ref_a)), ("b", float(loss[1]), float(ref_b))):
        err, bound = P.loss_error(got, want)
        print(f"\nCPS {tag:28s} cps_{side}={got:.9g} ref={want:.9g} err={err:.3e} (bound {bound:.3e})")
        if err / bound > WORST["loss"][0]:
            WORST["loss"] = [err / bound, f"{tag}/{side}: {err:.1e} of {want:.4g}"]
        assert math.isfinite(got) and err <= bound, (tag, side, "loss", err, bound)
    for side, got, want, s in zip("ab", grads, ref_grads, gscales):
        if got is None:
            continue
        err, bound = P.grad_error(got, want * s)
        print(f"CPS {tag:28s} grad_{side} err={err:.3e} (bound {bound:.3e}, max|ref|={float(want.abs().max()) * abs(s):.3e})")
        if err / bound > WORST["grad"][0]:
            WORST["grad"] = [err / bound, f"{tag}/{side}: {err:.1e}, max|ref| {float(want.abs().max()) * abs(s):.1e}"]
        assert bool(torch.isfinite(got).all()) and err <= bound, (tag, side, "grad", err, bound)
    if agree is not None:
        assert int(agree) == ref_agree, (tag, int(agree), ref_agree)


# ---------------------------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_cross_pseudo_vs_float64(name):
    a, b = P.case_inputs("mse", name)
    loss, ga, gb, agree = wrapper_run(dev_cl(a), dev_cl(b))
    assert agree.dtype == torch.int64 and tuple(agree.shape) == (1,) and tuple(loss.shape) == (2,)
    check(name, loss, (ga, gb), agree, reference(name))


def test_zz_worst_errors():
    for what, (worst, where) in WORST.items():
        print(f"\nCPS WORST {what:5s} {worst:.3f} of its bound ({where})")
    th.error_dump("cps", "worst", {k: {"fraction_of_bound": v[0], "case": v[1]} for k, v in WORST.items()})
    assert all(v[0] <= 1.0 for v in WORST.values())


# ---------------------------------------------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("c", [3, 4, 16])
def test_ties_go_to_the_first_maximum(c):
    """Logits from {-1, -0.0, 0.0, 1}: the labels a gradient implies (its one negative entry) are numpy.argmax's at every pixel."""
    a, b = P.tie_logits(f"cps/tie/a{c}", 3, c, 19, 23), P.tie_logits(f"cps/tie/b{c}", 3, c, 19, 23)
    ref = R.loss_grads_agree(a, b)
    loss, ga, gb, agree = raw(a, b)
    assert torch.equal(R.implied_labels(ga), P.first_argmax(b)) and torch.equal(R.implied_labels(gb), P.first_argmax(a))
    check(f"tie_c{c}", loss, (ga, gb), agree, ref)
    assert 0 < int(agree) < 3 * 19 * 23
    loss, ga, gb, agree = raw(a, a.clone())
    assert int(agree) == 3 * 19 * 23 and torch.equal(P.bits(ga), P.bits(gb)) and torch.equal(P.bits(loss[:1]), P.bits(loss[1:]))
    check(f"tie_c{c} a==b", loss, (ga, gb), agree, R.loss_grads_agree(a, a.clone()))


# ---------------------------------------------------------------------------------------------------------------- 3. optional arguments
@pytest.mark.parametrize("name", ["c4_s2", "c3_s12", "c16_s30"])
def test_optional_outputs_leave_the_loss_bits_alone_and_two_calls_agree(name):
    a, b = P.case_inputs("mse", name)
    full = raw(a, b)
    again = raw(a, b)
    for x, y in zip(full, again):
        assert torch.equal(P.bits(x), P.bits(y))
    one_sided = raw(a, b, want=("ga", "agree"))
    assert one_sided[2] is None and torch.equal(P.bits(one_sided[1]), P.bits(full[1])) and torch.equal(P.bits(one_sided[0]), P.bits(full[0]))
    other_side = raw(a, b, want=("gb",))
    assert other_side[1] is None and other_side[3] is None and torch.equal(P.bits(other_side[2]), P.bits(full[2]))
    bare = raw(a, b, want=())
    assert bare[1] is None and bare[2] is None and bare[3] is None
    assert torch.equal(P.bits(other_side[0]), P.bits(full[0])) and torch.equal(P.bits(bare[0]), P.bits(full[0]))
    check(f"{name} raw", full[0], full[1:3], full[3], reference(name))
    with torch.no_grad():
        loss, agree = ops().softmax_cross_pseudo(dev_cl(a), dev_cl(b))
    assert not loss.requires_grad and torch.equal(P.bits(loss), P.bits(full[0])) and int(agree) == int(full[3])


def test_upstream_through_autograd_and_through_the_device_pointer():
    a, b = P.case_inputs("mse", "c5_s2")
    ref = reference("c5_s2")
    loss, ga, gb, agree = wrapper_run(dev_cl(a), dev_cl(b), scales=(-2.5, 0.75))       # loss[0]'s scale reaches a only, loss[1]'s b only
    check("c5_s2 autograd (-2.5, 0.75)", loss, (ga, gb), agree, ref, gscales=(-2.5, 0.75))
    for value in (0.375, -3.0):
        up = torch.tensor([value], device=DEV)
        loss, ga, gb, agree = raw(a, b, upstream=up)
        check(f"c5_s2 upstream {value}", loss, (ga, gb), agree, ref, gscales=(value, value))


def test_plain_nchw_and_channels_last_inputs_agree_bit_for_bit():
    """Contiguous NCHW goes through the wrapper's conversion, channels-last does not; C = 3 so that the two layouts differ."""
    a, b = P.case_inputs("mse", "c3_s2")
    plain = wrapper_run(a.to(DEV).contiguous(), b.to(DEV).contiguous())
    cl = wrapper_run(dev_cl(a), dev_cl(b))
    for x, y in zip(plain, cl):
        assert torch.equal(P.bits(x), P.bits(y))
    check("c3_s2 nchw", plain[0], plain[1:3], plain[3], reference("c3_s2"))


def test_split_rows_parts_write_their_own_rows():
    """Operands that are parts of a split_rows: the unlabeled parts alone (``on_labeled: false``: the other rows get zeros), all parts as
    one batch (``on_labeled: true``), and the whole batch next to a supervised loss on the labeled part, whose rows then hold the sum."""
    a, b = P.case_inputs("mse", "c4_s2")                 # 3 x 19 x 23, C = 4: rows [0, 1) labeled, [1, 3) unlabeled
    labels = P.labels("cps/split/t", 1, 19, 23, 4)
    o = ops()

    def leaves():
        return dev_cl(a).requires_grad_(True), dev_cl(b).requires_grad_(True)

    # the unlabeled rows only
    x, y = leaves()
    (x0, x1), (y0, y1) = o.split_rows(x, [1, 2]), o.split_rows(y, [1, 2])
    loss, agree = o.softmax_cross_pseudo(x1, y1)
    (2.0 * loss[0] - 0.5 * loss[1]).backward()
    ref = R.loss_grads_agree(a[1:], b[1:])
    check("split unlabeled", loss.detach(), (x.grad[1:], y.grad[1:]), agree, ref, gscales=(2.0, -0.5))
    assert not bool(x.grad[:1].any()) and not bool(y.grad[:1].any())
    assert x.grad.is_contiguous(memory_format=CL)
    # all parts as one batch: the bits of the unsplit call
    whole = wrapper_run(dev_cl(a), dev_cl(b), scales=(2.0, -0.5))
    x, y = leaves()
    loss, agree = o.softmax_cross_pseudo(o.split_rows(x, [1, 2]), o.split_rows(y, [1, 2]))
    (2.0 * loss[0] - 0.5 * loss[1]).backward()
    for got, want in zip((loss, x.grad, y.grad, agree), whole):
        assert torch.equal(P.bits(got), P.bits(want))
    # ... and beside a supervised loss on the labeled part, in either order of the two calls
    kl_loss, kl_grad = P.value_and_grad("kl", a[:1], labels)
    (ref_a, ref_b), (ref_ga, ref_gb), _ = reference("c4_s2")
    want = 1.5 * ref_ga
    want[:1] += 3.0 * kl_grad
    for cross_first in (False, True):
        x, y = leaves()
        xs, ys = o.split_rows(x, [1, 2]), o.split_rows(y, [1, 2])
        if cross_first:
            loss, _ = o.softmax_cross_pseudo(xs, ys)
        sup = o.softmax_kl(xs[0], labels.to(DEV))
        if not cross_first:
            loss, _ = o.softmax_cross_pseudo(xs, ys)
        torch.autograd.backward([sup, loss], [torch.full((), 3.0, device=DEV), torch.tensor([1.5, 1.5], device=DEV)])
        err, bound = P.grad_error(x.grad, want)
        print(f"\nCPS split + kl (cross first: {cross_first}) grad err={err:.3e} (bound {bound:.3e})")
        assert err <= bound, (cross_first, err, bound)
        err, bound = P.grad_error(y.grad, 1.5 * ref_gb)
        assert err <= bound, (cross_first, err, bound)
        assert abs(float(sup.detach()) - float(kl_loss)) <= P.LOSS_REL * abs(float(kl_loss))


def test_wrapper_refuses_what_it_cannot_read_in_place():
    a, b = P.case_inputs("mse", "c4_s2")
    with pytest.raises(TypeError, match="softmax_cross_pseudo"):
        ops().softmax_cross_pseudo(dev_cl(a).half(), dev_cl(b))
    with pytest.raises(TypeError, match="softmax_cross_pseudo"):
        ops().softmax_cross_pseudo(dev_cl(a), b)
    with pytest.raises(TypeError, match="adjacent"):
        ops().softmax_cross_pseudo((dev_cl(a[:1]), dev_cl(a[1:])), dev_cl(b))


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing_and_write_nothing():
    from miseg_amd._cabi import MisegError
    n, h, w, c = 3, 19, 23, 4
    need = cabi().query("miseg_softmax_cross_pseudo_ws_bytes", n, h, w)
    assert need == 16 * P.loss_blocks(n * h * w)
    a, b = torch.randn(n, h, w, c, device=DEV), torch.randn(n, h, w, c, device=DEV)
    a0, b0 = a.clone(), b.clone()
    loss = torch.full((2,), SENTINEL, device=DEV)
    ga, gb = torch.full((n, h, w, 16), SENTINEL, device=DEV), torch.full((n, h, w, 16), SENTINEL, device=DEV)
    agree = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((loss == SENTINEL).all()) and bool((ga == SENTINEL).all()) and bool((gb == SENTINEL).all()) and int(agree) == 77 and \
            bool((ws == 0x5A).all()) and torch.equal(a, a0) and torch.equal(b, b0)

    good = dict(a=a, b=b, N=n, H=h, W=w, C=c, loss=loss, ga=ga, gb=gb, ws=ws, ws_bytes=need)
    refusals = [dict(C=k) for k in P.REFUSED_CLASS_COUNTS] + [
        dict(N=0), dict(H=0), dict(W=0), dict(ws_bytes=need - 1), dict(a=None), dict(b=None), dict(loss=None), dict(ws=None),
        dict(ws=ws[4:]),                                                      # a workspace off the 8-byte boundary
        dict(ga=a), dict(ga=b), dict(gb=a), dict(gb=b), dict(gb=ga),          # a gradient on top of an operand, or of the other gradient
        dict(ga=a.view(-1)[4:])]                                              # ... or overlapping it in part
    for change in refusals:
        k = {**good, **change}
        with pytest.raises(MisegError):
            cabi().call(ENTRY, stream(), ptr(k["a"]), ptr(k["b"]), k["N"], k["H"], k["W"], k["C"], None, ptr(k["loss"]), ptr(k["ga"]), ptr(k["gb"]),
                        ptr(agree), ptr(k["ws"]), k["ws_bytes"])
        assert untouched(), change
    assert cabi().query("miseg_softmax_cross_pseudo_ws_bytes", 0, h, w) == 0
    cabi().call(ENTRY, stream(), ptr(a), ptr(b), n, h, w, c, None, ptr(loss), ptr(ga), ptr(gb), ptr(agree), ptr(ws), need)      # the good call goes through
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and 0 <= int(agree) <= n * h * w and bool((ws[need:] == 0x5A).all())


# ---------------------------------------------------------------------------------------------------------------- 5. tape, entry point
def test_replay_equals_eager():
    import tape_harness
    T._G.manual_seed(zlib.crc32(f"{ENTRY}/call".encode()))
    c = T.CASES[ENTRY](None)
    torch.cuda.synchronize()
    try:
        names = tape_harness.assert_replay_equals_eager(c)
    finally:
        torch.cuda.synchronize()
    assert ENTRY in names
    T.RECORDED.update(names)


# ---------------------------------------------------------------------------------------------------------------- 6. tape, step
CPS = dict(H=64, LB=2, UB=3, lr=1e-3, wd=1e-5, weight=1.5)


def build(dtype="float32", num_batches=3, on_labeled=True):
    """Two networks from different seeded states in one fused optimiser, synthetic device loaders."""
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from semi_seg.epocher import CPSEpocher
    from semi_seg.synthetic import SyntheticPairs
    model, model_b = th.unet(dtype, 31), th.unet(dtype, 32)
    opt = Adam(chain(model.parameters(), model_b.parameters()), lr=CPS["lr"], weight_decay=CPS["wd"])
    lab = SyntheticPairs(CPS["LB"], CPS["H"], 4, seed=0, device=DEV)
    unl = SyntheticPairs(CPS["UB"], CPS["H"], 4, seed=1, device=DEV)
    ep = CPSEpocher(model, model_b, opt, iter(lab), iter(unl), KL_div(verbose=False), CPS["weight"], num_batches, 0, DEV,
                    feature_position=FEATURES, feature_importance=th.IMPORTANCE, on_labeled=on_labeled)
    return ep, model, model_b, opt


def _both_networks(built):
    ep, model, model_b, opt = built
    assert opt.flat.total >= sum(p.numel() for p in chain(model.parameters(), model_b.parameters()))      # "param", "m", "v": both networks
    return {"bn_a": [b.detach().clone() for b in model.buffers()], "bn_b": [b.detach().clone() for b in model_b.buffers()]}


@pytest.mark.parametrize("dtype,on_labeled", [("float32", True), ("bfloat16", True), ("float16", True), ("float32", False)])
def test_cps_tape_replay_equals_eager_steps(dtype, on_labeled):
    """7 iterations: 2 eager + 1 recorded + 4 replayed give both networks' parameters, Adam's moments, both networks' BatchNorm buffers
    and the meters of 7 eager iterations, bit for bit.  A recording exists only if the iteration held no ATen launch."""
    def run(tape):
        return th.run_steps(lambda: build(dtype, on_labeled=on_labeled), 7, tape, mi_precision="fp32" if dtype == "float32" else "f16f8",
                            extra_state=_both_networks)
    got, info = run(True)
    ref, _ = run(False)
    th.assert_replayed(info, 4)
    names = info.op_names
    assert names.count(ENTRY) == 1, names
    assert "miseg_softmax_mse" not in names and "miseg_softmax_klcons" not in names and "miseg_ema_update" not in names
    assert names.count("miseg_softmax_kl") == 2 and names.count("miseg_cat_flipped") == 1, names
    assert "agreement" in got["meters"] and "sup_loss_b" in got["meters"]
    th.assert_same_state(got, ref, ("param", "m", "v", "bn_a", "bn_b", "meters"))


# ---------------------------------------------------------------------------------------------------------------- 7. step vs the unfused twin
def _torch_twin(monkeypatch):
    """The kernel as a materialised torch expression on the device."""
    from miseg_amd import ops as O

    def cross_pseudo(a, b, agree_out=None):
        a = torch.cat(list(a)) if isinstance(a, (tuple, list)) else a
        b = torch.cat(list(b)) if isinstance(b, (tuple, list)) else b
        ya, yb = a.detach().argmax(1), b.detach().argmax(1)
        loss = torch.stack([F.cross_entropy(a.float(), yb), F.cross_entropy(b.float(), ya)])
        agree = (ya == yb).sum().view(1)
        if agree_out is not None:
            agree_out.copy_(agree)
        return loss, agree

    monkeypatch.setattr(O, "softmax_cross_pseudo", cross_pseudo)


def _first_iteration(on_labeled, monkeypatch, twin):
    with monkeypatch.context() as mp:
        th.replay_seeds(mp, [5])
        if twin:
            _torch_twin(mp)
        with th.adam_gradients(mp) as grads:
            ep, model, model_b, opt = build("float32", num_batches=1, on_labeled=on_labeled)
            before = opt.flat.flat_param.detach().clone() if opt.flat.flat_param is not None else None
            ep._TAPE_DEFAULT = False
            per_step = th.keep_records(ep)
            res = th.meter_items(ep.run())
        torch.cuda.synchronize()
        named = {net: {n: (opt.flat.offset_of(p), p.numel()) for n, p in m.named_parameters()} for net, m in (("a", model), ("b", model_b))}
        agreement = [v for k, v in res.items() if k.startswith("agreement")]
        assert len(agreement) == 1
        moved = {net: [float((p.detach() - q.detach()).abs().max()) for p, q in zip(m.parameters(), th.unet("float32", seed).parameters())]
                 for net, m, seed in (("a", model, 31), ("b", model_b, 32))}
        differ = any(not torch.equal(p, q) for p, q in zip(model.parameters(), model_b.parameters()))
        return per_step[0], grads[0].cpu(), named, agreement[0], moved, differ


@pytest.mark.parametrize("on_labeled", [True, False])
def test_first_iteration_matches_the_unfused_twin(on_labeled, monkeypatch):
    """fp32, 64 x 64, LB = 2, UB = 3: the iteration with the kernel against the same iteration with ``F.cross_entropy(a, b.argmax(1)) +
    F.cross_entropy(b, a.argmax(1))`` in its place (same U-Net kernels, same states, hence the same logits and labels), at the bounds
    of test_gpu_ict.py::test_first_iteration_matches_the_unfused_twin, for the gradient slices of BOTH networks."""
    got, grad, named, agreement, moved, differ = _first_iteration(on_labeled, monkeypatch, twin=False)
    ref, grad_ref, named_ref, agreement_ref, _, _ = _first_iteration(on_labeled, monkeypatch, twin=True)
    assert named == named_ref
    np.testing.assert_allclose(got["sup_loss"], ref["sup_loss"], rtol=2e-5)
    np.testing.assert_allclose(got["sup_loss_b"], ref["sup_loss_b"], rtol=2e-5)
    np.testing.assert_allclose(got["reg_loss"], ref["reg_loss"], rtol=2e-4)
    assert ref["reg_loss"] > 0 and got["sup_loss"] != got["sup_loss_b"]
    assert 0.0 < agreement < 1.0 and agreement == agreement_ref
    for net in ("a", "b"):
        worst = {}
        for n, (off, numel) in named[net].items():
            x, y = th.sampled(grad, off, numel, f"cps/grad/{net}/{n}"), th.sampled(grad_ref, off, numel, f"cps/grad/{net}/{n}")
            worst[n] = float(np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-30))
        print(f"\nCPS twin on_labeled={on_labeled} network {net}: sup {got['sup_loss']:.9g} / {ref['sup_loss']:.9g}, reg {got['reg_loss']:.9g} / "
              f"{ref['reg_loss']:.9g}, agreement {agreement:.6f}, worst gradient rel L2 {max(worst.values()):.3e} ({max(worst, key=worst.get)})")
        assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
        tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
        assert tail[len(tail) // 2] < 5e-3 and tail[-1] < 1.5e-2, tail
        assert max(worst.values()) < 3e-2, worst
        assert max(moved[net]) > 0.0, net            # both networks have moved
    assert differ                                     # ... and network B's weights are not network A's


# ---------------------------------------------------------------------------------------------------------------- 8. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.num_batches=2", "Data.size=64", "Data.name=synthetic", "LabeledData.batch_size=2",
         "UnlabeledData.batch_size=3"]


def test_main_cli_trains_resumes_and_infers_with_network_a(golden):
    import re
    save = f"pytest_cli_cps_{os.getpid()}"
    run_dir = th.run_dir(save)
    dirs = [run_dir, th.run_dir(save + "_resume"), th.run_dir(save + "_inf")]
    for d in dirs:
        shutil.rmtree(d, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=cps", f"Trainer.save_dir={save}", "Trainer.max_epoch=2", "CPSParameters.weight=1.0"] + _TINY)
        ref = sorted(str(x) for x in golden("trainer_io")["partial/tree_last_pth"])
        n_params = 1 + max(int(m.group(1)) for l in ref for m in [re.search(r"^_optimizer/param_groups\[0\]/params\[(\d+)\]", l)] if m)

        def of_network_b(line):        # the optimiser's entries of network B's parameters: the indices behind network A's
            m = re.match(r"_optimizer/(?:state/(\d+)/|param_groups\[0\]/params\[(\d+)\])", line)
            return m is not None and int(m.group(1) or m.group(2)) >= n_params

        def shifted(line):
            return re.sub(r"(state/|params\[)(\d+)", lambda m: m.group(1) + str(int(m.group(2)) - n_params), line, count=1)

        for name in ("last.pth", "best.pth"):
            lines = th.checkpoint_tree(os.path.join(run_dir, name))
            # the partial trainer's tree, plus network B (a second _model, and its parameters' slots in the one optimiser) and three histories
            own = ("_model_b/", "_storage/tra_reg_weight", "_storage/tra_sup_loss_b", "_storage/tra_agreement")
            mine = sorted(l for l in th.own_lines_removed(lines, own) if not of_network_b(l))
            if name == "last.pth":        # (best.pth may be the first epoch's: a shorter history)
                assert mine == ref, (sorted(set(mine) - set(ref))[:12], sorted(set(ref) - set(mine))[:12])
            assert sorted(l.replace("_model_b/", "_model/", 1) for l in lines if l.startswith("_model_b/")) == \
                sorted(l for l in lines if l.startswith("_model/"))
            assert sorted(shifted(l) for l in lines if of_network_b(l)) == sorted(l for l in lines if l.startswith(("_optimizer/state/", "_optimizer/param_groups[0]/params[")) and not of_network_b(l))
            for history in own[1:]:
                assert any(l.startswith(history) for l in lines), history
        sd = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert sd["_buffers"]["_cur_epoch"] == 1
        assert any(not torch.equal(sd["_model_b"][k], sd["_model"][k]) for k in sd["_model"] if "weight" in k)
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["CPSParameters"] == {"weight": 1.0}
        # a resume continues: one more epoch, both networks from the checkpoint
        th.run_main(["Trainer.name=cps", f"Trainer.save_dir={save}_resume", "Trainer.max_epoch=3", f"Checkpoint={run_dir}/last.pth"] + _TINY)
        sd2 = torch.load(os.path.join(dirs[1], "last.pth"), map_location="cpu", weights_only=False)
        assert sd2["_buffers"]["_cur_epoch"] == 2
        assert any(not torch.equal(sd2["_model_b"][k], sd["_model_b"][k]) for k in sd["_model_b"] if "weight" in k)
        # inference evaluates network A: a checkpoint whose network B is scrambled scores the same
        score = th.run_inference(["Trainer.name=cps", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "last.pth"))
        assert 0.0 <= score <= 1.0
        scrambled = dict(sd, _model_b={k: (torch.randn_like(v) if v.is_floating_point() else v) for k, v in sd["_model_b"].items()})
        torch.save(scrambled, os.path.join(run_dir, "scrambled.pth"))
        assert th.run_inference(["Trainer.name=cps", f"Trainer.save_dir={save}_inf"] + _TINY, os.path.join(run_dir, "scrambled.pth")) == score
    finally:
        for d in dirs:
            shutil.rmtree(d, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- 9. two ranks
def test_two_ranks_train_both_networks_as_one_process_on_the_mean_gradient(tmp_path):
    """Two processes on the one GPU over gloo, each on its own data: after 2 steps both ranks hold the same parameters for both
    networks, bit for bit (the bound of test_gpu_meanteacher.py::test_two_ranks_keep_identical_teachers), and they are the parameters a
    single process reaches that computes the two ranks' gradients in turn and steps on their mean."""
    worker = os.path.join(ROOT, "tests", "_cps_ddp_worker.py")
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    base["MISEG_PROGRESS"] = "0"
    port = 36500 + os.getpid() % 2000
    procs = []
    try:
        for r in range(2):
            env = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MISEG_DDP_BACKEND="gloo")
            procs.append(subprocess.Popen([sys.executable, worker, "rank", str(tmp_path / f"r{r}.pt"), f"pytest_cps_ddp_{os.getpid()}_{r}"], env=env,
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs = [p.communicate(timeout=300)[0] for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0, o[-3000:]
        procs = [subprocess.Popen([sys.executable, worker, "reference", str(tmp_path / "ref.pt"), f"pytest_cps_ddp_{os.getpid()}_ref"], env=base,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)]
        out = procs[0].communicate(timeout=300)[0]
        assert procs[0].returncode == 0, out[-3000:]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1, ref = (torch.load(tmp_path / f"{n}.pt") for n in ("r0", "r1", "ref"))
    assert r0["steps"] == r1["steps"] == ref["steps"] == 2
    assert torch.equal(r0["init"], r1["init"]) and torch.equal(r0["init"], ref["init"])
    for net in ("a", "b"):
        lo, hi = r0["span"][net]
        assert r0["span"] == r1["span"] == ref["span"] and hi > lo
        assert torch.equal(r0["param"][lo:hi], r1["param"][lo:hi]), net
        assert not torch.equal(r0["param"][lo:hi], r0["init"][lo:hi]), net
        assert torch.equal(r0["param"][lo:hi], ref["param"][lo:hi]), (net, float((r0["param"][lo:hi] - ref["param"][lo:hi]).abs().max()))
    assert not torch.equal(r0["bn_a"], r1["bn_a"])          # each rank saw its own data: the running statistics stay rank-local
