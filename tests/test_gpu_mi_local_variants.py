"""GPU: every fp32 kernel variant of the local-MI contraction (csrc/mi_local.hip), and the plain-bf16 kernels, once per row of
tests/mi_local_ref.py::VARIANT_CASES -- exactly on integer inputs (any summation order gives the same bits) and against the float64
oracle on peaked, correlated inputs.  Which variant a row reaches is the library's own answer (miseg_iic_local_joint_plan /
miseg_iic_local_bwd_plan, checked on the CPU by test_cpu_mi_local_plan.py); shapes, windows, inputs and references: mi_local_ref.py.

Bounds (none from a kernel's output): the raw joint 1e-5 of the oracle's largest entry; the loss 4 x the fp32 oracle's own deviation
from float64 + 1e-7 and 1e-5 relative; gradients LOCAL_BWD_ATOL of the float64 gradient's largest entry -- the figures of
test_gpu_mi.py.  With MISEG_ERROR_DUMP=<dir> (the switch of test_gpu_mi_loss.py) the worst achieved error per row and quantity is written to
<dir>/mi_local_variants.json.

Measured on the MI355X, worst over both maps and both window sets (raw / loss relative / gradients, whole op and backward alone):
  K = 21 .. 32 on the direct forms (sb 2 .. 4): raw 1.3e-7 .. 2.5e-7, loss 6.7e-8 .. 3.0e-7, gradients 1.9e-6 .. 5.1e-6
  K = 12, pad 3 (bwd2<9>, atomics): raw 1.8e-7, loss 3.8e-7, gradients 6.0e-7;  controls: raw <= 2.3e-7, loss <= 3.1e-7, gradients <= 1.1e-6
  K = 39 .. 64 (forward only, sb 1 .. 7): raw 7.9e-8 .. 1.4e-7, loss 3.4e-8 .. 1.4e-7
  precision "bf16", K = 20, pad 1 | 3, against the rounded operands: raw 1.5e-7, gradients 3.9e-7 | 6.9e-7
Found by this file: local_loss_finish_kernel added the (2 pad + 1)^2 per-displacement terms serially in fp32 -- at pad 6 / 7 (169 / 225
terms of one sign) the whole-image loss of K = 60 / 58 was 2.5e-7 / 4.9e-7 off, outside 4 x the fp32 oracle's deviation + 1e-7; with the
total kept in double it is 7.6e-9 / 4.9e-8.
"""
import pytest
import torch

import mi_local_ref as M
import synth
import trainer_harness as th
from test_gpu_mi import LOCAL_BWD_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
_WORST = {}

ROWS_BOTH = [(name, k, pad, which) for name, k, pad in M.VARIANT_CASES for which in (("small", "walking") if k <= 32 else ("small",))]
ROWS_BWD = [r for r in ROWS_BOTH if r[1] <= 32]
_ids = lambda rows: [f"{r[0]}-{r[3]}" for r in rows]


def _ops():
    from miseg_amd import ops
    return ops


def _mi():
    from miseg_amd.ops import mi
    return mi


def _record(name, quantity, err):
    """Worst relative error per row and quantity; with MISEG_ERROR_DUMP=<dir> (the switch of test_gpu_mi_loss.py::_record) they are
    written there as mi_local_variants.json: the figures of the docstring above."""
    row = _WORST.setdefault(name, {})
    row[quantity] = max(row.get(quantity, 0.0), float(err))
    th.error_dump("mi_local", "variants", _WORST, sort_keys=True)


def _d(t):
    return None if t is None else t.to(DEV)


def _bwd(x, y, mask, pad, wins, grad_raw, scales, gx, gy):
    """miseg_iic_local_bwd through ops._local_bwd: accumulate = 0 for the single whole-image window, 1 otherwise."""
    from miseg_amd._rt import windows_tensor
    scale = torch.tensor(list(scales), dtype=torch.float32, device=DEV)
    _mi()._local_bwd(x, y, mask, pad, wins, windows_tensor(wins, x.device), grad_raw.contiguous(), scale, gx, gy)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _outside(shape, wins):
    """[1,1,H,W] bool: pixels in no window."""
    out = torch.ones(1, 1, shape[2], shape[3], dtype=torch.bool)
    for h0, h1, w0, w1 in wins:
        out[:, :, h0:h1, w0:w1] = False
    return out


def _exact_forward(shape, pad, precision, use_mask):
    d = M.int_inputs(shape, pad, 2)
    x, y = _d(d["x"]), _d(d["y"])
    for kind in ("whole", "crops"):
        wins = M.windows(shape[2], shape[3], kind)
        mask = d["mask"] if (use_mask and kind == "crops") else None
        raw = _ops().local_mi_raw_joint(x, y, pad, wins, mask=_d(mask), precision=precision)
        ref = M.ref_joint(d["x"], d["y"], pad, wins, mask)
        assert float(ref.abs().max()) > 0
        bad = (raw.cpu().double() != ref)
        assert not bool(bad.any()), (kind, int(bad.sum()), bad.nonzero()[:4].tolist())


def _exact_backward(shape, pad, use_mask):
    d = M.int_inputs(shape, pad, 2)
    x, y = _d(d["x"]), _d(d["y"])
    # accumulate = 0 on the whole image: every pixel written (the outputs start as NaN), bit equality
    wins = M.windows(shape[2], shape[3], "whole")
    gx, gy = torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))
    _bwd(x, y, None, pad, wins, _d(d["G"][:1]), (1.0,), gx, gy)
    rx, ry = M.ref_bwd(d["x"], d["y"], pad, wins, d["G"][:1], (1.0,))
    assert float(rx.abs().max()) > 0 and float(ry.abs().max()) > 0
    assert torch.equal(gx.cpu().double(), rx) and torch.equal(gy.cpu().double(), ry)
    # accumulate = 1 on the two crops, into prefilled outputs
    wins = M.windows(shape[2], shape[3], "crops")
    mask = d["mask"] if use_mask else None
    gx, gy = _d(d["prefill_x"]).clone(), _d(d["prefill_y"]).clone()
    _bwd(x, y, _d(mask), pad, wins, _d(d["G"]), M.SCALES, gx, gy)
    rx, ry = M.ref_bwd(d["x"], d["y"], pad, wins, d["G"], M.SCALES, mask)
    keep = _outside(shape, wins) if mask is None else (_outside(shape, wins) | (mask == 0))
    for got, ref, pre in ((gx, rx, d["prefill_x"]), (gy, ry, d["prefill_y"])):
        got = got.cpu()
        assert float(ref.abs().max()) > 0
        assert torch.equal(got.double(), pre.double() + ref)
        sel = keep.expand_as(got)
        assert torch.equal(_bits(got)[sel], _bits(pre)[sel])        # outside both windows / where the mask is 0: the prefill's bits


# ----------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("name,k,pad,which", ROWS_BOTH, ids=_ids(ROWS_BOTH))
def test_forward_is_exact_on_integers(name, k, pad, which):
    _exact_forward(M.shape_of(k, pad, which), pad, "fp32", True)


@pytest.mark.parametrize("name,k,pad,which", ROWS_BWD, ids=_ids(ROWS_BWD))
def test_backward_is_exact_on_integers(name, k, pad, which):
    _exact_backward(M.shape_of(k, pad, which), pad, True)


# ----------------------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("name,k,pad,which", ROWS_BOTH, ids=_ids(ROWS_BOTH))
def test_forward_vs_float64(name, k, pad, which):
    shape = M.shape_of(k, pad, which)
    x, y, mask = M.real_inputs(shape)
    for kind in ("whole", "crops"):
        wins = M.windows(shape[2], shape[3], kind)
        m = mask if kind == "crops" else None
        raw = _ops().local_mi_raw_joint(_d(x), _d(y), pad, wins, mask=_d(m))
        ref = M.real_reference(shape, pad, kind)["raw"]
        for p in range(len(wins)):
            err = float((raw[p].cpu().double() - ref[p]).abs().max() / ref[p].abs().max())
            print(f"\n{name} {which} {kind}[{p}]: raw {err:.2e}", end="")
            _record(name, "raw", err)
            assert err <= 1e-5, (kind, p, err)


def _check_loss(name, loss, ref, tag):
    for p in range(ref["loss"].numel()):
        got, truth, dev32 = float(loss[p]), float(ref["loss"][p]), abs(float(ref["loss_fp32"][p]) - float(ref["loss"][p]))
        rel = abs(got - truth) / abs(truth)
        print(f"\n{name} {tag}[{p}]: loss {got:.7e} truth {truth:.7e} rel {rel:.2e} abs {abs(got - truth):.2e} (fp32 oracle {dev32:.2e})", end="")
        _record(name, "loss", rel)
        assert abs(got - truth) <= 4 * dev32 + 1e-7, (tag, p, got, truth, dev32)
        assert rel <= 1e-5, (tag, p, got, truth)


@pytest.mark.parametrize("name,k,pad,which", ROWS_BWD, ids=_ids(ROWS_BWD))
def test_whole_op_vs_float64(name, k, pad, which):
    shape = M.shape_of(k, pad, which)
    xs, ys, mask = M.real_inputs(shape)
    for kind in ("whole", "crops"):
        wins = M.windows(shape[2], shape[3], kind)
        m = mask if kind == "crops" else None
        ref = M.real_reference(shape, pad, kind)
        x, y = _d(xs).requires_grad_(True), _d(ys).requires_grad_(True)
        loss = _ops().local_mi_losses(x, y, pad, wins, mask=_d(m))
        (loss * torch.tensor(M.scales_for(wins), device=DEV)).sum().backward()
        for tag, got, r in (("gx", x.grad, ref["gx"]), ("gy", y.grad, ref["gy"])):
            err = float((got.cpu().double() - r).abs().max() / r.abs().max())
            print(f"\n{name} {which} {kind}: {tag} {err:.2e}", end="")
            _record(name, "grad", err)
            assert err <= LOCAL_BWD_ATOL, (kind, tag, err)
        _check_loss(name, loss.detach().cpu(), ref, f"{which} {kind}")


@pytest.mark.parametrize("name,k,pad", M.FWD_ONLY_CASES, ids=[c[0] for c in M.FWD_ONLY_CASES])
def test_above_32_clusters_the_loss_holds_and_the_backward_refuses(name, k, pad):
    from miseg_amd import _cabi
    shape = M.small_shape(k, pad)
    xs, ys, mask = M.real_inputs(shape)
    for kind in ("whole", "crops"):
        wins = M.windows(shape[2], shape[3], kind)
        m = mask if kind == "crops" else None
        ref = M.real_reference(shape, pad, kind)
        x, y = _d(xs).requires_grad_(True), _d(ys).requires_grad_(True)
        loss = _ops().local_mi_losses(x, y, pad, wins, mask=_d(m))
        _check_loss(name, loss.detach().cpu(), ref, kind)
        with pytest.raises(_cabi.MisegError, match="K<=32"):
            loss.sum().backward()
        assert x.grad is None and y.grad is None
        again = _ops().local_mi_losses(x, y, pad, wins, mask=_d(m))          # the same buffers, a valid call: unharmed by the refusal
        assert torch.equal(again.detach(), loss.detach())


@pytest.mark.parametrize("name,k,pad,which", ROWS_BWD, ids=_ids(ROWS_BWD))
def test_backward_alone_vs_float64(name, k, pad, which):
    """Real d loss / d raw, mask, crops, scales, accumulated into a prefill of the gradient's own magnitude."""
    shape = M.shape_of(k, pad, which)
    xs, ys, mask = M.real_inputs(shape)
    wins = M.windows(shape[2], shape[3], "crops")
    G = M.real_reference(shape, pad, "crops")["grad_raw"].float()
    rx, ry = M.ref_bwd(xs, ys, pad, wins, G, M.SCALES, mask)
    gscale = float(max(rx.abs().max(), ry.abs().max()))
    pre = [torch.from_numpy(synth.normal(f"mi_local/prefill/{name}/{which}/{t}", shape)) * gscale for t in "xy"]
    gx, gy = _d(pre[0]).clone(), _d(pre[1]).clone()
    _bwd(_d(xs), _d(ys), _d(mask), pad, wins, _d(G), M.SCALES, gx, gy)
    for tag, got, r, p0 in (("gx", gx, rx, pre[0]), ("gy", gy, ry, pre[1])):
        err = float((got.cpu().double() - (p0.double() + r)).abs().max() / r.abs().max())
        print(f"\n{name} {which}: {tag} {err:.2e}", end="")
        _record(name, "bwd_alone", err)
        assert err <= LOCAL_BWD_ATOL, (tag, err)


# ----------------------------------------------------------------------------------------------------------------- heads wrapper
@pytest.mark.parametrize("name,k,pad", M.HEADS_CASES, ids=[c[0] for c in M.HEADS_CASES])
def test_heads_wrapper_equals_per_head_calls(name, k, pad):
    """ops.local_mi_heads (S = 2, with and without a mask) against one ops.local_mi_losses per sub-head: the same kernels on the same
    operands, bit for bit (as test_gpu_mi.py::test_local_mi_heads_equals_per_head_calls, on an sb = 2 forward and a direct<2> backward)."""
    n, _, h, w = M.small_shape(k, pad)
    s, ub = 2, n
    base = torch.from_numpy(synth.probs(f"mi_local/heads/{name}", (s * 2 * ub, k, h, w))).view(s, 2 * ub, k, h, w).to(DEV)
    mask = _d(M.real_inputs((n, k, h, w))[2])
    wts = torch.tensor([1.0, -2.0], device=DEV)
    for kind, m in (("whole", None), ("crops", mask)):
        wins = M.windows(h, w, kind)
        a = base.clone().requires_grad_(True)
        fused = _ops().local_mi_heads(a, ub, pad, wins, mask=m)                       # [S, P]
        (fused * wts[:, None]).sum().backward()
        b = base.clone().requires_grad_(True)
        loop = torch.stack([_ops().local_mi_losses(q[:ub], q[ub:], pad, wins, mask=m) for q in b])
        (loop * wts[:, None]).sum().backward()
        assert torch.equal(fused.detach(), loop.detach())
        assert float(b.grad.abs().max()) > 0 and torch.equal(a.grad, b.grad)


# ----------------------------------------------------------------------------------------------------------------- precision "bf16"
@pytest.mark.parametrize("name,k,pad", M.BF16_CASES, ids=[c[0] for c in M.BF16_CASES])
@pytest.mark.parametrize("which", ["small", "walking"])
def test_plain_bf16_is_exact_on_integers(name, k, pad, which):
    """Every operand is exact in bf16 and every sum in fp32: forward (px kernel, one product) and backward (local_bwd_rows_kernel,
    NTERMS = 1) give the integer oracle's bits.  No mask: a mask sends the call to the fp32 kernels."""
    shape = M.shape_of(k, pad, which)
    assert M.bwd_plan(*shape, pad, 1, False, "bf16").kind == M.ROWS
    _mi().set_mi_precision("bf16")
    try:
        _exact_forward(shape, pad, "bf16", False)
        _exact_backward(shape, pad, False)
    finally:
        _mi().set_mi_precision("fp32")


@pytest.mark.parametrize("name,k,pad", M.BF16_CASES, ids=[c[0] for c in M.BF16_CASES])
@pytest.mark.parametrize("which", ["small", "walking"])
def test_plain_bf16_vs_float64_of_the_rounded_operands(name, k, pad, which):
    """Against the float64 contraction of the operands as the kernels round them (x, y and, in the backward, G to bf16 by
    f32_to_bf16_bits: round to nearest even) the plain-bf16 kernels owe what the fp32 kernels owe: products of bf16 values are exact
    in fp32, the sums are fp32 sums."""
    shape = M.shape_of(k, pad, which)
    xs, ys, _ = M.real_inputs(shape)
    xb, yb = M.to_bf16(xs), M.to_bf16(ys)
    _mi().set_mi_precision("bf16")
    try:
        for kind in ("whole", "crops"):
            wins = M.windows(shape[2], shape[3], kind)
            raw = _ops().local_mi_raw_joint(_d(xs), _d(ys), pad, wins, precision="bf16")
            ref = M.ref_joint(xb, yb, pad, wins)
            for p in range(len(wins)):
                err = float((raw[p].cpu().double() - ref[p]).abs().max() / ref[p].abs().max())
                print(f"\n{name} {which} {kind}[{p}]: raw {err:.2e}", end="")
                _record(name, "raw", err)
                assert err <= 1e-5, (kind, p, err)
        wins = M.windows(shape[2], shape[3], "crops")
        G = M.real_reference(shape, pad, "crops")["grad_raw"].float()
        rx, ry = M.ref_bwd(xb, yb, pad, wins, M.to_bf16(G), M.SCALES)
        gscale = float(max(rx.abs().max(), ry.abs().max()))
        pre = [torch.from_numpy(synth.normal(f"mi_local/prefill/{name}/{which}/{t}", shape)) * gscale for t in "xy"]
        gx, gy = _d(pre[0]).clone(), _d(pre[1]).clone()
        _bwd(_d(xs), _d(ys), None, pad, wins, _d(G), M.SCALES, gx, gy)
        for tag, got, r, p0 in (("gx", gx, rx, pre[0]), ("gy", gy, ry, pre[1])):
            err = float((got.cpu().double() - (p0.double() + r)).abs().max() / r.abs().max())
            print(f"\n{name} {which}: {tag} {err:.2e}", end="")
            _record(name, "bwd_alone", err)
            assert err <= LOCAL_BWD_ATOL, (tag, err)
    finally:
        _mi().set_mi_precision("fp32")
