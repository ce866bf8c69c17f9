"""The pixel-loss kernels (csrc/losses.hip: softmax_kl, softmax_mse, softmax_klcons, softmax_entropy, argmax_dice, flip) and the
batch-assembly kernels (cat_flip, cat_flip_pad, cat_flipped there; gather_rows, fill_zero, copy, assemble_rows at the end of
csrc/tape.hip) against the float64 references and case tables of tests/pixel_ref.py (checked on the CPU by test_cpu_pixel_ref.py).

Losses: every class count of MISEG_DISPATCH_C x logit scale (2, 12, 30) at 3 x 19 x 23 (five full blocks and one of 31 threads), a
short single block, exactly one block, the grid-stride loop (2 x 512 x 513 pixels > 2048 * 256), the fused flip replay with all four
masks, both memory layouts, upstream scaling through autograd and through the C ABI's device pointer, a null gradient pointer, edge
inputs, determinism, refusals that must write nothing, and labels outside [0, C).
Bounds (pixel_ref): |loss - ref| <= 1e-5 |ref| (<= 1e-7 where |ref| < 1e-6); max|grad - ref| <= 1e-5 max|ref|.  Everything else --
flip, the cat family, the byte movers, argmax, Dice counts, the zero gradient of a bad pixel -- is compared bit for bit.

Worst measured error per kernel over every case compared with a reference (MI355X, library 411; run with -s, every case prints its
own figures and test_zz_worst_errors the worst ones), as a fraction of the bound:
  kernel    loss: error / bound                         gradient: max error / bound
  kl        0.020  (c4_s30: 4.2e-06 of 20.87)           0.055  (c6_s30: 4.2e-10, max|ref| 7.6e-04)
  mse       0.013  (stride_c2: 3.5e-08 of 0.2603)       0.129  (c16_s2: 2.5e-11, max|ref| 1.9e-05)
  klcons    0.015  (c6_s2: 3.3e-07 of 2.123)            0.056  (c16_s12: 4.2e-10, max|ref| 7.6e-04)
  entropy   0.013  (c10_s2: 1.8e-07 of 1.357)           0.064  (c16_s12: 2.2e-10, max|ref| 3.5e-04)
No case needed a bound of its own.  split_rows + two scaled losses: gradient error <= 2.6e-09 against bounds >= 1.6e-08.
The whole module runs in about 5 s; the slowest case takes under a second.
"""
import math

import numpy as np
import pytest
import torch

import pixel_ref as P
from oracle import losses as OL

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
CL = torch.channels_last
WORST = {}


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
    """fp32 [N, C, H, W] on the device, NHWC memory."""
    return x.to(DEV).contiguous(memory_format=CL)


def masks_dev(masks):
    return None if masks is None else torch.tensor(list(masks), dtype=torch.int32, device=DEV)


def wrapper_run(kernel, a, second, flips=None, scale=None, **kw):
    """(loss tensor, gradient) through the ops wrapper; ``a`` a device tensor in the layout under test."""
    a = a.detach().clone().requires_grad_(True)
    o = ops()
    if kernel == "kl":
        loss = o.softmax_kl(a, second, **kw)
    elif kernel == "entropy":
        loss = o.softmax_entropy(a)
    else:
        loss = (o.softmax_mse if kernel == "mse" else o.softmax_kl_consistency)(a, second, flips)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), a.grad


def raw_call(kernel, a, second, n, h, w, c, flips=None, upstream=None, loss=None, grad=None, bad=None, ws=None, ws_bytes=None):
    """One C-ABI call of a loss entry point; every pointer as given (None = null)."""
    call = cabi().call
    if kernel == "kl":
        call("miseg_softmax_kl", stream(), ptr(a), ptr(second), n, h, w, c, ptr(upstream), ptr(loss), ptr(grad), ptr(bad), ptr(ws), ws_bytes)
    elif kernel == "entropy":
        call("miseg_softmax_entropy", stream(), ptr(a), n, h, w, c, ptr(upstream), ptr(loss), ptr(grad), ptr(ws), ws_bytes)
    else:
        call("miseg_softmax_mse" if kernel == "mse" else "miseg_softmax_klcons", stream(), ptr(a), ptr(second), ptr(flips), n, h, w, c,
             ptr(upstream), ptr(loss), ptr(grad), ptr(ws), ws_bytes)


def raw_run(kernel, a, second, flips=None, upstream=None, want_grad=True, sentinel=float("nan")):
    """The entry point on NCHW-shaped CPU inputs: (loss [1] device, grad NCHW-shaped device or None, bad [1] device)."""
    n, c, h, w = a.shape
    a_d = dev_cl(a)
    if kernel == "kl":
        s_d = second.to(DEV).contiguous()
    else:
        s_d = None if second is None else dev_cl(second)
    need = cabi().query("miseg_loss_ws_bytes", n, h, w)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), sentinel, device=DEV)
    grad = torch.full((n, c, h, w), sentinel, device=DEV).contiguous(memory_format=CL) if want_grad else None
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    raw_call(kernel, a_d, s_d, n, h, w, c, flips=flips, upstream=upstream, loss=loss, grad=grad, bad=bad, ws=ws, ws_bytes=need)
    torch.cuda.synchronize()
    return loss, grad, bad


def check(kernel, tag, loss, grad, ref_loss, ref_grad, gscale=1.0):
    el, bl = P.loss_error(float(loss), float(ref_loss))
    eg, bg = P.grad_error(grad, ref_grad * gscale)
    print(f"\nPIXEL {kernel:8s} {tag:28s} loss={float(loss):.9g} ref={float(ref_loss):.9g} err={el:.3e} (bound {bl:.3e})  "
          f"grad err={eg:.3e} (bound {bg:.3e}, max|ref|={float(ref_grad.abs().max()) * abs(gscale):.3e})")
    w = WORST.setdefault(kernel, [0.0, "", 0.0, ""])
    if el / bl > w[0]:
        w[0], w[1] = el / bl, tag
    if eg / bg > w[2]:
        w[2], w[3] = eg / bg, tag
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    assert el <= bl, (kernel, tag, "loss", el, bl)
    assert eg <= bg, (kernel, tag, "grad", eg, bg)


# ----------------------------------------------------------------------------- the four losses
@pytest.mark.parametrize("kernel", P.KERNELS)
@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_loss_kernels_vs_float64(name, kernel):
    a, second = P.case_inputs(kernel, name)
    ref_loss, ref_grad = P.case_reference(kernel, name)
    second_d = None if second is None else (second.to(DEV) if kernel == "kl" else dev_cl(second))
    loss, grad = wrapper_run(kernel, dev_cl(a), second_d)
    check(kernel, name, loss, grad, ref_loss, ref_grad)


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
@pytest.mark.parametrize("name", list(P.FLIP_CASES))
def test_flip_replay_vs_float64_on_the_materialised_flip(name, kernel):
    masks = P.FLIP_CASES[name][4]
    a, b = P.case_inputs(kernel, name)
    ref_loss, ref_grad = P.case_reference(kernel, name)
    loss, grad = wrapper_run(kernel, dev_cl(a), dev_cl(b), masks_dev(masks))
    check(kernel, name, loss, grad, ref_loss, ref_grad)
    if masks is not None:      # and the replay is not a no-op: without it the loss is another one
        plain, _ = wrapper_run(kernel, dev_cl(a), dev_cl(b), None)
        assert abs(float(plain) - float(ref_loss)) > 100 * P.LOSS_REL * abs(float(ref_loss))


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_plain_nchw_and_channels_last_inputs_agree_bit_for_bit(kernel):
    """Contiguous NCHW goes through the conversion of _logits_nhwc, channels-last does not; C = 3 so that the two layouts differ."""
    name = "c3_s12"
    a, second = P.case_inputs(kernel, name)
    ref_loss, ref_grad = P.case_reference(kernel, name)
    out = {}
    for layout in ("nchw", "cl"):
        conv = (lambda x: x.to(DEV).contiguous()) if layout == "nchw" else dev_cl
        second_d = None if second is None else (second.to(DEV) if kernel == "kl" else conv(second))
        x = conv(a)
        assert x.is_contiguous() == (layout == "nchw") and x.is_contiguous(memory_format=CL) == (layout == "cl")
        out[layout] = wrapper_run(kernel, x, second_d)
        check(kernel, f"{name}/{layout}", *out[layout], ref_loss, ref_grad)
    assert torch.equal(out["nchw"][0], out["cl"][0]) and torch.equal(out["nchw"][1], out["cl"][1])


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_upstream_scaling_and_null_gradient(kernel):
    """(0.37 loss).backward() through the wrapper scales the gradient only; the C ABI's `upstream` device scalar does the same inside the
    kernel and leaves the loss alone; a null gradient pointer gives the same loss bit for bit."""
    name = "c5_s2"
    a, second = P.case_inputs(kernel, name)
    ref_loss, ref_grad = P.case_reference(kernel, name)
    second_d = None if second is None else (second.to(DEV) if kernel == "kl" else dev_cl(second))
    loss, grad = wrapper_run(kernel, dev_cl(a), second_d, scale=0.37)
    check(kernel, f"{name}/0.37*loss", loss, grad, ref_loss, ref_grad, gscale=0.37)
    l1, g1, _ = raw_run(kernel, a, second)
    check(kernel, f"{name}/cabi", l1[0], g1, ref_loss, ref_grad)
    assert float(l1[0]) == float(loss)                                   # wrapper and C ABI: the same launch
    up = torch.tensor([-2.5], device=DEV)
    l2, g2, _ = raw_run(kernel, a, second, upstream=up)
    check(kernel, f"{name}/upstream=-2.5", l2[0], g2, ref_loss, ref_grad, gscale=-2.5)
    assert torch.equal(l2, l1)
    l3, g3, _ = raw_run(kernel, a, second, want_grad=False)
    assert g3 is None and torch.equal(l3, l1)


@pytest.mark.parametrize("kernel", P.KERNELS)
@pytest.mark.parametrize("name", ["c4_s12", "stride_c4"])
def test_two_calls_are_bit_identical(kernel, name):
    a, second = P.case_inputs(kernel, name)
    l1, g1, _ = raw_run(kernel, a, second)
    l2, g2, _ = raw_run(kernel, a, second)
    assert torch.equal(l1, l2) and torch.equal(P.bits(g1), P.bits(g2))


@pytest.mark.parametrize("c", [2, 4, 10, 16])
def test_edge_inputs(c):
    """All logits equal: entropy = log C, the consistency of a map with itself is 0 (the gradient there is judged against 1 / npix, the
    size of d loss / d logit for maps that differ: its reference is 0, a fraction of which bounds nothing).  Logits of +-1e4: nothing is
    NaN and the loss still matches.  A target class whose probability underflows to 0 in fp32: the per-pixel KL is -log(1e-16), the
    gradients are finite (and match)."""
    n, h, w = 3, 19, 23
    npix = n * h * w
    flat = torch.full((n, c, h, w), 0.75)
    for kernel in P.KERNELS:
        second = P.labels(f"edge/t{c}", n, h, w, c) if kernel == "kl" else (None if kernel == "entropy" else flat)
        loss, grad, _ = raw_run(kernel, flat, second)
        ref_loss, ref_grad = P.value_and_grad(kernel, flat, second)
        el, bl = P.loss_error(float(loss), float(ref_loss))
        eg = float((grad.cpu().to(F64) - ref_grad).abs().max())
        print(f"\nPIXEL {kernel:8s} equal_logits_c{c} loss={float(loss):.9g} ref={float(ref_loss):.9g} err={el:.3e} (bound {bl:.3e}) grad err={eg:.3e}")
        assert el <= bl and bool(torch.isfinite(grad).all())
        if kernel == "kl":
            assert eg <= P.GRAD_REL_OF_MAX * float(ref_grad.abs().max())
        else:
            assert eg <= P.GRAD_REL_OF_MAX / npix
        if kernel == "entropy":
            assert abs(float(loss) - math.log(c)) <= P.LOSS_REL * math.log(c)
        if kernel in ("mse", "klcons"):
            assert abs(float(loss)) <= P.LOSS_ABS_SMALL and float(ref_loss) == 0.0
    # a map with itself through the flip replay, ordinary logits
    a = P.logits(f"edge/self{c}", 4, c, 5, 7, 2)
    masks = (0, 1, 2, 3)
    b = OL.apply_flips(a, P.masks_to_decisions(masks))      # flip(b) == a
    for kernel in ("mse", "klcons"):
        loss, grad, _ = raw_run(kernel, a, b, flips=masks_dev(masks))
        assert abs(float(loss)) <= P.LOSS_ABS_SMALL and float(grad.abs().max()) <= P.GRAD_REL_OF_MAX / (4 * 5 * 7)
    # +-1e4
    big = torch.sign(P.logits(f"edge/big{c}", n, c, h, w)) * 1e4
    big_b = torch.sign(P.logits(f"edge/bigb{c}", n, c, h, w)) * 1e4
    for kernel in P.KERNELS:
        second = P.labels(f"edge/t{c}", n, h, w, c) if kernel == "kl" else (None if kernel == "entropy" else big_b)
        loss, grad, _ = raw_run(kernel, big, second)
        ref_loss, ref_grad = P.value_and_grad(kernel, big, second)
        el, bl = P.loss_error(float(loss), float(ref_loss))
        print(f"\nPIXEL {kernel:8s} logits_1e4_c{c} loss={float(loss):.9g} ref={float(ref_loss):.9g} err={el:.3e} (bound {bl:.3e})")
        assert not bool(torch.isnan(loss).any()) and not bool(torch.isnan(grad).any())
        assert bool(torch.isfinite(grad).all()) and el <= bl
    # the target's probability underflows: exp(-200) = 0 in fp32
    t = P.labels(f"edge/t{c}", n, h, w, c)
    z = torch.zeros(n, c, h, w).scatter_(1, t.unsqueeze(1), -200.0)
    loss, grad, bad = raw_run("kl", z, t)
    ref_loss, ref_grad = P.value_and_grad("kl", z, t)
    assert int(bad) == 0 and bool(torch.isfinite(grad).all())
    assert abs(float(loss) - (-math.log(1e-16))) <= P.LOSS_REL * 36.9 and abs(float(loss) - float(ref_loss)) <= P.LOSS_REL * float(ref_loss)
    assert float((grad.cpu().to(F64) - ref_grad).abs().max()) <= P.GRAD_REL_OF_MAX / npix


@pytest.mark.parametrize("kernel", P.KERNELS)
def test_refusals_write_nothing(kernel):
    """Unsupported class counts, an empty batch and a workspace one byte short are declined before anything is launched: the loss, the
    gradient and the flag, pre-filled with sentinels, are untouched."""
    E = cabi().MisegError
    n, h, w = 2, 5, 7
    need = cabi().query("miseg_loss_ws_bytes", n, h, w)
    ws = torch.zeros(max(need, 16) + 16, dtype=torch.uint8, device=DEV)

    def attempt(c, nn=n, ws_bytes=need):
        cc = max(c, 1)
        a = torch.zeros(n, h, w, cc, device=DEV)
        second = torch.zeros(n, h, w, dtype=torch.int64, device=DEV) if kernel == "kl" else (None if kernel == "entropy" else torch.zeros(n, h, w, cc, device=DEV))
        loss = torch.full((1,), float("nan"), device=DEV)
        grad = torch.full((n, h, w, cc), float("nan"), device=DEV)
        bad = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        with pytest.raises(E):
            raw_call(kernel, a, second, nn, h, w, c, loss=loss, grad=grad, bad=bad, ws=ws, ws_bytes=ws_bytes)
        torch.cuda.synchronize()
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(grad).all()) and int(bad) == -7 and int(ws.sum()) == 0

    for c in P.REFUSED_CLASS_COUNTS:
        attempt(c)
    attempt(4, nn=0, ws_bytes=need)
    assert need == 4 * P.loss_blocks(n * h * w)
    attempt(4, ws_bytes=need - 1)
    # (the same shape with the full workspace is accepted)
    loss = torch.full((1,), float("nan"), device=DEV)
    a = torch.zeros(n, h, w, 4, device=DEV)
    second = torch.zeros(n, h, w, dtype=torch.int64, device=DEV) if kernel == "kl" else (None if kernel == "entropy" else a)
    raw_call(kernel, a, second, n, h, w, 4, loss=loss, grad=None, bad=torch.zeros(1, dtype=torch.int32, device=DEV), ws=ws, ws_bytes=need)
    assert math.isfinite(float(loss))
    for c in P.REFUSED_CLASS_COUNTS:
        assert not ops().softmax_entropy_supported(c)


# ----------------------------------------------------------------------------- labels outside [0, C)
BAD_POSITIONS = ((0, 0, 0), (1, 9, 11), (2, 18, 22))       # the first, a middle and the last pixel of 3 x 19 x 23


@pytest.mark.parametrize("value", [-1, 4, 255])
def test_bad_labels_are_flagged_dropped_and_zeroed(value):
    """C = 4.  The kernel sets the flag; the bad pixels' gradient rows are exactly 0 (written: the buffer is pre-filled with NaN);
    every other gradient and the loss match the float64 reference that skips those pixels and keeps the divisor npix."""
    a = P.logits("bad/a", 3, 4, 19, 23, 2)
    t = P.labels("bad/t", 3, 19, 23, 4)
    clean_loss, _, clean_bad = raw_run("kl", a, t)
    assert int(clean_bad) == 0
    for positions in ([BAD_POSITIONS[0]], [BAD_POSITIONS[1]], [BAD_POSITIONS[2]], list(BAD_POSITIONS)):
        t2 = t.clone()
        for pos in positions:
            t2[pos] = value
        ref_loss, ref_grad = P.value_and_grad("kl", a, t2)
        loss, grad, bad = raw_run("kl", a, t2)
        assert int(bad) != 0
        for n_, h_, w_ in positions:
            assert torch.equal(P.bits(grad[n_, :, h_, w_]), torch.zeros(4, dtype=torch.int32)), (value, (n_, h_, w_), grad[n_, :, h_, w_])
        check("kl", f"bad_label_{value}@{len(positions)}", loss[0], grad, ref_loss, ref_grad)
        assert float(loss) != float(clean_loss)


@pytest.mark.parametrize("value", [-1, 4, 255])
def test_bad_labels_raise_like_class2one_hot_now_and_deferred(value):
    from miseg_amd import checks
    from semi_seg.epocher import _Pending
    a = dev_cl(P.logits("bad/a", 3, 4, 19, 23, 2))
    t = P.labels("bad/t", 3, 19, 23, 4)
    for pos in BAD_POSITIONS:
        t2 = t.clone()
        t2[pos] = value
        t2 = t2.to(DEV)
        with pytest.raises(AssertionError, match="4"):
            ops().softmax_kl(a.clone().requires_grad_(True), t2)
        loss, grad = wrapper_run("kl", a, t2, check_labels=False)          # does not raise; the gradient is clean
        ref_loss, ref_grad = P.value_and_grad("kl", a.cpu(), t2.cpu())
        check("kl", f"bad_label_{value}/unchecked", loss, grad, ref_loss, ref_grad)
        assert float(grad[pos[0], :, pos[1], pos[2]].abs().max()) == 0.0
        pend = _Pending()
        with checks.deferred(pend.checks):
            loss = ops().softmax_kl(a.clone().requires_grad_(True), t2)     # no exception yet
            pend.put("loss", loss)
        assert len(pend.checks) == 1
        flag = pend.checks[0][0]
        assert isinstance(flag, checks.LazyFlag) and flag.kind == "cast" and flag.tensor.dtype == torch.int32 and flag.tensor.numel() == 1
        with pytest.raises(AssertionError, match="4"):
            pend.fetch()
        assert pend.fetch() == {}
    # good labels: nothing raised either way, and the deferred flag reads zero
    pend = _Pending()
    with checks.deferred(pend.checks):
        pend.put("loss", ops().softmax_kl(a.clone().requires_grad_(True), t.to(DEV)))
    got = pend.fetch()
    assert abs(got["loss"] - float(ops().softmax_kl(a, t.to(DEV)))) == 0.0


# ----------------------------------------------------------------------------- argmax + Dice counts
def raw_dice(z, t, want_pred=True, adjacent=False, prefill=0):
    n, c, h, w = z.shape
    z_d = dev_cl(z)
    t_d = None if t is None else t.to(DEV).contiguous()
    pred = torch.full((n, h, w), -5, dtype=torch.int64, device=DEV) if want_pred else None
    inter = uni = None
    if t is not None:
        if adjacent:
            block = torch.full((2 * n * c,), prefill, dtype=torch.int64, device=DEV)
            inter, uni = block[:n * c].view(n, c), block[n * c:].view(n, c)
            assert uni.data_ptr() == inter.data_ptr() + n * c * 8
        else:
            inter = torch.full((n, c), prefill, dtype=torch.int64, device=DEV)
            pad = torch.empty(64, dtype=torch.int64, device=DEV)          # keeps the two allocations apart
            uni = torch.full((n, c), prefill, dtype=torch.int64, device=DEV)
            assert uni.data_ptr() != inter.data_ptr() + n * c * 8, pad.shape
    cabi().call("miseg_argmax_dice", stream(), ptr(z_d), ptr(t_d), n, h, w, c, ptr(pred), ptr(inter), ptr(uni))
    torch.cuda.synchronize()
    return pred, inter, uni


@pytest.mark.parametrize("name", list(P.DICE_CASES))
def test_argmax_dice_with_ties_bit_exact(name):
    n, h, w, c = P.DICE_CASES[name]
    z = P.tie_logits(f"{name}/z", n, c, h, w)
    t = P.labels(f"{name}/t", n, h, w, c)
    first = P.first_argmax(z)
    ri, ru = P.dice_bincount(first, t, c)
    oi, ou = OL.dice_counts(first, t, c)
    pred, inter, uni = ops().argmax_dice(dev_cl(z), t.to(DEV))
    assert torch.equal(pred.cpu(), dev_cl(z).cpu().max(1)[1]) and torch.equal(pred.cpu(), first)
    assert torch.equal(inter.cpu(), ri) and torch.equal(uni.cpu(), ru) and torch.equal(ri, oi) and torch.equal(ru, ou)
    # ordinary logits too (no ties), through the NCHW conversion
    z2 = P.logits(f"{name}/z2", n, c, h, w, 3)
    p2, i2, u2 = ops().argmax_dice(z2.to(DEV), t.to(DEV))
    ri2, ru2 = P.dice_bincount(P.first_argmax(z2), t, c)
    assert torch.equal(p2.cpu(), z2.max(1)[1]) and torch.equal(i2.cpu(), ri2) and torch.equal(u2.cpu(), ru2)
    # predictions only / counts only
    p3, i3, u3 = ops().argmax_dice(dev_cl(z), None)
    assert i3 is None and u3 is None and torch.equal(p3.cpu(), first)
    p4, i4, u4 = ops().argmax_dice(dev_cl(z), t.to(DEV), want_pred=False)
    assert p4 is None and torch.equal(i4.cpu(), ri) and torch.equal(u4.cpu(), ru)


@pytest.mark.parametrize("adjacent", [True, False])
def test_argmax_dice_memset_paths_and_no_accumulation(adjacent):
    """`inter` and `uni` back to back in one allocation (one fill) or apart (two): both start from garbage and a second call on the
    same buffers gives the same counts, not twice them."""
    n, h, w, c = P.DICE_CASES["dice_c5"]
    z, t = P.tie_logits("dice_c5/z", n, c, h, w), P.labels("dice_c5/t", n, h, w, c)
    first = P.first_argmax(z)
    ri, ru = P.dice_bincount(first, t, c)
    pred, inter, uni = raw_dice(z, t, adjacent=adjacent, prefill=0x0101010101010101)
    assert torch.equal(pred.cpu(), first) and torch.equal(inter.cpu(), ri) and torch.equal(uni.cpu(), ru)
    z_d, t_d = dev_cl(z), t.to(DEV)
    cabi().call("miseg_argmax_dice", stream(), ptr(z_d), ptr(t_d), n, h, w, c, None, ptr(inter), ptr(uni))
    torch.cuda.synchronize()
    assert torch.equal(inter.cpu(), ri) and torch.equal(uni.cpu(), ru)
    # want_pred = False through the C ABI left the sentinel alone; labels = None writes predictions only
    p_only, _, _ = raw_dice(z, None)
    assert torch.equal(p_only.cpu(), first)
    with pytest.raises(cabi().MisegError):
        cabi().call("miseg_argmax_dice", stream(), ptr(z_d), None, n, h, w, c, None, None, None)


def test_argmax_dice_out_of_range_labels_as_today():
    """A label outside [0, C): the prediction of that pixel is still counted in the union, the label adds to no class and to no
    intersection (pinned to what the kernel does; the reference's one-hot would assert)."""
    n, h, w, c = P.DICE_CASES["dice_c4"]
    z, t = P.tie_logits("dice_c4/z", n, c, h, w), P.labels("dice_c4/t", n, h, w, c).clone()
    for pos, v in zip(BAD_POSITIONS, (-1, c, 255)):
        t[pos] = v
    first = P.first_argmax(z)
    ri, ru = P.dice_bincount(first, t, c)
    pred, inter, uni = ops().argmax_dice(dev_cl(z), t.to(DEV))
    assert torch.equal(pred.cpu(), first) and torch.equal(inter.cpu(), ri) and torch.equal(uni.cpu(), ru)
    assert int(ru.sum()) == 2 * n * h * w - 3


# ----------------------------------------------------------------------------- flip
@pytest.mark.parametrize("shape", [(4, 3, 1, 7), (4, 3, 5, 1), (4, 2, 5, 7), (4, 1, 19, 23)])
def test_flip_degenerate_axes_all_masks_strided_input_and_backward(shape):
    masks = (0, 1, 2, 3)
    dec = P.masks_to_decisions(masks)
    fl = masks_dev(masks)
    x = P.bit_payload(f"flip/{shape}", shape, torch.int32)
    ref = OL.apply_flips(x, dec)
    out = ops().flip(x.to(DEV), fl)
    assert torch.equal(out.cpu(), ref)
    out = ops().flip(x.to(DEV).view(torch.float32), fl)
    assert torch.equal(P.bits(out), ref)
    # a strided, non-dense input
    n, c, h, w = shape
    wide = P.bit_payload(f"flip/wide/{shape}", (n, c, 2 * h, w), torch.int32)
    view = wide.to(DEV)[:, :, ::2]
    assert not view.is_contiguous() and tuple(view.shape) == shape
    assert torch.equal(ops().flip(view, fl).cpu(), OL.apply_flips(wide[:, :, ::2], dec))
    # backward of _Flip = the flip of the gradient, bit for bit
    xf = P.logits(f"flip/x/{shape}", *shape).to(DEV).requires_grad_(True)
    cot = P.bit_payload(f"flip/cot/{shape}", shape)
    y = ops().flip(xf, fl)
    assert y.requires_grad
    y.backward(cot.to(DEV))
    assert torch.equal(P.bits(xf.grad), OL.apply_flips(P.bits(cot), dec))


# ----------------------------------------------------------------------------- batch assembly
def raw_cat(entry, a, b, masks, three):
    """miseg_cat_flip / miseg_cat_flipped on int32 CPU tensors (a may be None: Na = 0, null pointer)."""
    nb, c, h, w = b.shape
    na = 0 if a is None else a.shape[0]
    out = torch.full(((na + (2 if three else 1) * nb), c, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    guard = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    a_d, b_d = None if a is None else a.to(DEV).contiguous(), b.to(DEV).contiguous()
    fl = masks_dev(masks)
    cabi().call(entry, stream(), ptr(a_d), na, ptr(b_d), nb, c, h, w, ptr(fl), ptr(out))
    torch.cuda.synchronize()
    assert bool((guard == 0x5A5A5A5A).all())
    return out.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32], ids=["f32", "i32"])
@pytest.mark.parametrize("name", list(P.CAT_CASES))
def test_cat_flip_and_cat_flipped_bit_exact(name, dtype):
    na, nb, c, h, w = P.CAT_CASES[name]
    masks = tuple((i + 1) % 4 for i in range(nb))                      # nb >= 3: at least three of the masks; 4: all four
    if nb >= 4:
        assert sorted(masks) == [0, 1, 2, 3]
    a, b = P.bit_payload(f"{name}/a", (na, c, h, w), torch.int32), P.bit_payload(f"{name}/b", (nb, c, h, w), torch.int32)
    ref3, ref2 = P.cat_flip_ref(a, b, masks), P.cat_flipped_ref(a, b, masks)
    fl = masks_dev(masks)
    cast = (lambda t: t.view(torch.float32)) if dtype == torch.float32 else (lambda t: t)
    out3 = ops().cat_flip(cast(a).to(DEV), cast(b).to(DEV), fl)
    out2 = ops().cat_flipped(cast(a).to(DEV), cast(b).to(DEV), fl)
    assert out3.dtype == dtype and out2.dtype == dtype
    assert torch.equal(P.bits(out3), ref3) and torch.equal(P.bits(out2), ref2)


def test_cat_family_remaining_masks_null_a_and_flipped_grid_stride():
    # the 3-sample case again with the mask the sweep above left out (0) first and 3 last
    na, nb, c, h, w = P.CAT_CASES["cat_2_3_1_5x7"]
    a, b = P.bit_payload("cat/a", (na, c, h, w), torch.int32), P.bit_payload("cat/b", (nb, c, h, w), torch.int32)
    for masks in ((0, 3, 1), (2, 0, 3)):
        assert torch.equal(raw_cat("miseg_cat_flip", a, b, masks, True), P.cat_flip_ref(a, b, masks))
        assert torch.equal(raw_cat("miseg_cat_flipped", a, b, masks, False), P.cat_flipped_ref(a, b, masks))
    # Na = 0 with a null `a`: C ABI only
    na, nb, c, h, w = P.CAT_CABI_CASE
    b = P.bit_payload("cat/b0", (nb, c, h, w), torch.int32)
    empty = torch.zeros((0, c, h, w), dtype=torch.int32)
    for masks in ((1, 2), (3, 0)):
        assert torch.equal(raw_cat("miseg_cat_flip", None, b, masks, True), P.cat_flip_ref(empty, b, masks))
        assert torch.equal(raw_cat("miseg_cat_flipped", None, b, masks, False), P.cat_flipped_ref(empty, b, masks))
    # cat_flipped's own grid-stride case
    na, nb, c, h, w = P.CAT_FLIPPED_GRID_STRIDE
    a, b = P.bit_payload("cat/ga", (na, c, h, w), torch.int32), P.bit_payload("cat/gb", (nb, c, h, w), torch.int32)
    masks = (3, 1, 2, 0)
    out = ops().cat_flipped(a.to(DEV), b.to(DEV), masks_dev(masks))
    assert torch.equal(out.cpu(), P.cat_flipped_ref(a, b, masks))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 19, 23)])
def test_cat_flip_pad_writes_the_batch_and_its_rounded_padded_copy(shape, dtype, monkeypatch):
    """`out` = the concatenation bit for bit; `_miseg_stem` = (dtype, pad [N, 8, H, W] NHWC) with channel 0 the round-to-nearest-even
    cast of `out` (the bits of `out.to(dtype)`, and of the CPU's conversion) and channels 1..7 zero.  Inputs: values that truncation and round-to-nearest
    round differently, finite values above 65504 (inf in half), half denormals, NaN, -0.0."""
    from miseg_amd import unet_ops
    monkeypatch.setattr(unet_ops, "_STEM_KERNELS", False)
    na, nb, h, w = shape
    masks = tuple((i + 1) % 4 for i in range(nb))
    a, b = P.rounding_image(f"pad/a/{shape}", na, h, w), P.rounding_image(f"pad/b/{shape}", nb, h, w)
    out = ops().cat_flip(a.to(DEV), b.to(DEV), masks_dev(masks), stem_dtype=dtype)
    ref = P.cat_flip_ref(P.bits(a), P.bits(b), masks)
    assert torch.equal(P.bits(out), ref)
    stem_dtype, pad = out._miseg_stem
    assert stem_dtype == dtype and pad.dtype == dtype and tuple(pad.shape) == (na + 2 * nb, 8, h, w) and pad.is_contiguous(memory_format=CL)
    got = pad.cpu()
    g0, src = P.bits(got[:, :1]).reshape(-1), ref.reshape(-1)

    def same_bits(want, where=None):      # on a mismatch: (fp32 bits in, 16 bits got, 16 bits wanted) of the first few
        w0 = P.bits(want).reshape(-1)
        bad = g0 != w0 if where is None else (g0 != w0) & where.reshape(-1)
        idx = bad.nonzero().reshape(-1)[:8]
        assert idx.numel() == 0, [(hex(int(src[i]) & 0xFFFFFFFF), hex(int(g0[i]) & 0xFFFF), hex(int(w0[i]) & 0xFFFF)) for i in idx]

    same_bits(out.to(dtype))                                           # the device's round-to-nearest-even cast of `out`, NaN included
    # and an independent conversion, the CPU's (its vectorised bf16 cast writes another NaN pattern, 0xFFFF: NaNs compared as NaNs)
    f32 = ref.view(torch.float32)
    want = f32.to(dtype)
    same_bits(want, ~torch.isnan(f32))
    assert torch.equal(torch.isnan(got[:, :1].float()), torch.isnan(f32)) and bool(torch.isnan(f32).any())
    assert torch.equal(P.bits(got[:, 1:]), torch.zeros_like(P.bits(got[:, 1:])))
    trunc = (ref >> 16).to(torch.int16)
    if dtype == torch.bfloat16:
        assert int((P.bits(got[:, :1]) != trunc).sum()) > 0            # (a truncating cast would have been seen)
    # with the stem's own kernels (the default) the plain cat_flip is taken: same `out`, no padded copy
    monkeypatch.setattr(unet_ops, "_STEM_KERNELS", True)
    out2 = ops().cat_flip(a.to(DEV), b.to(DEV), masks_dev(masks), stem_dtype=dtype)
    assert torch.equal(P.bits(out2), ref) and getattr(out2, "_miseg_stem", None) is None


def assemble_payload(tag, numel):
    x = P.logits(tag, 1, 1, 1, max(numel, 1))[0, 0, 0, :numel].clone()
    if numel >= 4:
        xi = x.view(torch.int32)
        xi[0], xi[1], xi[2], xi[-1] = -(1 << 31), 0x00000001, 0x7FC00000, 0x00400000     # -0.0, denormals, the quiet NaN
    return x


def raw_assemble(parts, guard=16):
    """[(src CPU fp32 or None, scale float or None, numel)] through miseg_assemble_rows: the output buffer (NaN-sentinel pre-filled),
    with `guard` floats behind its end."""
    total = sum(p[2] for p in parts)
    buf = torch.full((total + guard,), float("nan"), device=DEV)
    buf.view(torch.int32)[:] = 0x7FDEAD00
    keep, args = [], []
    for src, scale, numel in parts:
        s_d = None if src is None else src.to(DEV)
        k_d = None if scale is None else torch.tensor([scale], device=DEV)
        keep += [s_d, k_d]
        args += [ptr(s_d), ptr(k_d), numel]
    cabi().call("miseg_assemble_rows", stream(), ptr(buf), *args)
    torch.cuda.synchronize()
    return buf.cpu(), total


def test_assemble_rows_parts_scales_nulls_and_refusal():
    sizes = (4, 0, 1028)
    p0, p2 = assemble_payload("asm/p0", 4), assemble_payload("asm/p2", 1028)
    for parts in ([(p0, 0.37, 4), (None, None, 0), (p2, -2.5, 1028)],          # device scales, an empty middle part
                  [(p0, None, 4), (None, 3.0, 0), (p2, None, 1028)],           # null scales = 1: the source bit for bit
                  [(p2, 0.5, 1028), (None, 7.0, 1028), (p0, None, 4)],         # a null source gives zeros
                  [(None, None, 4), (p2, 1.5, 1028), (None, None, 1028)]):
        got, total = raw_assemble(parts)
        assert torch.equal(P.bits(got[:total]), P.bits(P.assemble_ref(parts)))
        assert bool((P.bits(got[total:]) == 0x7FDEAD00).all())
    got, total = raw_assemble([(p0, None, 4), (None, None, 0), (p2, None, 1028)])
    assert torch.equal(P.bits(got[:total]), torch.cat([P.bits(p0), P.bits(p2)]))
    assert sizes == (4, 0, 1028)
    # above 2048 * 256 float4: the grid-stride loop, part boundaries inside it
    big = assemble_payload("asm/big", P.ASSEMBLE_BIG)
    n0 = 4 * 1000
    parts = [(big[:n0], 0.37, n0), (None, None, 1028), (big[n0:P.ASSEMBLE_BIG - 1028].clone(), -1.25, P.ASSEMBLE_BIG - 1028 - n0)]
    got, total = raw_assemble(parts)
    assert total == P.ASSEMBLE_BIG and torch.equal(P.bits(got[:total]), P.bits(P.assemble_ref(parts)))
    assert bool((P.bits(got[total:]) == 0x7FDEAD00).all())
    # a part size that is no multiple of 4 floats: declined, nothing written
    for parts in ([(p0, None, 4), (p2, None, 1026), (None, None, 0)], [(p2, 2.0, 6), (None, None, 0), (None, None, 0)],
                  [(p0, None, 4), (None, None, 4), (p2, None, 1027)]):
        with pytest.raises(cabi().MisegError):
            raw_assemble(parts)
    buf = torch.full((64,), float("nan"), device=DEV)
    src = p2.to(DEV)
    with pytest.raises(cabi().MisegError):
        cabi().call("miseg_assemble_rows", stream(), ptr(buf), ptr(src), None, 6, None, None, 0, None, None, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize("chunk", [1, 5])
def test_gather_rows_equals_index_select(chunk):
    outer, n_src = 2, 7
    idx = [3, 0, 3, 6, 1, 1, 5, 0, 6]                                  # repeated and unordered
    src = P.bit_payload(f"gather/{chunk}", (outer, n_src, chunk))
    dst = torch.full((outer, len(idx), chunk), float("nan"), device=DEV)
    guard = torch.full((64,), float("nan"), device=DEV)
    src_d, idx_d = src.to(DEV), torch.tensor(idx, dtype=torch.int32, device=DEV)
    cabi().call("miseg_gather_rows", stream(), ptr(src_d), ptr(dst), outer, n_src, len(idx), ptr(idx_d), chunk)
    torch.cuda.synchronize()
    ref = P.bits(src).index_select(1, torch.tensor(idx))
    assert torch.equal(P.bits(dst), ref) and bool(torch.isnan(guard).all())
    with pytest.raises(cabi().MisegError):
        cabi().call("miseg_gather_rows", stream(), ptr(src_d), ptr(dst), outer, n_src, 0, ptr(idx_d), chunk)


@pytest.mark.parametrize("nbytes", P.BYTE_COUNTS)
def test_fill_zero_and_copy_byte_counts_tails_and_sentinels(nbytes):
    rs = np.random.RandomState(nbytes % 65521)
    src = torch.from_numpy(rs.randint(1, 256, nbytes + 64).astype(np.uint8)).to(DEV)       # no zero byte: a fill is told from a copy
    for op in ("fill", "copy"):
        dst = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
        if op == "fill":
            cabi().call("miseg_fill_zero", stream(), ptr(dst), nbytes)
        else:
            cabi().call("miseg_copy", stream(), ptr(dst), ptr(src), nbytes)
        torch.cuda.synchronize()
        want = torch.zeros(nbytes, dtype=torch.uint8, device=DEV) if op == "fill" else src[:nbytes]
        assert torch.equal(dst[:nbytes], want), op
        assert bool((dst[nbytes:] == 0xAB).all()), op                  # nothing behind the end
    # a pointer off the 16-byte boundary is declined and nothing is written; so is a misaligned source
    dst = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    E = cabi().MisegError
    with pytest.raises(E):
        cabi().call("miseg_fill_zero", stream(), ptr(dst) + 4, nbytes)
    with pytest.raises(E):
        cabi().call("miseg_copy", stream(), ptr(dst) + 8, ptr(src), nbytes)
    with pytest.raises(E):
        cabi().call("miseg_copy", stream(), ptr(dst), ptr(src) + 1, nbytes)
    cabi().call("miseg_fill_zero", stream(), ptr(dst) + 4, 0)            # an empty range is a no-op wherever it points
    torch.cuda.synchronize()
    assert bool((dst == 0xAB).all())


# ----------------------------------------------------------------------------- split_rows + the loss kernels' in-place gradients
@pytest.mark.parametrize("layout,c,h,w,library", [("cl", 4, 19, 23, True), ("nchw", 4, 19, 23, False), ("cl", 3, 5, 7, False)],
                         ids=["channels_last", "nchw", "rows_off_16_bytes"])
def test_split_rows_gradient_of_two_scaled_losses(layout, c, h, w, library, monkeypatch):
    """Logits batch [labeled | unlabeled | flipped]: softmax_kl on part 0, softmax_mse on part 2 against part 1 (detached by the op,
    flip replayed), each scaled by a 0-d device coefficient.  The batch gradient = float64 autograd of the same graph on torch.split:
    in channels-last (where _scaled_grad writes the parts' rows by miseg_assemble_rows), in NCHW (the kernels read a converted copy: torch
    product), and at C = 3, 5 x 7, whose rows start off a 16-byte boundary (torch product again)."""
    o = ops()
    sizes, masks, coeffs = (1, 2, 2), (3, 1), (0.7, 5.0)
    x = P.logits(f"split/{layout}/{c}", sum(sizes), c, h, w, 2)
    t = P.labels(f"split/t/{c}", sizes[0], h, w, c)
    ref_loss, ref_grad = P.split_losses_ref(x, sizes, t, masks, coeffs)
    xd = (dev_cl(x) if layout == "cl" else x.to(DEV).contiguous()).requires_grad_(True)
    names = []
    real = o.call
    monkeypatch.setattr(o, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    parts = o.split_rows(xd, sizes)
    c0, c1 = torch.tensor(coeffs[0], device=DEV), torch.tensor(coeffs[1], device=DEV)
    loss = c0 * o.softmax_kl(parts[0], t.to(DEV)) + c1 * o.softmax_mse(parts[2], parts[1], masks_dev(masks))
    loss.backward()
    if layout == "cl" and not library:
        assert parts[2].data_ptr() % 16 != 0 or parts[2].numel() % 4 != 0
    assert ("miseg_assemble_rows" in names) == library, names
    grad = xd.grad
    el, bl = P.loss_error(float(loss), float(ref_loss))
    eg, bg = P.grad_error(grad, ref_grad)
    print(f"\nPIXEL split    {layout}_c{c}_{h}x{w} loss err={el:.3e} (bound {bl:.3e}) grad err={eg:.3e} (bound {bg:.3e})")
    assert el <= bl and eg <= bg
    for i, coeff in ((0, coeffs[0]), (2, coeffs[1])):                   # each part against its own scale, not only the batch's largest entry
        lo = sum(sizes[:i])
        e, b = P.grad_error(grad[lo:lo + sizes[i]], ref_grad[lo:lo + sizes[i]])
        assert e <= b, (i, e, b)
    assert float(grad[sizes[0]:sizes[0] + sizes[1]].abs().max()) == 0.0  # the detached part: zeros
    assert grad.is_contiguous(memory_format=CL) == (layout == "cl") or c == 1


def test_zz_worst_errors():
    """Prints the worst error / bound per loss kernel seen by this run (for the table in this module's docstring)."""
    for k, (wl, tl, wg, tg) in sorted(WORST.items()):
        print(f"\nPIXEL-WORST {k:8s} loss err/bound={wl:.3f} at {tl}; grad err/bound={wg:.3f} at {tg}")
        assert wl <= 1.0 and wg <= 1.0
