"""Pixel-wise losses on the logits (csrc/losses.hip, dice.hip, ict.hip, uamt.hip, cps.hip): each is one fused kernel that also leaves the gradient of the
logits, which the backward only has to scale."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import checks
from .._cabi import query
from .._rt import _need_gpu, _ptr, _stream, _ws, empty_nhwc, logits_nhwc
from .. import stepio
from ..stepio import scalar_out, zero_counter
from ._pkg import call
from .batch import _scaled_grad, _split_part_of       # the shared piece: a loss on a part of a split_rows writes that part's rows


class _ScaledGradLoss(torch.autograd.Function):
    """A loss whose forward saved d loss / d logits (``ctx.part``: the logits' place in a split_rows, if any): the backward scales it
    by the upstream gradient; no other input has a gradient."""

    @staticmethod
    def backward(ctx, g: Tensor):
        (grad,) = ctx.saved_tensors
        return (_scaled_grad(ctx.part, grad, g),) + (None,) * (len(ctx.needs_input_grad) - 1)


def _outputs(ctx, raw: Tensor, logits: Tensor, want_grad: bool = True):
    """What every pixel loss writes, for ``logits = logits_nhwc(raw)``: the loss scalar and the buffer for d loss / d logits, saved for
    the backward (None without ``want_grad``) beside the logits' place in a split_rows (``ctx.part``)."""
    ctx.part = _split_part_of(raw, logits)
    loss = scalar_out((), logits.device)
    grad = empty_nhwc(*logits.shape, torch.float32, logits.device) if want_grad else None
    if want_grad:
        ctx.save_for_backward(grad)
    return loss, grad


def _int64_labels(labels: Tensor, n: int, h: int, w: int) -> Tensor:
    labels = labels.contiguous().view(n, h, w)
    return labels if labels.dtype == torch.int64 else labels.long()


def _report_bad_labels(name: str, bad: Tensor, classes: int) -> None:
    """Hand the kernel's bad-label flag to ``checks.require_zero`` (raised now, or at the iteration's fetch inside a deferred block)."""
    checks.require_zero(bad, AssertionError, f"{name}: a label lies outside [0, {classes}) "
                                             f"(class2one_hot of the {classes}-class configuration would refuse it)")


class _SoftmaxKL(_ScaledGradLoss):
    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor, flag_box: list):
        _need_gpu(logits, labels)
        raw, logits = logits, logits_nhwc(logits)
        n, c, h, w = logits.shape
        labels = _int64_labels(labels, n, h, w)
        loss, glogits = _outputs(ctx, raw, logits)
        bad = zero_counter(logits.device, (1,))
        ws = _ws(query("miseg_loss_ws_bytes", n, h, w), logits.device)
        call("miseg_softmax_kl", _stream(), _ptr(logits), _ptr(labels), n, h, w, c, None, _ptr(loss), _ptr(glogits), _ptr(bad),
             _ptr(ws), ws.numel())
        flag_box.append(bad)      # the bad-label flag, handed to softmax_kl beside the graph (a second output would cost the backward a zeros launch)
        return loss


def softmax_kl(logits: Tensor, labels: Tensor, check_labels: bool = True) -> Tensor:
    """KL_div(softmax(logits), class2one_hot(labels)) with reduction='mean'.  A label outside [0, C) -- an ignore index, a mask with
    more classes than the configuration -- makes the reference's ``class2one_hot`` raise AssertionError; the kernel flags it (such a
    pixel adds nothing to the loss and gets a zero gradient) and, with ``check_labels``, the flag goes to ``checks.require_zero``:
    raised here outside a ``checks.deferred`` block (one host read, as the evaluation epochers do: they read the loss right after
    anyway), and at the iteration's fetch inside one (the train step: the flag is one of the iteration's int32 counters and travels with
    its report -- no launch, no synchronisation)."""
    flag_box: list = []
    loss = _SoftmaxKL.apply(logits, labels, flag_box)
    if check_labels:
        _report_bad_labels("softmax_kl", flag_box[0], int(logits.shape[1]))
    return loss


class _SoftmaxMSE(_ScaledGradLoss):
    entry = "miseg_softmax_mse"

    @classmethod
    def forward(cls, ctx, a: Tensor, b: Tensor, flips: Optional[Tensor]):
        _need_gpu(a, b, flips)
        raw, a, b = a, logits_nhwc(a), logits_nhwc(b.detach())
        n, c, h, w = a.shape
        loss, ga = _outputs(ctx, raw, a)
        ws = _ws(query("miseg_loss_ws_bytes", n, h, w), a.device)
        call(cls.entry, _stream(), _ptr(a), _ptr(b), _ptr(flips), n, h, w, c, None, _ptr(loss), _ptr(ga), _ptr(ws), ws.numel())
        return loss


def softmax_mse(a: Tensor, b: Tensor, flips: Optional[Tensor] = None) -> Tensor:
    """mean((softmax(a) - softmax(flip(b)).detach())**2); ``flips`` replays the per-sample flip on b."""
    return _SoftmaxMSE.apply(a, b, flips)


class _SoftmaxKLCons(_SoftmaxMSE):
    entry = "miseg_softmax_klcons"


def softmax_kl_consistency(a: Tensor, b: Tensor, flips: Optional[Tensor] = None) -> Tensor:
    """KL_div()(softmax(a), softmax(flip(b)).detach()) -- the `UDARegCriterion.name: kl` consistency term, fused like softmax_mse."""
    return _SoftmaxKLCons.apply(a, b, flips)


class _SoftmaxMixMSE(_ScaledGradLoss):
    entry = "miseg_softmax_mix_mse"

    @classmethod
    def forward(cls, ctx, a: Tensor, b: Tensor, perm: Tensor, coef: Tensor, flag_box: list):
        _need_gpu(a, b, perm, coef)
        raw, a, b = a, logits_nhwc(a), logits_nhwc(b.detach())
        n, c, h, w = a.shape
        assert b.shape == a.shape and perm.dtype == torch.int32 and perm.numel() >= n and perm.is_contiguous(), (a.shape, b.shape, perm.dtype, perm.shape)
        assert coef.dtype == torch.float32 and coef.numel() >= 2 and coef.is_contiguous(), (coef.dtype, coef.shape)
        loss, ga = _outputs(ctx, raw, a)
        bad = zero_counter(a.device, (1,))
        ws = _ws(query("miseg_loss_ws_bytes", n, h, w), a.device)
        call(cls.entry, _stream(), _ptr(a), _ptr(b), _ptr(perm), _ptr(coef), n, h, w, c, None, _ptr(loss), _ptr(ga), _ptr(bad), _ptr(ws), ws.numel())
        flag_box.append(bad)      # the bad-index flag, handed over beside the graph as in _SoftmaxKL
        return loss


class _SoftmaxMixKLCons(_SoftmaxMixMSE):
    entry = "miseg_softmax_mix_klcons"


def _mix_loss(fn, name: str, a: Tensor, b: Tensor, perm: Tensor, coef: Tensor, check_perm: bool) -> Tensor:
    flag_box: list = []
    loss = fn.apply(a, b, perm, coef, flag_box)
    if check_perm:
        checks.require_zero(flag_box[0], IndexError, f"{name}: an entry of the permutation lies outside [0, {int(a.shape[0])})")
    return loss


def softmax_mix_mse(a: Tensor, b: Tensor, perm: Tensor, coef: Tensor, check_perm: bool = True) -> Tensor:
    """mean((softmax(a) - q)**2) with q = coef[0] * softmax(b) + coef[1] * softmax(b[perm]), detached: the ICT consistency term
    (DESIGN.md section 27), fused like ``softmax_mse``.  ``perm`` int32 [N] and ``coef`` fp32 [2] on the device.  A ``perm[i]`` outside
    [0, N) counts as i and is flagged; with ``check_perm`` the flag goes to ``checks.require_zero`` as in ``softmax_kl``."""
    return _mix_loss(_SoftmaxMixMSE, "softmax_mix_mse", a, b, perm, coef, check_perm)


def softmax_mix_kl_consistency(a: Tensor, b: Tensor, perm: Tensor, coef: Tensor, check_perm: bool = True) -> Tensor:
    """KL_div()(softmax(a), q) with the mixed target of ``softmax_mix_mse``: the ``ICTParameters.name: kl`` form."""
    return _mix_loss(_SoftmaxMixKLCons, "softmax_mix_kl_consistency", a, b, perm, coef, check_perm)


def softmax_accum(logits: Tensor, acc: Optional[Tensor] = None) -> Tensor:
    """``softmax(logits, 1)`` into a new accumulator (``acc`` None) or added to ``acc`` in place: the sum of the UA-MT teacher's
    predictions over its stochastic passes.  The accumulator is fp32 NHWC (a channels_last [N,C,H,W] tensor);
    the order of the additions is the order of the calls.  No autograd."""
    _need_gpu(logits, acc)
    logits = logits_nhwc(logits.detach())
    n, c, h, w = logits.shape
    first = acc is None
    if first:
        acc = empty_nhwc(n, c, h, w, torch.float32, logits.device)
    assert acc.shape == logits.shape and acc.dtype == torch.float32 and acc.is_contiguous(memory_format=torch.channels_last), \
        (acc.shape, acc.dtype, acc.stride())
    call("miseg_softmax_accum", _stream(), _ptr(logits), n, h, w, c, int(first), _ptr(acc))
    return acc


def _kept_out(device) -> Tensor:
    """int64[1] for the count of certain pixels: inside an iteration two adjacent counters of the step block (8-byte aligned; the
    kernel writes both words), otherwise an ordinary allocation."""
    io = stepio.CURRENT
    if io is None or io.device != device:
        return torch.empty(1, dtype=torch.int64, device=device)
    lo = io.counter()
    if lo.data_ptr() % 8:
        lo = io.counter()
    io.counter()
    i = io.counter_index(lo)
    return io.counters_base()[i:i + 2].view(torch.int64)


class _SoftmaxUMSE(_ScaledGradLoss):
    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, acc: Tensor, thr: Tensor, passes: int, box: list):
        _need_gpu(a, b, acc, thr)
        raw, a, b, acc = a, logits_nhwc(a), logits_nhwc(b.detach()), logits_nhwc(acc.detach())
        n, c, h, w = a.shape
        assert b.shape == a.shape and acc.shape == a.shape, (a.shape, b.shape, acc.shape)
        assert thr.dtype == torch.float32 and thr.numel() >= 1 and thr.is_contiguous(), (thr.dtype, thr.shape)
        loss, ga = _outputs(ctx, raw, a)
        kept, stats = _kept_out(a.device), scalar_out((2,), a.device)
        ws = _ws(query("miseg_softmax_umse_ws_bytes", n, h, w), a.device)
        call("miseg_softmax_umse", _stream(), _ptr(a), _ptr(b), _ptr(acc), n, h, w, c, 1.0 / int(passes), _ptr(thr), None, _ptr(loss),
             _ptr(ga), _ptr(kept), _ptr(stats), _ptr(ws), ws.numel())
        box.extend((kept, stats))      # handed over beside the graph, as the flag of _SoftmaxKL
        return loss


def softmax_umse(a: Tensor, b: Tensor, acc: Tensor, thr: Tensor, passes: int):
    """The UA-MT consistency term, fused like ``softmax_mse``: with ``m = acc / passes``,
    ``unc = -sum_c m_c log(m_c + 1e-6)`` and ``mask = unc < thr`` per pixel, ``sum(mask * (softmax(a) - softmax(b).detach())**2) /
    (C * K + 1e-16)`` for ``K = sum(mask)``; 0 with a zero gradient where no pixel is certain.  ``acc``: the sum ``softmax_accum``
    left; ``thr``: fp32 [1] on the device (the iteration's step block).  Returns ``(loss, kept, stats)``: ``kept`` int64 [1] = K,
    ``stats`` fp32 [2] = (K / (N H W), mean unc).  The gradient flows to ``a`` only."""
    box: list = []
    loss = _SoftmaxUMSE.apply(a, b, acc, thr, int(passes), box)
    return loss, box[0], box[1]


def _cps_operand(x, name: str):
    """One operand of ``softmax_cross_pseudo``: ``(tensors, rows, nhwc)`` -- the tensors autograd sees, their row counts and the fp32
    NHWC batch the kernel reads (``nhwc[i]``: the i-th tensor's rows of it).  A tensor is read in place when it is fp32 NHWC already
    and converted in layout otherwise; a sequence must be the parts of one ``split_rows`` in order, adjacent in memory."""
    parts = tuple(x) if isinstance(x, (tuple, list)) else (x,)
    for t in parts:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
            raise TypeError(f"softmax_cross_pseudo: {name} must be fp32 [N,C,H,W] logits on the GPU (there is no torch fallback), got "
                            f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', 'the host')}")
    if len(parts) == 1:
        nhwc = logits_nhwc(parts[0])
        return parts, [int(parts[0].shape[0])], [nhwc]
    nhwc = [logits_nhwc(t) for t in parts]
    for prev, t, given in zip(nhwc, nhwc[1:], parts[1:]):
        if t.data_ptr() != given.data_ptr() or t.shape[1:] != prev.shape[1:] or t.data_ptr() != prev.data_ptr() + 4 * prev.numel():
            raise TypeError(f"softmax_cross_pseudo: the parts of {name} must be adjacent fp32 NHWC rows of one batch (ops.split_rows)")
    return parts, [int(t.shape[0]) for t in parts], nhwc


class _SoftmaxCrossPseudo(torch.autograd.Function):
    """Two differentiable operands, each one tensor or the parts of a split_rows: ``ctx.groups[k]`` holds, per tensor of operand k, its
    place in a split_rows (if any), its first row and its row count in the saved gradient."""

    @staticmethod
    def forward(ctx, box: list, agree_out: Optional[Tensor], na: int, *tensors: Tensor):
        given = (tensors[:na], tensors[na:])
        read, ctx.groups, wants = [], [], []
        for k, (name, group) in enumerate(zip("ab", given)):
            parts, rows, nhwc = _cps_operand(group if len(group) > 1 else group[0], name)
            read.append((nhwc[0], sum(rows)))
            ctx.groups.append([(_split_part_of(t, u), sum(rows[:i]), rows[i]) for i, (t, u) in enumerate(zip(parts, nhwc))])
            first = 3 + (0 if k == 0 else na)
            wants.append(any(ctx.needs_input_grad[first:first + len(parts)]))
        (a, n), (b, nb) = read
        _, c, h, w = a.shape
        if nb != n or b.shape[1:] != a.shape[1:]:
            raise ValueError(f"softmax_cross_pseudo: a has {n} x {tuple(a.shape[1:])} logits and b {nb} x {tuple(b.shape[1:])}")
        dev = a.device
        loss = scalar_out((2,), dev)
        grads = [empty_nhwc(n, c, h, w, torch.float32, dev) if want else None for want in wants]
        agree = _kept_out(dev) if agree_out is None else agree_out
        assert agree.dtype == torch.int64 and agree.numel() == 1 and agree.data_ptr() % 8 == 0, (agree.dtype, agree.shape)
        ws = _ws(query("miseg_softmax_cross_pseudo_ws_bytes", n, h, w), dev)
        call("miseg_softmax_cross_pseudo", _stream(), _ptr(a), _ptr(b), n, h, w, c, None, _ptr(loss), _ptr(grads[0]), _ptr(grads[1]), _ptr(agree),
             _ptr(ws), ws.numel())
        ctx.wants = wants
        ctx.save_for_backward(*[g for g in grads if g is not None])
        box.append(agree)         # handed over beside the graph, as the flag of _SoftmaxKL
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        saved = list(ctx.saved_tensors)
        out = []
        for k, group in enumerate(ctx.groups):
            grad = saved.pop(0) if ctx.wants[k] else None
            for part, first, rows in group:
                out.append(None if grad is None else _scaled_grad(part, grad if len(group) == 1 else grad.narrow(0, first, rows), g[k]))
        return (None, None, None) + tuple(out)


def softmax_cross_pseudo(a, b, agree_out: Optional[Tensor] = None):
    """The cross pseudo supervision term of two networks' logits, one fused kernel with both gradients: with
    ``ya = argmax(a, 1)`` and ``yb = argmax(b, 1)`` (first maximum, labels detached), ``loss = [cross_entropy(a, yb),
    cross_entropy(b, ya)]`` as means over the pixels, and ``agree`` = int64 [1], the number of pixels with ``ya == yb``.  Returns
    ``(loss, agree)``; ``LinearLoss.of(loss)`` is the sum of the two.  The backward scales the saved gradient of ``a`` by the upstream
    gradient of ``loss[0]`` and that of ``b`` by ``loss[1]``'s.  An operand is one [N,C,H,W] tensor -- it may be a part of a
    ``split_rows`` -- or the sequence of all adjacent parts of one, read as the batch they make: each part's gradient then goes to its
    own rows.  Under ``torch.no_grad()`` or for an operand that needs none, that gradient is not computed.  fp32 logits on the device
    only: anything else raises ``TypeError``.  ``agree_out``: where to write the count (int64 [1], 8-byte aligned) instead of the
    iteration's counter pair."""
    ta = tuple(a) if isinstance(a, (tuple, list)) else (a,)
    tb = tuple(b) if isinstance(b, (tuple, list)) else (b,)
    box: list = []
    loss = _SoftmaxCrossPseudo.apply(box, agree_out, len(ta), *ta, *tb)
    return loss, box[0]


_LOSS_CLASS_COUNTS = (2, 3, 4, 5, 6, 8, 10, 16)     # MISEG_DISPATCH_C of csrc/pixel_loss.h


def softmax_entropy_supported(c: int) -> bool:
    """Whether ``softmax_entropy`` has a kernel for ``c`` classes (the pixel losses' dispatch list: 2-6, 8, 10, 16)."""
    return int(c) in _LOSS_CLASS_COUNTS


class _SoftmaxEntropy(_ScaledGradLoss):
    @staticmethod
    def forward(ctx, logits: Tensor):
        _need_gpu(logits)
        raw, logits = logits, logits_nhwc(logits)
        n, c, h, w = logits.shape
        loss, glogits = _outputs(ctx, raw, logits)
        ws = _ws(query("miseg_loss_ws_bytes", n, h, w), logits.device)
        call("miseg_softmax_entropy", _stream(), _ptr(logits), n, h, w, c, None, _ptr(loss), _ptr(glogits), _ptr(ws), ws.numel())
        return loss


def softmax_entropy(logits: Tensor) -> Tensor:
    """Entropy(reduction='mean', eps=1e-16)(softmax(logits, 1)) = mean_{n,h,w} -sum_c p_c log(p_c + 1e-16), one fused kernel with its
    backward; a per-sample flip of the logits does not change it.  Class counts: ``softmax_entropy_supported``."""
    return _SoftmaxEntropy.apply(logits)


def softmax_dice_supported(c: int) -> bool:
    """Whether ``softmax_dice`` has a kernel for ``c`` classes (the pixel losses' dispatch list: 2-6, 8, 10, 16)."""
    return int(c) in _LOSS_CLASS_COUNTS


class _SoftmaxDice(_ScaledGradLoss):
    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor, flag_box: list, consts: tuple, class_weight: Optional[Tensor], want_grad: bool):
        _need_gpu(logits, labels, class_weight)
        raw, logits = logits, logits_nhwc(logits)
        n, c, h, w = logits.shape
        labels = _int64_labels(labels, n, h, w)
        power, eps, kl_weight, dice_weight = consts
        loss, glogits = _outputs(ctx, raw, logits, want_grad)      # evaluation: forward only, no gradient pass
        bad = zero_counter(logits.device, (1,))
        ws = _ws(query("miseg_softmax_dice_ws_bytes", n, h, w, c), logits.device)
        call("miseg_softmax_dice", _stream(), _ptr(logits), _ptr(labels), n, h, w, c, power, eps, _ptr(class_weight), kl_weight,
             dice_weight, None, _ptr(loss), _ptr(glogits), _ptr(bad), _ptr(ws), ws.numel())
        flag_box.append(bad)      # the bad-label flag, handed over beside the graph as in _SoftmaxKL
        return loss


def softmax_dice(logits: Tensor, labels: Tensor, *, pow: int = 1, eps: float = 1e-8, class_weight: Optional[Tensor] = None,
                 kl_weight: float = 0.0, dice_weight: float = 1.0, check_labels: bool = True) -> Tensor:
    """``kl_weight * KL_div()(p, t) + dice_weight * GeneralizedDiceLoss(eps, class_weight, pow)(p, t)`` for ``p = softmax(logits, 1)``
    and ``t = class2one_hot(labels)``, reduction 'mean', in the fused entry point ``miseg_softmax_dice`` with its backward (with
    ``kl_weight == 0`` the KL part is not computed).  ``class_weight``: a float32 vector of C entries on the logits' device (the
    criterion objects upload theirs once), or None.  Under ``torch.no_grad()`` the gradient pass is not launched.  A label outside
    [0, C) is flagged, adds nothing and gets a zero gradient; with ``check_labels`` the flag goes to ``checks.require_zero`` exactly
    as in ``softmax_kl``.  Class counts: ``softmax_dice_supported``."""
    if class_weight is not None:
        assert class_weight.dtype == torch.float32 and class_weight.is_contiguous() and class_weight.numel() == int(logits.shape[1]), \
            (class_weight.dtype, tuple(class_weight.shape), int(logits.shape[1]))
    flag_box: list = []
    want_grad = torch.is_grad_enabled() and logits.requires_grad
    loss = _SoftmaxDice.apply(logits, labels, flag_box, (int(pow), float(eps), float(kl_weight), float(dice_weight)), class_weight, want_grad)
    if check_labels:
        _report_bad_labels("softmax_dice", flag_box[0], int(logits.shape[1]))
    return loss
