"""MetaDice / GeneralizedDiceLoss (ref whl:deepclustering2/loss/dice_loss.py:8-76, 79-135).

``GeneralizedDiceLoss()(prob, onehot)`` keeps the reference call form and expression.  On the train-step hot path the epocher calls
``GeneralizedDiceLoss.from_logits(logits, labels)`` instead, which is the fused HIP entry point ``miseg_softmax_dice`` (softmax +
one-hot + the per-sample per-class sums + mean, and the backward) -- the same expression evaluated from the logits.

One deliberate difference from the wheel: ``forward`` accepts ``disable_assert=True`` (the reference's ``EvalEpocher`` passes it to the
supervised criterion, ``semi_seg/epocher.py:62``; the wheel's class would raise ``TypeError`` there).  ``MetaDice`` / ``dice_coef`` /
``dice_batch`` are metrics, restated in plain torch.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from deepclustering2.utils import one_hot, simplex


def _per_class(x: Tensor) -> Tensor:
    """[B, C, *] -> [B, C, npix] (a [B, C] input counts as one pixel)."""
    return x.reshape(x.shape[0], x.shape[1], -1)


class MetaDice(nn.Module):
    """Dice coefficient ``(2 sum p t + eps) / (sum (p + t) + eps)`` of a simplex prediction against a one-hot target, per sample and
    class (``"2d"``) or per class over the whole batch (``"3d"``); a metric, not a loss.  ``weight`` scales the intersection."""

    def __init__(self, method: str, weight: Tensor = None, reduce: bool = False, eps: float = 1e-8) -> None:
        super().__init__()
        assert method in ("2d", "3d"), method
        self.method, self.reduce, self.eps, self.weight = method, reduce, eps, weight

    def forward(self, pred: Tensor, target: Tensor):
        assert pred.shape == target.shape, f"`pred` {tuple(pred.shape)} and `target` {tuple(target.shape)} differ in shape"
        assert not target.requires_grad
        assert simplex(pred), "pred should be simplex"
        assert one_hot(target), "target should be onehot"
        p, t = _per_class(pred.float()), _per_class(target.float())
        over = (2,) if self.method == "2d" else (0, 2)
        inter, union = (p * t).sum(over), (p + t).sum(over)
        if self.weight is not None:
            inter = self.weight * inter
        dices = (2.0 * inter + self.eps) / (union + self.eps)
        return dices.mean(0) if self.reduce and self.method == "2d" else dices


dice_coef = MetaDice(method="2d", reduce=False)
dice_batch = MetaDice(method="3d", reduce=False)


class GeneralizedDiceLoss(nn.Module):
    """``I[b,c] = sum_px p t``, ``D[b,c] = sum_px (p^pow + t^pow)``, ``dice = 1 - (2 I + eps) / (D + eps)`` (times ``weight[c]``),
    reduced over ``[B, C]`` (https://arxiv.org/pdf/1707.03237.pdf as the wheel states it).  ``ignore_index``: as in the wheel, the
    entries of the ONE-HOT that equal it are masked out of both operands."""

    def __init__(self, epsilon=1e-8, weight=None, pow=1, ignore_index=None, reduction="mean"):
        super().__init__()
        assert reduction in ("mean", "sum", "none"), reduction
        self.epsilon, self.weight, self.ignore_index, self.pow, self.reduction = epsilon, weight, ignore_index, pow, reduction
        self._device_weight = {}     # device -> fp32[C] copy of ``weight`` for the fused call: uploaded once per criterion object

    def forward(self, input: Tensor, target: Tensor, **kwargs) -> Tensor:
        assert input.shape == target.shape, "'input' and 'target' must have the same shape"
        if not kwargs.get("disable_assert"):
            assert simplex(input) and one_hot(target)
        p = _per_class(input)
        t = _per_class(target).to(p.dtype if p.dtype == torch.float64 else torch.float32)
        if self.ignore_index is not None:
            keep = (t != self.ignore_index).to(t.dtype)
            p, t = p * keep, t * keep
        inter = (p * t).sum(2)
        denom = (p ** self.pow + t ** self.pow).sum(2)
        dices = 1 - (2 * inter + self.epsilon) / (denom + self.epsilon)
        if self.weight is not None:
            dices = torch.as_tensor(self.weight, dtype=dices.dtype, device=dices.device) * dices
        return dices.mean() if self.reduction == "mean" else dices.sum() if self.reduction == "sum" else dices

    # ---- the fused path
    def supports_fused(self, num_classes: int = None) -> bool:
        if self.reduction != "mean" or self.pow not in (1, 2) or isinstance(self.pow, bool) or self.ignore_index is not None:
            return False
        if self.weight is None:
            return True
        w = torch.as_tensor(self.weight)
        return w.dim() == 1 and (num_classes is None or w.numel() == int(num_classes))

    def class_weight_on(self, device):
        """``weight`` as a device fp32 vector (None without weights); cached per device."""
        if self.weight is None:
            return None
        key = str(torch.device(device))
        w = self._device_weight.get(key)
        if w is None:
            w = self._device_weight[key] = torch.as_tensor(self.weight).detach().to(device=device, dtype=torch.float32).contiguous()
        return w

    def from_logits(self, logits: Tensor, labels: Tensor) -> Tensor:
        """== self(softmax(logits, 1), class2one_hot(labels)) in the fused HIP entry point (+ fused backward)."""
        from miseg_amd import ops
        assert self.supports_fused(logits.shape[1])
        return ops.softmax_dice(logits, labels, pow=int(self.pow), eps=float(self.epsilon), class_weight=self.class_weight_on(logits.device),
                                kl_weight=0.0, dice_weight=1.0)

    def signature(self) -> tuple:
        """The constants a recorded fused call has baked in."""
        w = None if self.weight is None else tuple(float(v) for v in torch.as_tensor(self.weight).flatten().tolist())
        return (float(self.epsilon), self.pow, w, self.ignore_index, self.reduction)
