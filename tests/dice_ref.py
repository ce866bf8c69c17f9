"""Float64 references of the Dice supervised loss, on the CPU.

``reference``: the wheel's expression (whl:deepclustering2/loss/dice_loss.py:79-135, reduction "mean") on ``softmax(logits)`` and the
one-hot of the labels, optionally plus ``KL_div`` (whl:deepclustering2/loss/kl_losses.py:107-126), with torch autograd.
``closed_form``: what the kernel evaluates -- per (sample, class) the sums ``I`` and ``D``, the two coefficients
``a = -2 w / (D + eps)`` and ``b = w (2 I + eps) pow / (D + eps)^2`` and the softmax Jacobian -- written out without autograd.
``bad``: a boolean pixel mask [N,H,W]; those pixels' ``p`` and ``t`` are zeroed (the kernel's rule for a label outside [0, C)).
The inputs of the tests come from ``logits`` / ``labels`` below and are never modified.
"""
import torch

SHAPES = ((3, 4, 33, 31), (2, 16, 5, 7), (2, 2, 64, 64))
KL_EPS = 1e-16


def logits(shape, scale, seed=None):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(1000 * c + int(scale) + 7 * h if seed is None else seed)
    return torch.randn(n, c, h, w, generator=g) * scale


def labels(shape, seed=None):
    """Sample 0 is labelled entirely with class 1 and class 0 is absent everywhere."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(31 * c + h if seed is None else seed)
    t = torch.randint(1, c, (n, h, w), generator=g) if c > 2 else torch.ones(n, h, w, dtype=torch.long)
    t[0] = 1
    return t


def class_weights(c):
    return [0.5 + 0.25 * i for i in range(c)]


def _operands(z64, lab, bad):
    c = z64.shape[1]
    p = z64.softmax(1)
    t = torch.stack([lab == k for k in range(c)], 1).double()
    if bad is not None:
        keep = (~bad).unsqueeze(1).double()
        p, t = p * keep, t * keep
    return p, t


def dice_of(p, t, pow=1, eps=1e-8, weight=None):
    """The wheel's GeneralizedDiceLoss.forward on given operands, reduction 'mean', any floating dtype."""
    dims = list(range(2, p.dim()))
    inter = (p * t).sum(dims)
    den = (p.pow(pow) + t.pow(pow)).sum(dims)
    dices = 1 - (2 * inter + eps) / (den + eps)
    if weight is not None:
        dices = torch.as_tensor(weight, dtype=dices.dtype) * dices
    return dices.mean()


def kl_of(p, t, npix=None):
    kl = (-t * torch.log((p + KL_EPS) / (t + KL_EPS))).sum(1)
    return kl.mean() if npix is None else kl.sum() / npix


def reference(z, lab, pow=1, eps=1e-8, weight=None, kl_weight=0.0, dice_weight=1.0, bad=None):
    """(loss, d loss / d logits) in float64 by autograd."""
    z64 = z.double().clone().requires_grad_()
    p, t = _operands(z64, lab, bad)
    loss = dice_weight * dice_of(p, t, pow, eps, weight)
    if kl_weight != 0.0:
        loss = loss + kl_weight * kl_of(p, t)
    loss.backward()
    return float(loss.detach()), z64.grad


def closed_form(z, lab, pow=1, eps=1e-8, weight=None, kl_weight=0.0, dice_weight=1.0, bad=None):
    """The same two results from the kernel's formulas, float64, no autograd."""
    with torch.no_grad():
        z64 = z.double()
        n, c, h, w = z64.shape
        p_full = z64.softmax(1)
        p, t = _operands(z64, lab, bad)
        wv = torch.ones(c, dtype=torch.float64) if weight is None else torch.as_tensor(weight, dtype=torch.float64)
        inter = (p * t).sum((2, 3))
        den = p.pow(pow).sum((2, 3)) + t.sum((2, 3))
        loss = dice_weight * float((wv * (1 - (2 * inter + eps) / (den + eps))).mean())
        a = (-2 * wv / (den + eps)) * dice_weight / (n * c)
        b = (wv * (2 * inter + eps) * pow / (den + eps) ** 2) * dice_weight / (n * c)
        g = a[:, :, None, None] * t + b[:, :, None, None] * (p_full if pow == 2 else torch.ones_like(p_full))
        if kl_weight != 0.0:
            loss += kl_weight * float(kl_of(p, t))
            g = g + t * (-1.0 / (p_full + KL_EPS)) * kl_weight / (n * h * w)
        grad = p_full * (g - (g * p_full).sum(1, keepdim=True))
        if bad is not None:
            grad = grad * (~bad).unsqueeze(1).double()
    return loss, grad


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())
