"""Float64 restatement of the cross pseudo supervision kernel (csrc/cps.hip, ``miseg_softmax_cross_pseudo``):
both losses, both gradients written out by hand, and the agreement count.  Shared by test_cpu_cps.py, which checks the restatement
against float64 autograd of ``F.cross_entropy`` on fixed labels, and test_gpu_cps.py, which runs the kernel against it.

Conventions: logits are [N, C, H, W].  The hard labels are taken on the fp32 INPUTS by numpy's argmax rule (the first maximum; +0.0
and -0.0 compare equal), so they are exactly the labels the kernel must find; everything after them is float64.  Plain cross entropy,
no epsilon; means over the N H W pixels.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def labels(z: torch.Tensor) -> torch.Tensor:
    """argmax over the channel axis of the fp32 logits, first maximum: int64 [N, H, W]."""
    assert z.dtype == torch.float32
    return torch.from_numpy(np.argmax(z.detach().cpu().numpy(), axis=1).astype(np.int64))


def top_two_gap(z: torch.Tensor) -> torch.Tensor:
    """Largest minus second largest logit of every pixel, in the inputs' own fp32 (exact: zero only for a tie)."""
    top = z.detach().float().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def one_sided(z: torch.Tensor, y: torch.Tensor):
    """(mean_pix (logsumexp(z) - z[y]), its gradient (softmax(z) - e_y) / npix) in float64 for fixed labels ``y``."""
    z64 = z.detach().to(F64)
    n, c, h, w = z64.shape
    onehot = torch.stack([y == k for k in range(c)], 1).to(F64)
    loss = (torch.logsumexp(z64, 1) - (z64 * onehot).sum(1)).mean()
    return loss, (z64.softmax(1) - onehot) / (n * h * w)


def loss_grads_agree(a: torch.Tensor, b: torch.Tensor):
    """((cps_a, cps_b), (ga, gb), agree): cps_a = CE(a, argmax b), cps_b = CE(b, argmax a), agree = #{ya == yb}."""
    ya, yb = labels(a), labels(b)
    la, ga = one_sided(a, yb)
    lb, gb = one_sided(b, ya)
    return (la, lb), (ga, gb), int((ya == yb).sum())


def autograd_one_sided(z: torch.Tensor, y: torch.Tensor):
    """The same pair by float64 autograd of ``F.cross_entropy`` on the fixed labels: the check of ``one_sided``."""
    z64 = z.detach().to(F64).clone().requires_grad_(True)
    loss = F.cross_entropy(z64, y)
    loss.backward()
    return loss.detach(), z64.grad


def implied_labels(grad: torch.Tensor, upstream: float = 1.0) -> torch.Tensor:
    """The label a gradient ``upstream * (softmax(z) - e_y) / npix`` was computed with: its one entry of the other sign (every softmax
    entry lies strictly inside (0, 1) for the bounded logits of the tests)."""
    g = grad.detach().cpu().to(F64) * (1.0 if upstream > 0 else -1.0)
    assert bool(((g < 0).sum(1) == 1).all()), "each pixel has exactly one entry below zero"
    return g.argmin(1)
