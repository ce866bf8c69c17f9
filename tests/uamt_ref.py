"""Float64 restatement of the uncertainty-aware Mean Teacher's device work (csrc/uamt.hip): the threshold
ramp, the clipped noise, the accumulation of softmaxes over the passes, the predictive entropy, and the masked consistency term with
its gradient with respect to the student's logits -- by autograd AND written out by hand.  Shared by test_cpu_uamt.py, which checks
the restatement, and test_gpu_mt_uncertainty.py, which runs the kernels against it.

Conventions: logits are [N, C, H, W]; ``acc`` is the SUM of the passes' softmaxes, ``m = acc / passes`` their mean;
``unc = -sum_c m_c log(m_c + 1e-6)``; a pixel is certain where ``unc < thr``, strictly; ``K`` counts them.

Thresholds of kernel tests come from ``gap_threshold``: the midpoint of the widest gap between consecutive sorted uncertainties that
leaves a share of the pixels on each side, so that no pixel lies within fp32 error of the threshold and the kernel's mask must equal
the reference's at every pixel.  The gap of N values spread over [0, ln C] shrinks like 1 / N: 1 311 pixels (3 x 19 x 23) leave a few
1e-3, half a million would leave a few 1e-6 -- within fp32 error of somebody.  ``pass_logits`` therefore draws the passes of a case
with more than 4 096 pixels on a 16 x coarser grid and repeats every value over its 16 x 16 cell: the kernel still walks every pixel
of the large shape (its grid-stride loop), the uncertainty map has some two thousand distinct values.  The student's and the target's
logits are pixel_ref's at full resolution everywhere.
"""
from __future__ import annotations

import functools
import math

import torch

import pixel_ref as P

F64 = torch.float64
UNC_EPS = 1e-6
DEN_EPS = 1e-16
PASSES = 3                       # T of the kernel tests
PASS_SCALE = 2.0                 # logit scale of the passes: probabilities spread over the simplex, entropies over [0, ln C]
COARSE_ABOVE, CELL = 4096, 16
MIN_HALF_GAP = 1e-4


def threshold(k: int, k_total: int, start: float, end: float, num_classes: int) -> float:
    """``(start + (end - start) * exp(-5 (1 - min(k / k_total, 1))^2)) * ln(C)`` in double."""
    r = min(k / k_total, 1.0)
    return (start + (end - start) * math.exp(-5.0 * (1.0 - r) ** 2)) * math.log(num_classes)


def noise(x: torch.Tensor, z: torch.Tensor, sigma: float, clip: float) -> torch.Tensor:
    """``x + clamp(sigma * z, -clip, clip)`` in the dtype of its operands (float64 for the reference, float32 for the bit-exact twin of
    the kernel: one multiply, a clamp, one add)."""
    return x + (z * sigma).clamp(-clip, clip)


def accumulate(logit_list) -> torch.Tensor:
    """Sum of the softmaxes over the class axis, float64, in the order of the list."""
    acc = None
    for z in logit_list:
        p = z.detach().to(F64).softmax(1)
        acc = p if acc is None else acc + p
    return acc


def uncertainty(acc: torch.Tensor, passes: int) -> torch.Tensor:
    """[N, H, W] float64: the entropy of the mean prediction, ``-sum_c m_c log(m_c + 1e-6)``."""
    m = acc.to(F64) / passes
    return -(m * torch.log(m + UNC_EPS)).sum(1)


def umse_expr(a64: torch.Tensor, b64: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """``sum_pix mask * sum_c (softmax(a) - softmax(b))_c^2 / (C K + 1e-16)``, b detached."""
    d = a64.softmax(1) - b64.detach().softmax(1)
    k = mask.sum().to(F64)
    return (mask.to(F64).unsqueeze(1) * d * d).sum() / (a64.shape[1] * k + DEN_EPS)


def umse_value_and_grad(a: torch.Tensor, b: torch.Tensor, acc: torch.Tensor, passes: int, thr: float):
    """``(loss, grad by autograd, grad by hand, K, mask, unc)`` in float64.  By hand: ``mask * 2 p_c (d_c - sum_k d_k p_k) /
    (C K + 1e-16)`` through the softmax Jacobian.  ``thr`` is compared as given (the caller passes the float32 value the device
    holds)."""
    unc = uncertainty(acc, passes)
    mask = unc < float(thr)
    a64 = a.detach().to(F64).clone().requires_grad_(True)
    b64 = b.detach().to(F64)
    loss = umse_expr(a64, b64, mask)
    loss.backward()
    p = a64.detach().softmax(1)
    d = p - b64.softmax(1)
    k = int(mask.sum())
    hand = mask.to(F64).unsqueeze(1) * 2.0 * p * (d - (d * p).sum(1, keepdim=True)) / (a.shape[1] * k + DEN_EPS)
    return loss.detach(), a64.grad, hand, k, mask, unc


def gap_threshold(unc64: torch.Tensor, lo_share: float = 0.1):
    """``(thr, half_gap)``: the midpoint of the widest gap between consecutive sorted uncertainties that leaves at least ``lo_share``
    of the pixels on each side, and half that gap's width."""
    u = torch.sort(unc64.detach().to(F64).flatten()).values
    n = u.numel()
    lo = max(int(math.ceil(lo_share * n)), 1)          # at least `lo` values at or below the gap, and as many above it
    assert n >= 2 * lo, n
    gaps = u[lo:n - lo + 1] - u[lo - 1:n - lo]
    i = int(torch.argmax(gaps))
    return float((u[lo - 1 + i] + u[lo + i]) / 2.0), float(gaps[i] / 2.0)


def f32(v: float) -> float:
    """The value a float32 device word holds, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


# ----------------------------------------------------------------------------- the kernel tests' cases: every pixel_ref.LOSS_CASES entry
def pass_logits(name: str, p: int) -> torch.Tensor:
    """fp32 [N, C, H, W] logits of pass ``p`` of a LOSS_CASES entry (module docstring: coarse above 4 096 pixels)."""
    n, h, w, c, _ = P.LOSS_CASES[name]
    if n * h * w <= COARSE_ABOVE:
        return P.logits(f"uamt/{name}/pass{p}", n, c, h, w, PASS_SCALE)
    hc, wc = -(-h // CELL), -(-w // CELL)
    z = P.logits(f"uamt/{name}/pass{p}", n, c, hc, wc, PASS_SCALE)
    return z.repeat_interleave(CELL, 2).repeat_interleave(CELL, 3)[:, :, :h, :w].contiguous()


@functools.lru_cache(maxsize=None)
def case_acc(name: str) -> torch.Tensor:
    """Float64 sum of the ``PASSES`` softmaxes of a case.  Shared: callers must not write into it."""
    return accumulate([pass_logits(name, p) for p in range(PASSES)])


@functools.lru_cache(maxsize=None)
def case_threshold(name: str):
    """``(thr as float32, half gap)`` of a case, on the uncertainties of its accumulator ROUNDED TO FLOAT32 (what the kernel reads)."""
    thr, half = gap_threshold(uncertainty(case_acc(name).float(), PASSES))
    return f32(thr), half


@functools.lru_cache(maxsize=None)
def case_reference(name: str, thr: float):
    """``umse_value_and_grad`` of a case at ``thr`` with ``(a, b) = pixel_ref.case_inputs("mse", name)``.  Shared, read-only."""
    a, b = P.case_inputs("mse", name)
    return umse_value_and_grad(a, b, case_acc(name).float(), PASSES, thr)
