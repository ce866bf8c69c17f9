"""Shared by tests/test_cpu_mi_loss_ref.py and tests/test_gpu_mi_loss.py: the case tables, inputs, float64 reference and bounds of the
small kernels that turn a K x K joint into the mutual-information loss and its gradient -- csrc/mi_global.hip (six entry points) and
the local-MI loss epilogue of csrc/mi_local.hip (loss_displacement, local_loss_kernel, local_loss_disp_kernel,
local_loss_finish_kernel) -- in the pattern of heads_var_ref.py.

Reference: oracle/iic.py (iid_loss, global_joint, local_mi_from_raw, local_mi_grad_wrt_raw) in float64 on the float32 inputs; the
gradients of the global losses by autograd on that float64 oracle.

Global inputs: S = 3 sub-heads with different data each (keyed draws of tests/golden/synth.py), "independent" (synth.probs) or
"peaked" (synth.peaked_pair); every (N, K) of GLOBAL_NK at lambda 1.0 and 1.5; the gradient is that of (loss * WTS).sum().  N = 1 peaked
is left out (its joint is a near-delta, the loss scale collapses and the fp32 oracle itself is at 1e-4 of it); K = 1 is no member of a
family: its joint is [[1]] and both losses and every gradient are exactly 0.
compute_joint: S = 2 pairs (one independent, one peaked), symmetric or not, a synth.normal cotangent.
Local epilogue: synthetic raw[P = 2, T, T, K, K], "rand" (uniform * 3 + 0.01) or "peak" (diagonal 5..6, off-diagonal <= 0.02, one
entry of each window exactly 0: after the min shift it is eps only), lambda 1.0 and 1.5.  K = 1 expects loss and grad_raw exactly 0.

Errors.  Losses over the sum of |summands| (the entropy scale of test_gpu_mi.py's docstring), gradients over max |g64| (per sub-head /
window), joints over their largest entry.  One bound per family and quantity: min(10 x E32, CAP), E32 the LARGEST error over the
family's cases of the same oracle evaluated in float32 on the CPU against its float64 value (the maximum, so that a lucky 1e-10 of one
case is nobody's bound); the margin of 10 as in heads_var_ref.py (the kernels add in another order and use the device's logf); CAP the
project's standing figure (1e-5 losses and joints, 2e-4 global gradients, 1e-4 = LOCAL_BWD_ATOL for grad_raw).  No bound is taken from a
kernel's output.  Computed on these tables where the tests run (test_cpu_mi_loss_ref.py prints them and asserts 10 x E32 < CAP for
every family; the figures move with the CPU's summation order -- another machine gave 9.8e-08 for local_loss and 9.7e-06 for
global_grad -- and stay below the caps):

  family         E32       bound
  global_loss    6.52e-08  6.52e-07
  global_nl      6.52e-08  6.52e-07
  global_joint   7.30e-07  7.30e-06
  global_grad    1.59e-05  1.59e-04
  cj_value       6.16e-07  6.16e-06
  cj_grad        3.55e-07  3.55e-06
  local_loss     6.88e-08  6.88e-07
  local_grad     4.01e-07  4.01e-06
"""
from __future__ import annotations

import functools

import torch

import synth
from oracle import iic as OI

F64, F32 = torch.float64, torch.float32
LAMBS = (1.0, 1.5)

# ----------------------------------------------------------------------------------------------------------------- tables
S_GLOBAL = 3
WTS = (1.0, -2.0, 0.5)                      # upstream of the three sub-heads
GLOBAL_NK = [(1, 2), (2, 3), (7, 5), (16, 20), (48, 20), (300, 2), (300, 20), (16, 33), (7, 64), (300, 64), (1, 64), (16, 1)]
GLOBAL_KINDS = ("independent", "peaked")
# every family member: K >= 2, and no N = 1 peaked
GLOBAL_CASES = [(n, k, kind) for n, k in GLOBAL_NK if k >= 2 for kind in GLOBAL_KINDS if not (n == 1 and kind == "peaked")]
GLOBAL_K1 = [(n, k) for n, k in GLOBAL_NK if k == 1]

S_JOINT = 2
JOINT_NK = [(1, 2), (24, 7), (300, 33), (7, 64)]
JOINT_CASES = [(n, k, sym) for n, k in JOINT_NK for sym in (True, False)]

P_LOCAL = 2
LOCAL_KINDS = ("rand", "peak")
LDS_BUDGET = 156 * 1024                     # kLdsBudget of csrc/mi_local.h
SINGLE_WAVES = 16                           # local_loss_kernel: 1024 threads, one LDS slice per wave


def single_block_lds(k: int) -> int:
    """Dynamic LDS of miseg_iic_local_loss_fwd: per wave P, G, R [K*K] and 4 K marginals' logarithms / ratios."""
    return SINGLE_WAVES * (3 * k * k + 4 * k) * 4


SINGLE_MAX_K = max(k for k in range(1, 65) if single_block_lds(k) <= LDS_BUDGET)          # 28
LOCAL_SINGLE = [(k, pad) for k in (1, 2, 3, 5, 8, 20, 28) for pad in (0, 1, 2, 3)]
LOCAL_WS = LOCAL_SINGLE + [(k, pad) for k in (29, 32, 33, 48, 64) for pad in (0, 2)] + [(32, 1)]

CAPS = dict(global_loss=1e-5, global_nl=1e-5, global_joint=1e-5, global_grad=2e-4, cj_value=1e-5, cj_grad=2e-4, local_loss=1e-5,
            local_grad=1e-4)
FAMILIES = tuple(CAPS)


def _T(a):
    return torch.from_numpy(a)


# ----------------------------------------------------------------------------------------------------------------- global MI
@functools.lru_cache(maxsize=None)
def global_inputs(n: int, k: int, kind: str):
    """-> (xs, ys) [S, N, K] fp32, different data per sub-head."""
    xs, ys = [], []
    for s in range(S_GLOBAL):
        tag = f"mi_loss/global/{kind}/n{n}_k{k}/s{s}"
        if kind == "peaked":
            x, y = synth.peaked_pair(tag, (n, k))
        else:
            x, y = synth.probs(tag + "/x", (n, k)), synth.probs(tag + "/y", (n, k))
        xs.append(_T(x))
        ys.append(_T(y))
    return torch.stack(xs), torch.stack(ys)


def global_eval(xs, ys, lamb: float, dtype, loss_fn=OI.iid_loss):
    """The oracle per sub-head in ``dtype`` -> dict(loss [S], nl [S], joint [S,K,K], gx, gy [S,N,K] of (loss * WTS).sum()), float64."""
    out = dict(loss=[], nl=[], joint=[], gx=[], gy=[])
    for s in range(xs.shape[0]):
        x, y = xs[s].to(dtype).requires_grad_(True), ys[s].to(dtype).requires_grad_(True)
        loss, nl, p = loss_fn(x, y, lamb)
        gx, gy = torch.autograd.grad(loss * WTS[s], [x, y])
        for key, v in zip(out, (loss, nl, p, gx, gy)):
            out[key].append(v.detach().to(F64))
    return {k: torch.stack(v) for k, v in out.items()}


def entropy_scale(p, lamb: float, eps: float) -> float:
    """Sum of |summands| of -sum P (log P - lamb log Pj - lamb log Pi) over the last two dims of a float64 joint."""
    row, col = p.sum(-1, keepdim=True), p.sum(-2, keepdim=True)
    return float((p * (torch.log(p + eps).abs() + lamb * torch.log(row + eps).abs() + lamb * torch.log(col + eps).abs())).sum())


def global_errors(got, ref, lamb: float):
    """Per family, the largest error over the sub-heads of ``got`` (dict as global_eval, any float type) against the float64 ``ref``."""
    e = dict(global_loss=0.0, global_nl=0.0, global_joint=0.0, global_grad=0.0)
    for s in range(ref["loss"].shape[0]):
        p = ref["joint"][s]
        e["global_loss"] = max(e["global_loss"], abs(float(got["loss"][s]) - float(ref["loss"][s])) / entropy_scale(p, lamb, OI.GLOBAL_EPS))
        e["global_nl"] = max(e["global_nl"], abs(float(got["nl"][s]) - float(ref["nl"][s])) / entropy_scale(p, 1.0, OI.GLOBAL_EPS))
        e["global_joint"] = max(e["global_joint"], float((got["joint"][s].to(F64) - p).abs().max() / p.max()))
        gs = float(max(ref["gx"][s].abs().max(), ref["gy"][s].abs().max()))
        for k in ("gx", "gy"):
            e["global_grad"] = max(e["global_grad"], float((got[k][s].to(F64) - ref[k][s]).abs().max()) / gs)
    return e


@functools.lru_cache(maxsize=None)
def global_reference(n: int, k: int, kind: str, lamb: float):
    """-> dict(ref = float64 outputs, fp32 = the fp32 oracle's errors per family).  Computed once and shared; treat as read-only."""
    xs, ys = global_inputs(n, k, kind)
    ref = global_eval(xs, ys, lamb, F64)
    return dict(ref=ref, fp32=global_errors(global_eval(xs, ys, lamb, F32), ref, lamb))


# ----------------------------------------------------------------------------------------------------------------- compute_joint
@functools.lru_cache(maxsize=None)
def joint_inputs(n: int, k: int):
    """-> (xs, ys) [2, N, K] fp32 (pair 0 independent, pair 1 peaked) and the cotangent [2, K, K]."""
    tag = f"mi_loss/joint/n{n}_k{k}"
    x1, y1 = synth.peaked_pair(tag + "/peaked", (n, k))
    xs = torch.stack([_T(synth.probs(tag + "/x", (n, k))), _T(x1)])
    ys = torch.stack([_T(synth.probs(tag + "/y", (n, k))), _T(y1)])
    return xs, ys, _T(synth.normal(tag + "/cot", (S_JOINT, k, k)))


def joint_eval(xs, ys, cot, symmetric: bool, dtype):
    out = dict(joint=[], gx=[], gy=[])
    for s in range(xs.shape[0]):
        x, y = xs[s].to(dtype).requires_grad_(True), ys[s].to(dtype).requires_grad_(True)
        p = OI.global_joint(x, y, symmetric)
        gx, gy = torch.autograd.grad((p * cot[s].to(dtype)).sum(), [x, y])
        for key, v in zip(out, (p, gx, gy)):
            out[key].append(v.detach().to(F64))
    return {k: torch.stack(v) for k, v in out.items()}


def joint_errors(got, ref):
    e = dict(cj_value=0.0, cj_grad=0.0)
    for s in range(ref["joint"].shape[0]):
        e["cj_value"] = max(e["cj_value"], float((got["joint"][s].to(F64) - ref["joint"][s]).abs().max() / ref["joint"][s].max()))
        gs = float(max(ref["gx"][s].abs().max(), ref["gy"][s].abs().max()))
        for k in ("gx", "gy"):
            e["cj_grad"] = max(e["cj_grad"], float((got[k][s].to(F64) - ref[k][s]).abs().max()) / gs)
    return e


@functools.lru_cache(maxsize=None)
def joint_reference(n: int, k: int, symmetric: bool):
    xs, ys, cot = joint_inputs(n, k)
    ref = joint_eval(xs, ys, cot, symmetric, F64)
    return dict(ref=ref, fp32=joint_errors(joint_eval(xs, ys, cot, symmetric, F32), ref))


# ----------------------------------------------------------------------------------------------------------------- local epilogue
@functools.lru_cache(maxsize=None)
def local_inputs(k: int, pad: int, kind: str):
    """-> raw [P, T, T, K, K] fp32, different data per window."""
    t = 2 * pad + 1
    tag = f"mi_loss/local/{kind}/k{k}_p{pad}"
    u = _T(synth.uniform(tag + "/u", (P_LOCAL, t, t, k, k)))
    if kind == "rand":
        return u * 3.0 + 0.01
    raw = u * 0.02
    d = _T(synth.uniform(tag + "/d", (P_LOCAL, t, t, k)))
    raw.diagonal(dim1=3, dim2=4).copy_(5.0 + d)
    raw[0, 0, 0, 0, k - 1] = 0.0                 # the window's minimum: eps only after the shift
    raw[1, t - 1, t - 1, k - 1, 0] = 0.0
    return raw


def local_eval(raw, lamda: float, dtype):
    """-> dict(loss [P], grad [P,T,T,K,K]) of the oracle's epilogue and its closed-form gradient in ``dtype``, as float64."""
    r = raw.to(dtype)
    return dict(loss=torch.stack([OI.local_mi_from_raw(w, lamda) for w in r]).to(F64),
                grad=torch.stack([OI.local_mi_grad_wrt_raw(w, lamda) for w in r]).to(F64))


def local_loss_scale(raw64, lamda: float) -> float:
    """Sum of |summands| / T^2 of one window's loss (float64 raw [T,T,K,K])."""
    t = raw64.shape[0]
    s = raw64 - raw64.min() + OI.LOCAL_EPS
    q = s / s.sum(dim=(2, 3), keepdim=True)
    return entropy_scale((q + q.transpose(2, 3)) / 2.0, lamda, OI.LOCAL_EPS) / float(t * t)


def local_errors(got, ref, raw, lamda: float):
    e = dict(local_loss=0.0, local_grad=0.0)
    for p in range(raw.shape[0]):
        e["local_loss"] = max(e["local_loss"], abs(float(got["loss"][p]) - float(ref["loss"][p])) / local_loss_scale(raw[p].to(F64), lamda))
        e["local_grad"] = max(e["local_grad"], float((got["grad"][p].to(F64) - ref["grad"][p]).abs().max() / ref["grad"][p].abs().max()))
    return e


@functools.lru_cache(maxsize=None)
def local_reference(k: int, pad: int, kind: str, lamda: float):
    raw = local_inputs(k, pad, kind)
    ref = local_eval(raw, lamda, F64)
    return dict(ref=ref, fp32=local_errors(local_eval(raw, lamda, F32), ref, raw, lamda) if k >= 2 else None)


# ----------------------------------------------------------------------------------------------------------------- bounds
@functools.lru_cache(maxsize=None)
def e32():
    """family -> the largest fp32-oracle error over the family's cases."""
    e = dict.fromkeys(FAMILIES, 0.0)

    def fold(d):
        for k, v in d.items():
            e[k] = max(e[k], v)

    for n, k, kind in GLOBAL_CASES:
        for lamb in LAMBS:
            fold(global_reference(n, k, kind, lamb)["fp32"])
    for n, k, sym in JOINT_CASES:
        fold(joint_reference(n, k, sym)["fp32"])
    for k, pad in LOCAL_WS:
        if k >= 2:
            for kind in LOCAL_KINDS:
                for lamda in LAMBS:
                    fold(local_reference(k, pad, kind, lamda)["fp32"])
    return e


@functools.lru_cache(maxsize=None)
def bounds():
    return {k: min(10.0 * v, CAPS[k]) for k, v in e32().items()}
