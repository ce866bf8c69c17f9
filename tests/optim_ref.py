"""The three update rules the wheel ships beside torch's optimisers (whl:deepclustering2/optim/radam.py:16-91, adabound.py:67-136,
199-270), restated in plain torch on explicit tensors, with a dtype argument: float32 is what the wheel's RAdam computes in
(``p.data.float()``), float64 is the yardstick of the HIP kernels.  The scalars of a step (``*_scalars``) are Python doubles, as in
the wheel; they are what ``FusedRAdam`` / ``FusedAdaBound``'s ``host_step`` must return.

Cases: the golden files' (tests/golden/make_golden_optim.py), stated once here -- the generator imports them."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

STEPS, NUMEL = 8, 1000
RADAM_CASES = {            # steps 1-5 unrectified, 6-8 rectified, for each beta2
    "radam/b999_wd1e-2": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
    "radam/b9_wd0": dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8, weight_decay=0),
    "radam/b999_wd1e-5": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5),
}
# final_lr and gamma put the clamp to work: the bounds close in on final_lr like 1 -+ 1 / (gamma t), and the per-element rates
# lr sqrt(bc2) / bc1 / (sqrt(v) + eps) of unit-normal gradients spread around 2e-3 (the generator prints how many elements sit on either
# bound at every step).  ``lr_at``: step -> the learning rate a scheduler sets before that step.
_BOUND = dict(lr=1e-3, betas=(0.9, 0.999), final_lr=2e-3, gamma=0.5, eps=1e-8)
# Both classes at weight decay 0 and 1e-2, each with amsbound off and on, and one case whose learning rate moves.  ``file``: the golden
# file that holds the case (the float64 states of one case are 190-250 KB, so the nine cases take three files).
ADABOUND_CASES = {
    "adabound/wd0": dict(kind="AdaBound", weight_decay=0, amsbound=False, file="optim_adabound", **_BOUND),
    "adabound/wd1e-2_ams": dict(kind="AdaBound", weight_decay=1e-2, amsbound=True, file="optim_adabound", **_BOUND),
    "adaboundw/wd1e-2": dict(kind="AdaBoundW", weight_decay=1e-2, amsbound=False, file="optim_adabound", **_BOUND),
    "adaboundw/wd1e-2_ams_lr": dict(kind="AdaBoundW", weight_decay=1e-2, amsbound=True, lr_at={5: 5e-4, 7: 2.5e-4}, file="optim_adabound", **_BOUND),
    "adabound/wd0_ams": dict(kind="AdaBound", weight_decay=0, amsbound=True, file="optim_adabound2", **_BOUND),
    "adabound/wd1e-2": dict(kind="AdaBound", weight_decay=1e-2, amsbound=False, file="optim_adabound2", **_BOUND),
    "adaboundw/wd0": dict(kind="AdaBoundW", weight_decay=0, amsbound=False, file="optim_adabound2", **_BOUND),
    "adaboundw/wd0_ams": dict(kind="AdaBoundW", weight_decay=0, amsbound=True, file="optim_adabound3", **_BOUND),
    "adaboundw/wd1e-2_ams": dict(kind="AdaBoundW", weight_decay=1e-2, amsbound=True, file="optim_adabound3", **_BOUND),
}


def golden_file(name: str) -> str:
    """The golden file (without its suffix) that holds the case ``name``."""
    return "optim" if name in RADAM_CASES else ADABOUND_CASES[name]["file"]


def ctor_args(cfg: dict) -> dict:
    return {k: v for k, v in cfg.items() if k not in ("kind", "lr_at", "file")}


def lr_of(cfg: dict, t: int) -> float:
    lr = cfg["lr"]
    for step, value in sorted(cfg.get("lr_at", {}).items()):
        if t >= step:
            lr = value
    return lr


# ------------------------------------------------------------------------------------------------------------------ RAdam
def radam_scalars(t: int, lr: float, betas, eps: float, weight_decay: float) -> List[float]:
    """[step size, rectified as 1.0 / 0.0, eps, weight decay x lr] of step ``t`` (radam.py:55-80)."""
    b1, b2 = betas
    beta2_t = b2 ** t
    n_sma_max = 2 / (1 - b2) - 1
    n_sma = n_sma_max - 2 * t * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        step_size = lr * math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) \
            / (1 - b1 ** t)
    else:
        step_size = lr / (1 - b1 ** t)
    return [step_size, 1.0 if n_sma >= 5 else 0.0, eps, weight_decay * lr]


def radam_step(p, g, m, v, t: int, lr: float, betas, eps: float, weight_decay: float) -> None:
    """One step in place, in the tensors' dtype, in the wheel's order of operations (radam.py:46-87)."""
    b1, b2 = betas
    step_size, rectified, _, _ = radam_scalars(t, lr, betas, eps, weight_decay)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    m.mul_(b1).add_(g, alpha=1 - b1)
    if weight_decay != 0:
        p.add_(p, alpha=-weight_decay * lr)
    if rectified:
        p.addcdiv_(m, v.sqrt().add_(eps), value=-step_size)
    else:
        p.add_(m, alpha=-step_size)


# ------------------------------------------------------------------------------------------------------------------ AdaBound / AdaBoundW
def adabound_scalars(t: int, lr: float, base_lr: float, betas, final_lr: float, gamma: float, eps: float, weight_decay: float) -> List[float]:
    """[step size, lower bound, eps, weight decay, upper bound] of step ``t`` (adabound.py:122-130)."""
    b1, b2 = betas
    step_size = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    final = final_lr * lr / base_lr
    return [step_size, final * (1 - 1 / (gamma * t + 1)), eps, weight_decay, final * (1 + 1 / (gamma * t))]


def adabound_step(p, g, m, v, vmax: Optional[torch.Tensor], t: int, lr: float, base_lr: float, betas, final_lr: float, gamma: float,
                  eps: float, weight_decay: float, decoupled: bool) -> None:
    """One step in place (adabound.py:108-134; decoupled: 240-268); ``vmax`` = the amsbound variant's running maximum, or None."""
    b1, b2 = betas
    step_size, lower, _, _, upper = adabound_scalars(t, lr, base_lr, betas, final_lr, gamma, eps, weight_decay)
    if weight_decay != 0 and not decoupled:
        g = g.add(p, alpha=weight_decay)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    if vmax is not None:
        torch.max(vmax, v, out=vmax)
        denom = vmax.sqrt().add_(eps)
    else:
        denom = v.sqrt().add_(eps)
    step = torch.full_like(denom, step_size).div_(denom).clamp_(lower, upper).mul_(m)
    if weight_decay != 0 and decoupled:
        decayed = torch.mul(p, weight_decay)
        p.add_(-step)
        p.sub_(decayed)
    else:
        p.add_(-step)


# ------------------------------------------------------------------------------------------------------------------ whole runs
def run(name: str, p0: torch.Tensor, grads, dtype) -> List[Dict[str, torch.Tensor]]:
    """The case ``name`` from ``p0`` over ``grads`` in ``dtype``: per step, clones of p / m / v (/ vmax) after it."""
    cfg = {**RADAM_CASES, **ADABOUND_CASES}[name]
    p = p0.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    vmax = torch.zeros_like(p) if cfg.get("amsbound") else None
    out = []
    for t, g in enumerate(grads, 1):
        g = g.to(dtype)
        if name in RADAM_CASES:
            radam_step(p, g, m, v, t, **cfg)
        else:
            a = ctor_args(cfg)
            adabound_step(p, g, m, v, vmax, t, lr_of(cfg, t), cfg["lr"], a["betas"], a["final_lr"], a["gamma"], a["eps"], a["weight_decay"],
                          cfg["kind"] == "AdaBoundW")
        out.append({"p": p.clone(), "m": m.clone(), "v": v.clone(), **({} if vmax is None else {"vmax": vmax.clone()})})
    return out


def scalars(name: str, t: int) -> List[float]:
    cfg = {**RADAM_CASES, **ADABOUND_CASES}[name]
    if name in RADAM_CASES:
        return radam_scalars(t, **cfg)
    a = ctor_args(cfg)
    return adabound_scalars(t, lr_of(cfg, t), cfg["lr"], a["betas"], a["final_lr"], a["gamma"], a["eps"], a["weight_decay"])
