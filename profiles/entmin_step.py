#!/usr/bin/env python
"""`entmin` against `partial` at BASELINE cfg2 (LB = UB = 16, 256^2, bf16, launch tape on), in one process: warm-up, then the two
trainers' steps alternated in timed blocks with device-synchronised timing; launches per step from each recorded tape; the entropy term
alone (``ops.softmax_entropy``), forward + backward, against the torch composition.  Prints one JSON object.  Kernel statistics come
from a separate rocprofv3 run:

    python profiles/entmin_step.py --repeats 3 --steps 20
    rocprofv3 --kernel-trace --stats -d <dir> -o entmin -- python profiles/entmin_step.py --repeats 1 --steps 10 --no-term
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FEATURES = ["Conv5", "Up_conv3", "Up_conv2"]


def build(kind, device, lb, ub, size, dtype, weight):
    from contrastyou.arch import UNet
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from semi_seg import epocher as E
    from semi_seg.synthetic import SyntheticPairs
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4, compute_dtype=dtype).to(device)
    opt = Adam(model.parameters(), lr=1e-7 * 400, weight_decay=1e-5)
    lab = SyntheticPairs(lb, size, 4, seed=0, device=device)
    unl = SyntheticPairs(ub, size, 4, seed=1, device=device)
    common = dict(feature_position=FEATURES, feature_importance=[0.5, 0.25, 0.25])
    if kind == "partial":
        return E.TrainEpocher(model, opt, iter(lab), iter(unl), KL_div(verbose=False), 0, 1, 0, device, **common)
    return E.EntropyMinEpocher(model, opt, iter(lab), iter(unl), KL_div(verbose=False), weight, 1, 0, device, **common)


def time_steps(drv, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        drv.step()
    drv.ep._flush_records()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def term(device, ub, size, reps):
    """Forward + backward of the entropy term alone on [UB, 4, size, size] fp32 NHWC logits: the fused node against torch."""
    from deepclustering2.loss import Entropy
    from miseg_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    z = torch.randn(ub, 4, size, size, generator=g).to(device).contiguous(memory_format=torch.channels_last).requires_grad_()
    crit = Entropy()

    def fused():
        ops.softmax_entropy(z).backward()

    def composed():
        crit(z.softmax(1)).backward()

    out = {}
    for name, fn in (("fused", fused), ("composed", composed)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out[name + "_ms"] = (time.perf_counter() - t0) * 1e3 / reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lb", type=int, default=16)
    ap.add_argument("--ub", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--weight", type=float, default=1e-5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-term", action="store_true")
    args = ap.parse_args()
    import bench
    device = torch.device("cuda", 0)
    random.seed(0)
    drivers = {k: bench.StepDriver(build(k, device, args.lb, args.ub, args.size, args.dtype, args.weight)) for k in ("partial", "entmin")}
    for drv in drivers.values():      # eager, recorded, then replayed iterations
        time_steps(drv, args.warmup)
    res = {k: [] for k in drivers}
    for _ in range(args.repeats):
        for k, drv in drivers.items():
            res[k].append(time_steps(drv, args.steps))
    out = {"config": vars(args), "ms_per_step": {k: sorted(v) for k, v in res.items()},
           "median_ms": {k: sorted(v)[len(v) // 2] for k, v in res.items()}}
    out["entmin_minus_partial_ms"] = out["median_ms"]["entmin"] - out["median_ms"]["partial"]
    for k, drv in drivers.items():
        tp = drv.ep._step_tape
        out.setdefault("launches_per_step", {})[k] = tp.n_ops if tp is not None and tp.handle else None
        out.setdefault("tape_refused", {})[k] = None if tp is None else tp.disabled
        drv.close()
    if not args.no_term:
        out["entropy_term"] = term(device, args.ub, args.size, reps=20)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
