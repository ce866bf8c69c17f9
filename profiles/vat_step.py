#!/usr/bin/env python
"""The `vat` step and the stem's data-gradient kernel at BASELINE cfg2 (LB = UB = 16, 256^2, bf16), the numbers of DESIGN.md section 23.
Device-synchronised host timing, every shape warmed up, the variants of a comparison alternated in timed blocks inside one process.
Prints one JSON object.

    python profiles/vat_step.py --kinds partial uda vat        # steps of this tree (vat runs eagerly, the others under the launch tape)
    python profiles/vat_step.py --root <other tree> --kinds partial uda --no-kernel     # the same trainers from another checkout
    python profiles/vat_step.py --kinds                         # the kernel comparison alone

``--kinds vat`` also times the phases of one iteration on their own (each behind a synchronise, so they add up to more than the
pipelined step): the clean forward of the unlabeled batch, one direction pass (forward + data-gradient backward to the image), the
perturbed forward.  The kernel comparison is ``miseg_conv3x3_stem_dgrad`` against the generic path (channel-padded dgrad-packed
weight through the streaming convolution) on [32, 16, 256, 256] in bf16 and fp32."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

FEATURES = ["Conv5", "Up_conv3", "Up_conv2"]


def build(kind, device, lb, ub, size, dtype):
    import torch
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
    kl = KL_div(verbose=False)
    if kind == "partial":
        return E.TrainEpocher(model, opt, iter(lab), iter(unl), kl, 0, 1, 0, device, **common)
    if kind == "uda":
        return E.UDATrainEpocher(model, opt, iter(lab), iter(unl), kl, torch.nn.MSELoss(), 5.0, 1, 0, device, **common)
    return E.VATEpocher(model, opt, iter(lab), iter(unl), kl, 1.0, 1, 0, device, **common)


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def time_steps(drv, n):
    def step():
        drv.step()
    ms = timed(step, n)
    drv.ep._flush_records()
    return ms


def phases(device, ub, size, dtype, reps):
    """The three kinds of pass inside ``VATLoss.forward`` on their own, [UB, 1, size, size]."""
    import torch
    from contrastyou.arch import UNet
    from miseg_amd import ops, unet_ops
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4, compute_dtype=dtype).to(device).train()
    x = torch.rand(ub, 1, size, size, device=device)
    with torch.no_grad():
        pred = model(x)

    def clean():
        with torch.no_grad():
            model(x)

    def direction():
        xh = x.clone().requires_grad_()
        with unet_ops.bn_untracked(), unet_ops.data_grad_only():
            adv = ops.softmax_kl_consistency(model(xh), pred, None)
        torch.autograd.grad(adv, xh)

    def perturbed():
        with unet_ops.bn_untracked():
            ops.softmax_kl_consistency(model(x), pred, None)

    out = {}
    for name, fn in (("clean_forward", clean), ("direction_pass", direction), ("perturbed_forward", perturbed)):
        timed(fn, 5)
        out[name + "_ms"] = timed(fn, reps)
    return out


def kernel(device, n, cout, size, reps, rounds):
    """``ops.stem_dgrad`` against ``unet_ops.stem_dgrad_generic`` on [n, cout, size, size], alternated; median of the rounds."""
    import torch
    from miseg_amd import ops, unet_ops
    out = {}
    for name, dt in (("bfloat16", torch.bfloat16), ("float32", torch.float32)):
        g = torch.Generator().manual_seed(0)
        graw = torch.randn(n, cout, size, size, generator=g).to(device=device, dtype=dt).contiguous(memory_format=torch.channels_last)
        w = torch.randn(cout, 1, 3, 3, generator=g).to(device)
        fns = {"kernel": lambda: ops.stem_dgrad(graw, w), "generic": lambda: unet_ops.stem_dgrad_generic(graw, w, unet_ops.vec_of(dt))}
        a, b = fns["kernel"]().double(), fns["generic"]()[:, :1].double()
        res = {k: [] for k in fns}
        for fn in fns.values():
            timed(fn, 20)
        for _ in range(rounds):
            for k, fn in fns.items():
                res[k].append(timed(fn, reps) * 1e3)
        npix = n * size * size
        out[name] = {"us": {k: sorted(v) for k, v in res.items()}, "median_us": {k: sorted(v)[len(v) // 2] for k, v in res.items()},
                     "kernel_bytes": npix * (graw.element_size() * cout + 4), "max_abs_difference": float((a - b).abs().max()),
                     "max_abs_value": float(a.abs().max())}
        out[name]["kernel_GBps"] = out[name]["kernel_bytes"] / out[name]["median_us"]["kernel"] * 1e-3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    ap.add_argument("--kinds", nargs="*", default=["partial", "uda", "vat"])
    ap.add_argument("--lb", type=int, default=16)
    ap.add_argument("--ub", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-kernel", action="store_true")
    args = ap.parse_args()
    for p in (args.root, os.path.join(args.root, "mi-based-regularized-semi-supervised-segmentation_amd")):
        sys.path.insert(0, p)
    import torch
    import bench
    device = torch.device("cuda", 0)
    random.seed(0)
    out = {"config": vars(args)}
    drivers = {k: bench.StepDriver(build(k, device, args.lb, args.ub, args.size, args.dtype)) for k in args.kinds}
    for drv in drivers.values():      # eager, recorded, then replayed iterations
        time_steps(drv, args.warmup)
    res = {k: [] for k in drivers}
    for _ in range(args.repeats):
        for k, drv in drivers.items():
            res[k].append(time_steps(drv, args.steps))
    out["ms_per_step"] = {k: sorted(v) for k, v in res.items()}
    out["median_ms"] = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    for k, drv in drivers.items():
        tp = drv.ep._step_tape
        out.setdefault("tape", {})[k] = "eager" if tp is None else ("refused: " + str(tp.disabled) if tp.disabled else f"{tp.replays} replays")
        drv.close()
    if "vat" in args.kinds:
        out["vat_phases"] = phases(device, args.ub, args.size, args.dtype, reps=10)
    if not args.no_kernel:
        out["stem_dgrad"] = kernel(device, args.lb + args.ub, 16, args.size, reps=50, rounds=7)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
