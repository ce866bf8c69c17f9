#!/usr/bin/env python
"""Contrastive decoder pre-training (`Trainer.name=contrastdecoder`) at UB = 16, 256^2, bf16, in one process:
warm-up, then timed blocks of eager pre-training steps with device-synchronised timing; GPU kernel launches per step (torch.profiler);
the local projection head alone, forward + backward on a [32, 32, 128, 128] channels_last feature, the kernels against the ATen
composition of the same head on the same device, with the launches of each; and each new kernel alone (its time and the fraction of
the HBM floor of one pass over the feature).  Prints one JSON object.  Kernel statistics come from a separate rocprofv3 run:

    python profiles/contrast_decoder_step.py --repeats 3 --steps 20
    rocprofv3 --kernel-trace --stats -d <dir> -o contrastdecoder -- python profiles/contrast_decoder_step.py --repeats 1 --steps 10 --no-head --no-count
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from contrast_step import launches, timed  # noqa: E402

HBM_TBS = 6.3      # the roofline the streaming kernels are compared against


def build(device, ub, size, dtype):
    from itertools import chain
    from contrastyou.arch import UNet
    from contrastyou.losses.contrast_loss import SupConLoss
    from contrastyou.trainer._utils import LocalProjectionHead
    from deepclustering2.optim import Adam
    from semi_seg.epocher import PretrainDecoderEpocher
    from semi_seg.synthetic import SyntheticPairs
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4, compute_dtype=dtype).to(device)
    head = LocalProjectionHead(32).to(device)
    model.disable_grad_all()
    model.enable_grad("Up5", "Up_conv3")
    params = chain(*(getattr(model, n).parameters() for n in model._range("Up5", "Up_conv3")), head.parameters())
    opt = Adam(params, lr=1e-6 * 300, weight_decay=0.0)
    loader = iter(SyntheticPairs(ub, size, 4, seed=1, device=device))
    ep = PretrainDecoderEpocher(model, head, opt, loader, SupConLoss(), 1, 0, device, "Up_conv3", (2, 2))
    model.train()
    return ep, loader, head


def head_alone(device, n, hw, dtype, reps, count):
    """Forward + backward of ``LocalProjectionHead.embeddings`` on an [n, 32, hw, hw] channels_last feature of ``dtype``: the kernels
    against the ATen composition (the module's own fallback, run in ``dtype`` as autocast-free eager torch would)."""
    from contrastyou.epocher._utils import unfold_position
    from contrastyou.trainer._utils import LocalProjectionHead
    torch.manual_seed(1)
    head = LocalProjectionHead(32).to(device)
    twin = LocalProjectionHead(32).to(device).to(dtype)
    twin.load_state_dict(head.state_dict())
    feat = torch.randn(n, 32, hw, hw, device=device).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_()
    probe = torch.randn(4 * n, 128, device=device)

    def fused():
        (head.embeddings(feat, 2, (2, 2)) * probe).sum().backward()

    def composed():
        pooled = torch.nn.functional.adaptive_max_pool2d(twin._projector(feat), (4, 4))
        rows = torch.cat([unfold_position(c, (2, 2))[0].reshape(2 * n, -1) for c in torch.chunk(pooled, 2)])
        (rows.float() * probe).sum().backward()

    out = {}
    for name, fn in (("kernels", fused), ("aten", composed)):
        timed(fn, 5)
        out[name + "_ms"] = sorted(timed(fn, reps) for _ in range(3))
        if count:
            out[name + "_launches"] = launches(fn)
    return out


def kernels_alone(device, n, hw, dtype, reps):
    """Each new entry point alone on [n, hw, hw, 32] (64 channels for the LeakyReLU pair, the hidden layer's width): microseconds per
    call and the fraction of the HBM floor of the bytes it must move."""
    from miseg_amd import ops
    out = {}
    es = torch.empty((), dtype=dtype).element_size()
    for c in (32, 64):
        raw = torch.randn(n, c, hw, hw, device=device).to(dtype).contiguous(memory_format=torch.channels_last)
        bias = torch.randn(c, device=device)
        nbytes = raw.numel() * es
        y = ops.bias_lrelu(raw, bias, 0.01)
        yg = y.detach().requires_grad_()
        cases = {f"bias_lrelu_fwd_c{c}": (lambda: ops.bias_lrelu(raw, bias, 0.01), 2 * nbytes)}
        rows, idx = ops.bias_amaxpool(raw, bias, (4, 4), (2, 2), 2, return_indices=True)
        cases[f"bias_amaxpool_fwd_c{c}"] = (lambda: ops.bias_amaxpool(raw, bias, (4, 4), (2, 2), 2), nbytes)
        ge, gy = torch.randn_like(rows), torch.randn_like(raw)
        leaf = raw.detach().requires_grad_()
        biasg = bias.detach().requires_grad_()

        def pool_bwd():
            ops.bias_amaxpool(leaf, biasg, (4, 4), (2, 2), 2).backward(ge)

        def lrelu_bwd():
            ops.bias_lrelu(leaf, biasg, 0.01).backward(gy)

        for name, (fn, moved) in cases.items():
            timed(fn, 5)
            us = min(timed(fn, reps) for _ in range(3)) * 1e3
            out[name] = {"us": us, "floor_us": moved / (HBM_TBS * 1e6), "fraction_of_floor": moved / (HBM_TBS * 1e6) / us}
        # the backward pairs are timed as forward + backward minus the forward measured above
        for name, fn, fwd, moved in ((f"bias_amaxpool_bwd_c{c}", pool_bwd, f"bias_amaxpool_fwd_c{c}", nbytes),
                                     (f"bias_lrelu_bwd_c{c}", lrelu_bwd, f"bias_lrelu_fwd_c{c}", 3 * nbytes)):
            timed(fn, 5)
            us = min(timed(fn, reps) for _ in range(3)) * 1e3 - out[fwd]["us"]
            out[name] = {"us": us, "floor_us": moved / (HBM_TBS * 1e6), "fraction_of_floor": moved / (HBM_TBS * 1e6) / us}
        del yg, idx
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ub", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-head", action="store_true")
    ap.add_argument("--no-count", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    dtype = getattr(torch, args.dtype)
    ep, loader, _ = build(device, args.ub, args.size, args.dtype)
    step = lambda: ep._step(next(loader))  # noqa: E731
    timed(step, args.warmup)
    ms = sorted(timed(step, args.steps) for _ in range(args.repeats))
    out = {"config": vars(args), "ms_per_step": ms, "median_ms": ms[len(ms) // 2]}
    if not args.no_count:
        out["launches_per_step"] = launches(step)
    if not args.no_head:
        out["head_fwd_bwd"] = head_alone(device, 2 * args.ub, args.size // 2, dtype, reps=20, count=not args.no_count)
        out["kernels"] = kernels_alone(device, 2 * args.ub, args.size // 2, dtype, reps=50)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
