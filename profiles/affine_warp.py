#!/usr/bin/env python
"""``ops.affine_warp`` against torch's ``F.affine_grid`` + ``F.grid_sample`` on the same device, forward and forward + backward, in one
process: per shape and memory order 5 warm-up and 20 timed calls between ``torch.cuda.Event`` pairs, median [min .. max] in
microseconds, and the bytes a call must move (read the input once, write the output once; twice that with the backward) with the
bandwidth that floor would mean at the median.  Matrices: the class's default ranges under a fixed numpy seed.  Prints one JSON object
(DESIGN.md section 21):

    python profiles/affine_warp.py
"""
from __future__ import annotations

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

CASES = (((16, 4, 256, 256), True), ((16, 16, 256, 256), False), ((16, 16, 256, 256), True), ((16, 64, 64, 64), False),
         ((16, 64, 64, 64), True))
WARMUP, TIMED = 5, 20


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e) * 1e3)
    return {"median_us": round(statistics.median(ms), 1), "min_us": round(min(ms), 1), "max_us": round(max(ms), 1)}


def main():
    from contrastyou.augment import AffineTensorTransform
    from miseg_amd import ops
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "timed": TIMED, "cases": []}
    for shape, channels_last in CASES:
        n, c, h, w = shape
        np.random.seed(0)
        tf = AffineTensorTransform()
        theta = torch.stack([tf.get_random_affinematrix() for _ in range(n)])
        theta_dev = theta.to(dev)
        reach = ops.affine_reach(theta, h, w)
        x = torch.randn(*shape, device=dev)
        g = torch.randn(*shape, device=dev)
        if channels_last:
            x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
        xg = x.clone().requires_grad_(True)

        def torch_fwd(inp=x):
            return F.grid_sample(inp, F.affine_grid(theta_dev, list(shape), align_corners=True), mode="bilinear", padding_mode="zeros",
                                 align_corners=True)

        def hip_fwd(inp=x):
            return ops.affine_warp(inp, theta_dev, reach=reach)

        def both(fwd):
            def run():
                xg.grad = None
                fwd(xg).backward(g)
            return run

        nbytes = x.numel() * 4 * 2
        row = {"shape": list(shape), "channels_last": channels_last, "reach": reach, "floor_bytes_fwd": nbytes, "floor_bytes_fwd_bwd": 2 * nbytes,
               "hip_fwd": timed(hip_fwd), "torch_fwd": timed(torch_fwd), "hip_fwd_bwd": timed(both(hip_fwd)), "torch_fwd_bwd": timed(both(torch_fwd))}
        row["hip_fwd_floor_GBps"] = round(nbytes / row["hip_fwd"]["median_us"] * 1e-3, 1)
        row["hip_fwd_bwd_floor_GBps"] = round(2 * nbytes / row["hip_fwd_bwd"]["median_us"] * 1e-3, 1)
        err = float((hip_fwd() - torch_fwd()).abs().max())
        row["max_abs_difference_to_torch_fwd"] = err
        out["cases"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
