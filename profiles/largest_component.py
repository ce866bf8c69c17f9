#!/usr/bin/env python
"""``ops.largest_component`` on the device against its host twin (``scipy.ndimage.label``) on the same tensors: rank 2, connectivity 1,
classes 1..3, Dice counts on, at 16 x 256 x 256 on random discs and on 55 % noise, plus one 512 x 512 spiral (the long chain).  Per
case 5 warm-up and 20 timed calls between ``torch.cuda.Event`` pairs with a final synchronise, median [min .. max] in microseconds;
the host twin is timed with the wall clock around the same call (it starts and ends with device tensors, as the epocher would use
it).  Prints one JSON object:

    python profiles/largest_component.py            # both paths
    python profiles/largest_component.py --device   # the device path only (for a kernel trace)
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

WARMUP, TIMED = 5, 20


def timed_events(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(TIMED):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    torch.cuda.synchronize()
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def timed_wall(fn, warmup=1, timed=5):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "calls": timed}


def main():
    import component_ref
    import surface_ref
    from miseg_amd import ops
    assert torch.cuda.is_available(), "needs a GPU"
    os.environ.pop("MISEG_COMPONENTS_HOST", None)
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    discs_p, discs_t = surface_ref.discs(16, 256, seed=5)
    noise = np.where(rng.random((16, 256, 256)) < 0.55, rng.integers(1, 4, (16, 256, 256)), 0).astype(np.int64)
    spiral, _ = component_ref.spiral(512)
    cases = (("discs", discs_p, discs_t), ("noise", noise, discs_t), ("spiral", spiral, np.zeros_like(spiral)))
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "timed": TIMED, "cases": []}
    for name, p, t in cases:
        dp, dt = torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev)
        n, h, w = p.shape
        ws = torch.empty(ops.query("miseg_largest_component_ws_bytes", n, h, w, 3, 2), dtype=torch.uint8, device=dev)

        def device():
            return ops.largest_component(dp, (1, 2, 3), target=dt, num_classes=4, ws=ws)

        def host():
            os.environ["MISEG_COMPONENTS_HOST"] = "1"
            try:
                return ops.largest_component(dp, (1, 2, 3), target=dt, num_classes=4)
            finally:
                del os.environ["MISEG_COMPONENTS_HOST"]

        row = {"case": name, "shape": [n, h, w], "device": timed_events(device)}
        # what a call must move: pred in, out out (8 bytes each), target in (8), and the two 4-byte label planes written and read once
        row["floor_bytes"] = n * h * w * (8 + 8 + 8 + 4 * 4)
        if "--device" not in sys.argv:
            row["host"] = timed_wall(host)
            a, b = device(), host()
            row["equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][0], b[2][0])
                                and torch.equal(a[2][1], b[2][1]))
            row["components"] = a[1][..., 0].sum(0).tolist()
        out["cases"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
