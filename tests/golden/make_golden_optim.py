#!/usr/bin/env python
"""Golden vectors of the wheel's RAdam, AdaBound and AdaBoundW (tests/golden/optim.npz, optim_adabound{,2,3}.npz) from the WHEEL'S OWN
classes: ``deepclustering2/optim/radam.py`` and ``adabound.py`` are read out of the reference's vendored wheel into a throw-away
directory and loaded as two stand-alone modules (they import ``math`` and ``torch`` only, and run under a current torch).

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_optim.py

Every case (tests/optim_ref.py states them) steps ONE 1000-element parameter through the same 8 recorded gradients; recorded are the
parameter and the optimiser's state tensors after every step, and the key names of ``state_dict()``.  The parameter and the gradients
are drawn in float32; the AdaBound cases run on their float64 images (the wheel's AdaBound computes in the parameter's dtype, its
RAdam always in float32), so the same inputs feed a float32 kernel exactly.  Four files: the float64 states of one AdaBound case are
190-250 KB, and a committed file has a size limit (each case names its file, tests/optim_ref.py).  Only data is written."""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, save  # noqa: E402
import optim_ref as R  # noqa: E402
import synth  # noqa: E402


def load_wheel_optimisers():
    scratch = tempfile.mkdtemp(prefix="miseg_whl_optim_")
    mods = {}
    with zipfile.ZipFile(os.path.join(REF, "deepclustering2-2.0.0-py3-none-any.whl")) as z:
        for name in ("radam", "adabound"):
            path = z.extract(f"deepclustering2/optim/{name}.py", scratch)
            spec = importlib.util.spec_from_file_location(f"whl_optim_{name}", path)
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    return mods["radam"].RAdam, mods["adabound"].AdaBound, mods["adabound"].AdaBoundW


def inputs():
    p0 = torch.from_numpy(synth.normal("optim/p", (R.NUMEL,)))
    grads = [torch.from_numpy(synth.normal(f"optim/g{t}", (R.NUMEL,))) for t in range(1, R.STEPS + 1)]
    return p0, grads


def record(out, name, cls, cfg, p0, grads, dtype):
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = cls([p], **R.ctor_args(cfg))
    counts = []
    for t, g in enumerate(grads, 1):
        opt.param_groups[0]["lr"] = R.lr_of(cfg, t)          # what a scheduler does between steps
        p.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[p]
        assert st["step"] == t
        out[f"{name}/p{t}"] = p.detach().clone()
        out[f"{name}/m{t}"] = st["exp_avg"].clone()
        out[f"{name}/v{t}"] = st["exp_avg_sq"].clone()
        if "max_exp_avg_sq" in st:
            out[f"{name}/vmax{t}"] = st["max_exp_avg_sq"].clone()
        if "final_lr" in cfg:        # where the clamp bites: the rate of every element against the step's bounds
            step_size, lower, eps, _, upper = R.scalars(name, t)
            rate = step_size / (st.get("max_exp_avg_sq", st["exp_avg_sq"]).double().sqrt() + eps)
            counts.append([int((rate <= lower).sum()), int((rate >= upper).sum()), int(((rate > lower) & (rate < upper)).sum())])
    sd = opt.state_dict()
    out[f"{name}/state_keys"] = np.asarray(sorted(sd["state"][0].keys()))
    out[f"{name}/group_keys"] = np.asarray(sorted(sd["param_groups"][0].keys()))
    out[f"{name}/step_type"] = np.asarray(type(sd["state"][0]["step"]).__name__)
    if counts:
        out[f"{name}/clamp_counts"] = np.asarray(counts, dtype=np.int64)         # per step: on the lower bound, on the upper, on neither
        print(f"{name}: elements on the lower bound / on the upper bound / on neither, per step: {counts}")
        total = np.asarray(counts).sum(0)
        assert (total > 0).all(), f"{name}: the clamp never reaches one of its three regimes: {total}"


def main():
    torch.set_num_threads(1)
    RAdam, AdaBound, AdaBoundW = load_wheel_optimisers()
    p0, grads = inputs()
    out = {"p0": p0, **{f"g{t}": g for t, g in enumerate(grads, 1)}}
    for name, cfg in R.RADAM_CASES.items():
        record(out, name, RAdam, cfg, p0, grads, torch.float32)
        flags = [R.scalars(name, t)[1] for t in range(1, R.STEPS + 1)]
        assert flags == [0.0] * 5 + [1.0] * 3, (name, flags)                     # unrectified through step 5, rectified from step 6
    save("optim", **out)
    files = {}
    for name, cfg in R.ADABOUND_CASES.items():
        record(files.setdefault(cfg["file"], {}), name, {"AdaBound": AdaBound, "AdaBoundW": AdaBoundW}[cfg["kind"]], cfg, p0, grads,
               torch.float64)
    for file, out in files.items():
        save(file, **out)


if __name__ == "__main__":
    main()
