#!/usr/bin/env python
"""Golden vectors of ``AffineTensorTransform`` (tests/golden/affine.npz) from the REFERENCE's own class, on the CPU in fp32.

Run in the build container only (needs the reference tree; see make_golden.py; ``MISEG_REFERENCE`` overrides its location):

    python tests/golden/make_golden_affine.py

The reference's file is loaded by path (contrastyou/augment/tensor_affine_transform.py needs numpy and torch alone; its package's
``__init__`` wants torchvision and is not imported).  For each numpy seed s in 0..2, with a default-constructed transform:

    seed{s}/x          a 3 x 5 x 9 x 7 standard-normal input (torch generator seeded 100 + s)
    seed{s}/theta_ind  np.random.seed(s); the matrices of tf(x)                       (independent=True: one per sample)
    seed{s}/y          ... and its bilinear output
    seed{s}/theta_dep  np.random.seed(s); the matrices of tf(x, independent=False)    (one for the batch)
    seed{s}/theta_inv  the matrices tf(y, AffineMatrix=theta_ind, inverse=True) returns (the inverses)
    seed{s}/back       ... and its output: the round trip

Only data is written."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_golden import save  # noqa: E402

SEEDS = (0, 1, 2)
SHAPE = (3, 5, 9, 7)


def load_reference_module():
    ref = os.environ.get("MISEG_REFERENCE") or make_golden.REF
    path = os.path.join(ref, "contrastyou", "augment", "tensor_affine_transform.py")
    spec = importlib.util.spec_from_file_location("reference_tensor_affine_transform", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    ref = load_reference_module()
    out = {}
    for s in SEEDS:
        x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(100 + s))
        tf = ref.AffineTensorTransform()
        np.random.seed(s)
        y, theta_ind = tf(x)
        np.random.seed(s)
        _, theta_dep = tf(x, independent=False)
        back, theta_inv = tf(y, AffineMatrix=theta_ind, inverse=True)
        for key, v in (("x", x), ("theta_ind", theta_ind), ("y", y), ("theta_dep", theta_dep), ("theta_inv", theta_inv), ("back", back)):
            assert v.dtype == torch.float32
            out[f"seed{s}/{key}"] = v
    save("affine", **out)


if __name__ == "__main__":
    main()
