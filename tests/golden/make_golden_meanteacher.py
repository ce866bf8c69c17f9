#!/usr/bin/env python
"""Golden vectors of the Mean Teacher step (tests/golden/meanteacher.npz) from the REFERENCE's own MeanTeacherEpocher
(contrastyou/epocher/base_epocher.py:129-216) and the wheel's ema_updater (deepclustering2/models/ema.py:96-131).

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_meanteacher.py

3 iterations at 64^2, LB = UB = 2, 4 classes, Adam lr 1e-3 (weight decay 1e-5), consistency weight 10, EMA alpha 0.999 with
weight decay 1e-6.  Student and teacher start from different seeded oracle.unet.init_state dicts; the unlabeled stream carries the
labeled images (the reference reads its unlabeled batch from the labeled one, base_epocher.py:174); the flip transformer is the
semi_seg one (TensorRandomFlip(axis=[1, 2], threshold=0.8)).  Recorded: seeds and alpha per step, per-step sup / reg losses, the
meters, step-1 gradients, the teacher's parameters after the first and the last EMA and its BatchNorm running statistics -- large
tensors as fingerprints.  Only data is written."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, put_fp, save  # noqa: E402
import synth  # noqa: E402

MT = dict(H=64, LB=2, UB=2, NB=3, lr=1e-3, wd=1e-5, weight=10.0, alpha=0.999, ema_wd=1e-6, student_seed=61, teacher_seed=62)


def inputs():
    H, LB, NB = MT["H"], MT["LB"], MT["NB"]
    T = torch.from_numpy
    return [(T(synth.uniform(f"mt/lab{i}", (LB, 1, H, H))), T(synth.integers(f"mt/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from contrastyou.arch import UNet
    from contrastyou.epocher import base_epocher as BE
    from deepclustering2.augment.tensor_augment import TensorRandomFlip
    from deepclustering2.loss import KL_div
    from deepclustering2.models import ema_updater
    from oracle import unet as OU
    torch.set_num_threads(4)
    model, teacher = UNet(1, 4), UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=MT["student_seed"]))
    teacher.load_state_dict(OU.init_state(1, 4, seed=MT["teacher_seed"]))
    for p in teacher.parameters():
        p.detach_()
    out = {}
    names = [n for n, _ in model.named_parameters()]

    class RecordingAdam(torch.optim.Adam):
        grad_log = []

        def step(self, closure=None):
            self.grad_log.append({n: p.grad.detach().clone() for n, p in zip(names, self.param_groups[0]["params"])})
            return super().step(closure)

    opt = RecordingAdam(model.parameters(), lr=MT["lr"], weight_decay=MT["wd"])
    batches = inputs()

    def loader():
        for img, tgt in batches:
            b = len(img)
            yield [[img, tgt], [img.clone(), tgt.clone()]], [f"patient{i:03d}_00_{i}" for i in range(b)], ["0"] * b, \
                [f"patient{i:03d}_00" for i in range(b)]

    losses = {"sup": [], "reg": []}
    kl = KL_div(verbose=False)
    mse = torch.nn.MSELoss()

    def sup(*a, **k):
        v = kl(*a, **k)
        losses["sup"].append(float(v))
        return v

    def reg(*a, **k):
        v = mse(*a, **k)
        losses["reg"].append(float(v))
        return v

    upd = ema_updater(alpha=MT["alpha"], justify_alpha=True, weight_decay=MT["ema_wd"])
    alphas, after = [], []

    def spy_upd(ema_model, student_model):
        k = len(alphas)
        alphas.append(min(1 - 1 / (k + 1), MT["alpha"]))
        upd(ema_model=ema_model, student_model=student_model)
        after.append(({n: p.detach().clone() for n, p in student_model.named_parameters()},
                      {n: b.detach().clone() for n, b in ema_model.state_dict().items()}))

    seeds, real = [], random.randint

    def spy(a, b):
        v = real(a, b)
        seeds.append(v)
        return v

    BE.random.randint = spy
    random.seed(2024)
    try:
        ep = BE.MeanTeacherEpocher(model, teacher, opt, loader(), loader(), num_batches=MT["NB"], sup_criterion=sup, reg_criterion=reg,
                                   cur_epoch=0, device="cpu", transform_axis=[1, 2], reg_weight=MT["weight"], ema_updater=spy_upd)
        ep._transformer = TensorRandomFlip(axis=[1, 2], threshold=0.8)       # the semi_seg epochers' transformer
        # SimpleFineTuneEpoch passes (model, cur_epoch, device) positionally to the wheel's _Epocher(model, num_batches, cur_epoch,
        # device): put the three where the wheel reads them
        ep._num_batches, ep._cur_epoch, ep._device = MT["NB"], 0, torch.device("cpu")
        res = ep.run()
    finally:
        BE.random.randint = real
    out["seeds"] = np.asarray(seeds, dtype=np.int64)
    out["alpha"] = np.asarray(alphas, dtype=np.float64)
    out["sup_loss"] = np.asarray(losses["sup"], dtype=np.float64)
    out["reg_loss"] = np.asarray(losses["reg"], dtype=np.float64)
    flat = {}
    for k, v in res.items():
        for kk, vv in dict(v).items():
            flat[f"{k}/{kk}"] = float(vv)
    out["meter_keys"] = np.asarray(list(flat.keys()))
    out["meter_values"] = np.asarray(list(flat.values()), dtype=np.float64)
    out["param_names"] = np.asarray(names)
    out["buffer_names"] = np.asarray([n for n, _ in teacher.named_buffers()])
    for n, g in opt.grad_log[0].items():
        put_fp(out, f"grad_step1/{n}", g)
    # the teacher after the first EMA (alpha 0: the student's step-1 weights, decayed) and after the last one, with its running
    # statistics (the file stays under the size limit with these two)
    for i in (1, MT["NB"]):
        t = after[i - 1][1]
        for n in names:
            put_fp(out, f"teacher{i}/{n}", t[n])
    for n, _ in teacher.named_buffers():
        if "running" in n:
            put_fp(out, f"teacher{MT['NB']}/{n}", after[-1][1][n])
    for k, v in MT.items():
        out[f"cfg/{k}"] = np.asarray(v)
    save("meanteacher", **out)


if __name__ == "__main__":
    main()
