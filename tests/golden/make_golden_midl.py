#!/usr/bin/env python
"""Golden vectors of the `midl` step (tests/golden/midl.npz) from the REFERENCE's own UDATrainEpocher (semi_seg/epocher.py:200-226)
and its IIDSegmentationSmallPathLoss (contrastyou/losses/iic_loss.py:152-189).

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_midl.py

The reference ships `MIDLPaperParameters` but no epocher that reads it; the subclass below is this project's definition of the term
(DESIGN.md section 12), written on the reference's own classes: the `uda` iteration, whose regulariser is

    x = softmax(flip(unlabeled_logits)), y = softmax(unlabeled_tf_logits)
    reg = cons_weight * MSE(y, x.detach()) + iic_weight * IIDSegmentationSmallPathLoss(padding, patch_size)(x, y)

with reg_weight 1.  3 iterations at 64^2, LB = UB = 2, 4 classes, fp32, Adam lr 1e-3 (weight decay 1e-5), cons_weight 5,
iic_weight 1, two geometries: (a) padding 1, patch 1024 (one window); (b) padding 3, patch 32 (9 overlapping windows).  Recorded per
geometry: the flip seeds, per-step sup / uda / mi losses, the meters, the step-1 gradients and the final parameters of the decoder's tail
(fingerprints, samples stored as float32: the values are fp32).  Only data is written."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402

MIDL = dict(H=64, LB=2, UB=2, NB=3, lr=1e-3, wd=1e-5, cons_weight=5.0, iic_weight=1.0, model_seed=71)
TAIL = ("Up_conv2", "DeConv_1x1")        # the final parameters are recorded for the decoder's tail only (the file's size)
GEOMETRIES = {"a": dict(padding=1, patch_size=1024), "b": dict(padding=3, patch_size=32)}


def inputs():
    H, LB, UB, NB = MIDL["H"], MIDL["LB"], MIDL["UB"], MIDL["NB"]
    T = torch.from_numpy
    lab = [(T(synth.uniform(f"midl/lab{i}", (LB, 1, H, H))), T(synth.integers(f"midl/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"midl/unl{i}", (UB, 1, H, H))) for i in range(NB)]
    return lab, unl


def put_fp32(out, key, tensor):
    fp = synth.fingerprint(np_(tensor), key)
    fp["sample"] = fp["sample"].astype(np.float32)
    out.update(synth.fp_pack(key, fp))


def run(geom: str, out: dict) -> None:
    from contrastyou.arch import UNet
    from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    from deepclustering2.loss import KL_div
    from deepclustering2.meters2 import AverageValueMeter
    import semi_seg.epocher as ref_epocher
    from oracle import unet as OU
    g = GEOMETRIES[geom]
    H, LB, UB, NB = MIDL["H"], MIDL["LB"], MIDL["UB"], MIDL["NB"]
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=MIDL["model_seed"]))
    names = [n for n, _ in model.named_parameters()]

    class RecordingAdam(torch.optim.Adam):
        grad_log: list = []

        def step(self, closure=None):
            self.grad_log.append({n: p.grad.detach().clone() for n, p in zip(names, self.param_groups[0]["params"])})
            return super().step(closure)

    log = {"uda": [], "mi": []}

    class MIDLEpocher(ref_epocher.UDATrainEpocher):
        def _configure_meters(self, meters):
            meters = super()._configure_meters(meters)
            meters.register_meter("mi", AverageValueMeter())
            return meters

        def regularization(self, unlabeled_tf_logits, unlabeled_logits_tf, seed, *args, **kwargs):
            x = unlabeled_logits_tf.softmax(1)          # prob1: the flipped untransformed side (the IIC tap's order)
            y = unlabeled_tf_logits.softmax(1)          # prob2: the transformed side
            uda = self._reg_criterion(y, x.detach())
            mi = self._mi_criterion(x, y)
            self.meters["uda"].add(uda.item())
            self.meters["mi"].add(-mi.item())
            log["uda"].append(float(uda))
            log["mi"].append(float(mi))
            return MIDL["cons_weight"] * uda + MIDL["iic_weight"] * mi

    lab, unl = inputs()

    def loader(imgs, tgts, B):
        for img, tgt in zip(imgs, tgts):
            yield [[[img, tgt], [img.clone(), tgt.clone()]], [f"patient{i:03d}_00_{i}" for i in range(B)], ["0"] * B,
                   [f"patient{i:03d}_00" for i in range(B)]]

    sup_log = []
    kl = KL_div(verbose=False)

    def sup(*a, **k):
        v = kl(*a, **k)
        sup_log.append(float(v))
        return v

    RecordingAdam.grad_log = []
    opt = RecordingAdam(model.parameters(), lr=MIDL["lr"], weight_decay=MIDL["wd"])
    seeds, real = [], random.randint

    def spy(a, b):
        v = real(a, b)
        seeds.append(v)
        return v

    ref_epocher.random.randint = spy
    random.seed(4242)
    try:
        ep = MIDLEpocher(model, opt, loader([a for a, _ in lab], [b for _, b in lab], LB),
                         loader(unl, [torch.zeros(UB, 1, H, H, dtype=torch.long)] * NB, UB), sup, torch.nn.MSELoss(), 1.0, NB, 0,
                         "cpu", feature_position=["Conv5", "Up_conv3", "Up_conv2"], feature_importance=[0.5, 0.25, 0.25])
        ep._mi_criterion = IIDSegmentationSmallPathLoss(lamda=1.0, padding=g["padding"], patch_size=g["patch_size"])
        res = ep.run()
    finally:
        ref_epocher.random.randint = real
    p = f"{geom}/"
    out[p + "seeds"] = np.asarray(seeds, dtype=np.int64)
    out[p + "sup_loss"] = np.asarray(sup_log, dtype=np.float64)
    out[p + "uda"] = np.asarray(log["uda"], dtype=np.float64)
    out[p + "mi_loss"] = np.asarray(log["mi"], dtype=np.float64)
    flat = {}
    for k, v in res.items():
        for kk, vv in dict(v).items():
            flat[f"{k}/{kk}"] = float(vv)
    out[p + "meter_keys"] = np.asarray(list(flat.keys()))
    out[p + "meter_values"] = np.asarray(list(flat.values()), dtype=np.float64)
    for n, gr in RecordingAdam.grad_log[0].items():
        put_fp32(out, f"{p}grad_step1/{n}", gr)
    for n, v in model.named_parameters():
        if n.startswith(TAIL):
            put_fp32(out, f"{p}param_after/{n}", v)
    for k, v in g.items():
        out[f"{p}cfg/{k}"] = np.asarray(v)


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    torch.set_num_threads(4)
    out = {}
    for geom in GEOMETRIES:
        run(geom, out)
    import contrastyou  # noqa: F401  (the reference's, imported by run)
    from contrastyou.arch import UNet
    out["param_names"] = np.asarray([n for n, _ in UNet(1, 4).named_parameters()])
    for k, v in MIDL.items():
        out[f"cfg/{k}"] = np.asarray(v)
    save("midl", **out)


if __name__ == "__main__":
    main()
