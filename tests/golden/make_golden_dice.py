#!/usr/bin/env python
"""Golden vectors of the Dice supervised loss (tests/golden/dice.npz) from the WHEEL's own GeneralizedDiceLoss
(deepclustering2/loss/dice_loss.py:79-135) and the REFERENCE's own TrainEpocher (semi_seg/epocher.py:110-197) given that criterion.

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_dice.py

1. The criterion: for the three shapes of tests/dice_ref.py, pow 1 and 2, with and without class weights, the wheel's
   ``GeneralizedDiceLoss(...)(softmax(z, 1), onehot)`` in float64 and its gradient with respect to the logits (inputs from
   tests/dice_ref.py, ``randn * 2``, bit-reproducible; the gradients are stored as fingerprints with float64 samples).
2. The step: 3 `partial` iterations of the reference epocher with ``sup_criterion=GeneralizedDiceLoss()`` at 64^2, LB = UB = 2,
   4 classes, fp32, Adam lr 1e-3 (weight decay 1e-5).  Recorded: the flip seeds, per-step sup_loss, the meters, the step-1 gradients of
   every parameter and the final parameters of the decoder's tail (fingerprints, samples stored as float32).  Only data is written.

The fixture's own error is handled as in make_golden_entmin.py: iteration 1 runs a second time in float64 and the first model seed,
counting up from 83, whose fp32 gradients lie within HALF of each bound that the test takes over from tests/test_gpu_step.py
(``OWN_ERROR_LIMITS``) of the float64 ones is taken.  The criterion looks at the reference only; the distances are stored under
``own_error/``."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402
import dice_ref  # noqa: E402

DICE = dict(H=64, LB=2, UB=2, NB=3, lr=1e-3, wd=1e-5)
FIRST_MODEL_SEED = 83
OWN_ERROR_LIMITS = dict(logits=1e-5, tail_median=2.5e-3, tail_max=7.5e-3, all_max=1.5e-2)
TAIL = ("Up_conv2", "DeConv_1x1")


def criterion_vectors(out: dict) -> None:
    from deepclustering2.loss.dice_loss import GeneralizedDiceLoss
    for si, shape in enumerate(dice_ref.SHAPES):
        c = shape[1]
        lab = dice_ref.labels(shape)
        onehot = torch.stack([lab == k for k in range(c)], 1).long()
        z = dice_ref.logits(shape, 2)
        for pw in (1, 2):
            for weighted in (0, 1):
                weight = torch.tensor(dice_ref.class_weights(c), dtype=torch.float64) if weighted else None
                z64 = z.double().requires_grad_()
                loss = GeneralizedDiceLoss(pow=pw, weight=weight)(z64.softmax(1), onehot)
                loss.backward()
                key = f"crit/s{si}_p{pw}_w{weighted}"
                out[key + "/loss"] = np.asarray(float(loss), dtype=np.float64)
                out.update(synth.fp_pack(key + "/grad", synth.fingerprint(np_(z64.grad), key + "/grad")))      # float64 samples


def inputs():
    H, LB, UB, NB = DICE["H"], DICE["LB"], DICE["UB"], DICE["NB"]
    T = torch.from_numpy
    lab = [(T(synth.uniform(f"dice/lab{i}", (LB, 1, H, H))), T(synth.integers(f"dice/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"dice/unl{i}", (UB, 1, H, H))) for i in range(NB)]
    return lab, unl


def put_fp32(out, key, tensor):
    fp = synth.fingerprint(np_(tensor), key)
    fp["sample"] = fp["sample"].astype(np.float32)
    out.update(synth.fp_pack(key, fp))


def run(out: dict, model_seed: int, dtype=torch.float32, nb: int = None) -> dict:
    """``nb`` iterations (default: all) of the reference's TrainEpocher in ``dtype``; fills ``out`` and returns the step-1 gradients."""
    from contrastyou.arch import UNet
    from deepclustering2.loss.dice_loss import GeneralizedDiceLoss
    import semi_seg.epocher as ref_epocher
    from oracle import unet as OU
    H, LB, UB, NB = DICE["H"], DICE["LB"], DICE["UB"], nb or DICE["NB"]
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
    model = model.to(dtype)
    names = [n for n, _ in model.named_parameters()]

    class RecordingAdam(torch.optim.Adam):
        grad_log: list = []

        def step(self, closure=None):
            self.grad_log.append({n: p.grad.detach().clone() for n, p in zip(names, self.param_groups[0]["params"])})
            return super().step(closure)

    lab, unl = inputs()

    def loader(imgs, tgts, B):
        for img, tgt in zip(imgs, tgts):
            img = img.to(dtype)
            yield [[[img, tgt], [img.clone(), tgt.clone()]], [f"patient{i:03d}_00_{i}" for i in range(B)], ["0"] * B,
                   [f"patient{i:03d}_00" for i in range(B)]]

    sup_log = []
    gdl = GeneralizedDiceLoss()

    def sup(*a, **k):
        v = gdl(*a, **k)
        sup_log.append(float(v))
        return v

    RecordingAdam.grad_log = []
    opt = RecordingAdam(model.parameters(), lr=DICE["lr"], weight_decay=DICE["wd"])
    seeds, real = [], random.randint

    def spy(a, b):
        v = real(a, b)
        seeds.append(v)
        return v

    ref_epocher.random.randint = spy
    random.seed(2525)
    try:
        ep = ref_epocher.TrainEpocher(model, opt, loader([a for a, _ in lab][:NB], [b for _, b in lab][:NB], LB),
                                      loader(unl[:NB], [torch.zeros(UB, 1, H, H, dtype=torch.long)] * NB, UB), sup, 0.0, NB, 0, "cpu",
                                      feature_position=["Conv5", "Up_conv3", "Up_conv2"], feature_importance=[0.5, 0.25, 0.25])
        res = ep.run()
    finally:
        ref_epocher.random.randint = real
    out["seeds"] = np.asarray(seeds, dtype=np.int64)
    out["sup_loss"] = np.asarray(sup_log, dtype=np.float64)
    flat = {}
    for k, v in res.items():
        for kk, vv in dict(v).items():
            flat[f"{k}/{kk}"] = float(vv)
    out["meter_keys"] = np.asarray(list(flat.keys()))
    out["meter_values"] = np.asarray(list(flat.values()), dtype=np.float64)
    for n, gr in RecordingAdam.grad_log[0].items():
        put_fp32(out, f"grad_step1/{n}", gr)
    for n, v in model.named_parameters():
        if n.startswith(TAIL):
            put_fp32(out, f"param_after/{n}", v)
    return RecordingAdam.grad_log[0]


def own_error(model_seed: int) -> dict:
    """Relative L2 distance of the reference's fp32 step-1 gradients from its float64 ones, summarised as the test summarises its own."""
    g32 = run({}, model_seed, torch.float32, 1)
    g64 = run({}, model_seed, torch.float64, 1)
    rel = {n: float((g32[n].double() - g64[n]).norm() / g64[n].norm()) for n in g64}
    tail = sorted(v for n, v in rel.items() if n.startswith(("Up_conv2", "DeConv")))
    return dict(logits=max(v for n, v in rel.items() if n.startswith("DeConv")), tail_median=tail[len(tail) // 2], tail_max=tail[-1],
                all_max=max(rel.values()))


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    torch.set_num_threads(4)
    out = {}
    criterion_vectors(out)
    for model_seed in range(FIRST_MODEL_SEED, FIRST_MODEL_SEED + 32):
        err = own_error(model_seed)
        ok = all(err[k] < OWN_ERROR_LIMITS[k] for k in OWN_ERROR_LIMITS)
        print(f"model seed {model_seed}: fp32 against float64 {err} -> {'taken' if ok else 'too far from float64'}")
        if ok:
            break
    else:
        raise SystemExit("no model seed whose fp32 gradients are within the limits of the float64 ones")
    out.update({f"own_error/{k}": np.asarray(v) for k, v in err.items()})
    DICE["model_seed"] = model_seed
    run(out, model_seed)
    from contrastyou.arch import UNet
    out["param_names"] = np.asarray([n for n, _ in UNet(1, 4).named_parameters()])
    for k, v in DICE.items():
        out[f"cfg/{k}"] = np.asarray(v)
    save("dice", **out)


if __name__ == "__main__":
    main()
