#!/usr/bin/env python
"""Golden vectors of the `entmin` step (tests/golden/entmin.npz) from the REFERENCE's own TrainEpocher (semi_seg/epocher.py:110-197)
and the wheel's Entropy (deepclustering2/loss/kl_losses.py:20-49).

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_entmin.py

The reference ships `EntropyMinParameters` (and imports Entropy, semi_seg/epocher.py:18) but has no epocher that reads it; the subclass
below is this project's definition of the term, written on the reference's own classes: the `partial` iteration,
whose regulariser is

    reg   = Entropy(reduction="mean", eps=1e-16)(softmax(unlabeled_logits_tf, 1))      unlabeled_logits_tf = flip(f(x)), ref :160-161
          = mean_{n,h,w} -sum_c p_c * log(p_c + 1e-16)
    total = sup_loss + weight * reg                                                     weight = the epocher's reg_weight

3 iterations at 64^2, LB = UB = 2, 4 classes, fp32, Adam lr 1e-3 (weight decay 1e-5), weight 1.0 (at the shipped 1e-5 the term would
vanish in the gradients and the fixture would pin nothing).  Recorded: the flip seeds, per-step sup_loss / entropy, the meters, the
step-1 gradients of every parameter and the final parameters of the decoder's tail (fingerprints, samples stored as float32: the
values are fp32).  Only data is written.

The fixture's own error.  A ReLU whose input sits within fp32 rounding of zero takes the other branch in fp32 than in exact
arithmetic, and one such flip in the last decoder block moves that block's gradients by ~5e-3 relative (tests/test_gpu_step.py).  The
test takes over test_gpu_step's first-iteration bounds (logits layer 2e-5, last block median 5e-3 / worst 1.5e-2, any tensor 3e-2), so a
fixture that is itself that far from the exact gradients cannot be held to them.  The generator therefore runs iteration 1 a second
time in float64 -- the same reference classes, the same inputs -- and takes the first model seed, counting up from 83, whose fp32
gradients lie within HALF of each of those bounds of the float64 ones (``OWN_ERROR_LIMITS``).  The criterion looks at the reference
only.  The measured distances are stored under ``own_error/``."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402

ENTMIN = dict(H=64, LB=2, UB=2, NB=3, lr=1e-3, wd=1e-5, weight=1.0)
FIRST_MODEL_SEED = 83
# half of the bounds tests/test_gpu_entmin.py::test_epocher_matches_the_reference_run takes over from test_gpu_step
OWN_ERROR_LIMITS = dict(logits=1e-5, tail_median=2.5e-3, tail_max=7.5e-3, all_max=1.5e-2)
TAIL = ("Up_conv2", "DeConv_1x1")        # the final parameters are recorded for the decoder's tail only (the file's size)


def inputs():
    H, LB, UB, NB = ENTMIN["H"], ENTMIN["LB"], ENTMIN["UB"], ENTMIN["NB"]
    T = torch.from_numpy
    lab = [(T(synth.uniform(f"entmin/lab{i}", (LB, 1, H, H))), T(synth.integers(f"entmin/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"entmin/unl{i}", (UB, 1, H, H))) for i in range(NB)]
    return lab, unl


def put_fp32(out, key, tensor):
    fp = synth.fingerprint(np_(tensor), key)
    fp["sample"] = fp["sample"].astype(np.float32)
    out.update(synth.fp_pack(key, fp))


def run(out: dict, model_seed: int, dtype=torch.float32, nb: int = None) -> dict:
    """``nb`` iterations (default: all) of the reference epocher in ``dtype``; fills ``out`` and returns the step-1 gradients."""
    from contrastyou.arch import UNet
    from deepclustering2.loss import Entropy, KL_div
    from deepclustering2.meters2 import AverageValueMeter
    import semi_seg.epocher as ref_epocher
    from oracle import unet as OU
    H, LB, UB, NB = ENTMIN["H"], ENTMIN["LB"], ENTMIN["UB"], nb or ENTMIN["NB"]
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
    model = model.to(dtype)
    names = [n for n, _ in model.named_parameters()]

    class RecordingAdam(torch.optim.Adam):
        grad_log: list = []

        def step(self, closure=None):
            self.grad_log.append({n: p.grad.detach().clone() for n, p in zip(names, self.param_groups[0]["params"])})
            return super().step(closure)

    log = []
    entropy = Entropy()

    class EntMinEpocher(ref_epocher.TrainEpocher):
        def _configure_meters(self, meters):
            meters = super()._configure_meters(meters)
            meters.register_meter("entropy", AverageValueMeter())
            return meters

        def regularization(self, unlabeled_tf_logits, unlabeled_logits_tf, seed, *args, **kwargs):
            reg = entropy(unlabeled_logits_tf.softmax(1))
            self.meters["entropy"].add(reg.item())
            log.append(float(reg))
            return reg

    lab, unl = inputs()

    def loader(imgs, tgts, B):
        for img, tgt in zip(imgs, tgts):
            img = img.to(dtype)
            yield [[[img, tgt], [img.clone(), tgt.clone()]], [f"patient{i:03d}_00_{i}" for i in range(B)], ["0"] * B,
                   [f"patient{i:03d}_00" for i in range(B)]]

    sup_log = []
    kl = KL_div(verbose=False)

    def sup(*a, **k):
        v = kl(*a, **k)
        sup_log.append(float(v))
        return v

    RecordingAdam.grad_log = []
    opt = RecordingAdam(model.parameters(), lr=ENTMIN["lr"], weight_decay=ENTMIN["wd"])
    seeds, real = [], random.randint

    def spy(a, b):
        v = real(a, b)
        seeds.append(v)
        return v

    ref_epocher.random.randint = spy
    random.seed(2424)
    try:
        ep = EntMinEpocher(model, opt, loader([a for a, _ in lab][:NB], [b for _, b in lab][:NB], LB),
                           loader(unl[:NB], [torch.zeros(UB, 1, H, H, dtype=torch.long)] * NB, UB), sup, ENTMIN["weight"], NB, 0, "cpu",
                           feature_position=["Conv5", "Up_conv3", "Up_conv2"], feature_importance=[0.5, 0.25, 0.25])
        res = ep.run()
    finally:
        ref_epocher.random.randint = real
    out["seeds"] = np.asarray(seeds, dtype=np.int64)
    out["sup_loss"] = np.asarray(sup_log, dtype=np.float64)
    out["entropy"] = np.asarray(log, dtype=np.float64)
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
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    torch.set_num_threads(4)
    for model_seed in range(FIRST_MODEL_SEED, FIRST_MODEL_SEED + 32):
        err = own_error(model_seed)
        ok = all(err[k] < OWN_ERROR_LIMITS[k] for k in OWN_ERROR_LIMITS)
        print(f"model seed {model_seed}: fp32 against float64 {err} -> {'taken' if ok else 'too far from float64'}")
        if ok:
            break
    else:
        raise SystemExit("no model seed whose fp32 gradients are within the limits of the float64 ones")
    out = {f"own_error/{k}": np.asarray(v) for k, v in err.items()}
    ENTMIN["model_seed"] = model_seed
    run(out, model_seed)
    from contrastyou.arch import UNet
    out["param_names"] = np.asarray([n for n, _ in UNet(1, 4).named_parameters()])
    for k, v in ENTMIN.items():
        out[f"cfg/{k}"] = np.asarray(v)
    save("entmin", **out)


if __name__ == "__main__":
    main()
