#!/usr/bin/env python
"""Golden vectors of the `contrast` pre-training step (tests/golden/contrast.npz) from the REFERENCE's own classes: PretrainEncoderEpoch
(contrastyou/epocher/contrast_epocher.py:21-113), ProjectionHead (contrastyou/trainer/_utils.py:44-65), SupConLoss
(contrastyou/losses/contrast_loss.py), UNetFeatureExtractor("Conv5") and GlobalLabelGenerator.

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_contrast.py

3 iterations at 64^2, B = 4 samples per view (N = 8 embedding rows), fp32, group_option="partition" with partitions 0 1 0 1 of two
patients: every anchor has three positives and four negatives.  Adam lr 1e-4 (weight decay 1e-5) over every parameter, the decoder's
gradients disabled, as the reference's trainer sets it up (contrast_trainer.py:74-78, :98-99).  The model is
``oracle.unet.init_state``; the projector's weights and the two views come from ``synth`` (the test rebuilds them from the same tags,
so they are not stored).  Recorded: the labels, the per-step loss, the projector's raw output of iteration 1, the step-1 gradients of every encoder and projector parameter and the
encoder's parameters after the third step (fingerprints, samples stored as float32: the values are fp32).  Only data is written.

The fixture's own error.  A ReLU whose input sits within fp32 rounding of zero takes the other branch in fp32 than in exact
arithmetic, so the reference's fp32 gradients are themselves some distance from the exact ones.  The generator runs iteration 1 a second
time in float64 -- the same classes, the same inputs -- and stores the relative L2 distance fp32 <-> float64 per parameter group
(``own_error/projector``, ``own_error/Conv5``, ``own_error/Conv1-4``), measured on the fingerprint samples, i.e. on the entries the test
compares.  The test allows 4 x that distance per group, floored at 2e-5 and capped at 3e-2; the generator takes the first model seed,
counting up from 83, for which 4 x the distance stays under the cap in every group.  The criterion looks at the reference only."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402

CONTRAST = dict(H=64, B=4, NB=3, lr=1e-4, wd=1e-5, output_dim=256, position="Conv5")
PARTITIONS = ["0", "1", "0", "1"]
PATIENTS = ["patient001_00", "patient001_00", "patient002_00", "patient002_00"]
FIRST_MODEL_SEED = 83
FACTOR, CAP = 4.0, 3e-2
GROUPS = ("projector", "Conv5", "Conv1-4")


def group_of(name: str) -> str:
    if name.startswith("_header"):
        return "projector"
    return "Conv5" if name.startswith("Conv5") else "Conv1-4"


def projector_state() -> dict:
    """The mlp ProjectionHead(256, 256)'s state: seeded normals at the scale of nn.Linear's default initialisation."""
    T = torch.from_numpy
    return {"_header.2.weight": T(synth.normal("contrast/proj/w1", (256, 256), scale=1.0 / 16)),
            "_header.2.bias": T(synth.normal("contrast/proj/b1", (256,), scale=1.0 / 16)),
            "_header.4.weight": T(synth.normal("contrast/proj/w2", (CONTRAST["output_dim"], 256), scale=1.0 / 16)),
            "_header.4.bias": T(synth.normal("contrast/proj/b2", (CONTRAST["output_dim"],), scale=1.0 / 16))}


def views(i: int):
    H, B = CONTRAST["H"], CONTRAST["B"]
    return torch.from_numpy(synth.uniform(f"contrast/img{i}", (B, 1, H, H))), torch.from_numpy(synth.uniform(f"contrast/tf{i}", (B, 1, H, H)))


def put_fp32(out, key, tensor):
    fp = synth.fingerprint(np_(tensor), key)
    fp["sample"] = fp["sample"].astype(np.float32)
    out.update(synth.fp_pack(key, fp))


def run(out: dict, model_seed: int, dtype=torch.float32, nb: int = None) -> dict:
    """``nb`` iterations (default: all) of the reference epocher in ``dtype``; fills ``out`` and returns the step-1 gradients by name
    (encoder parameters under their model names, the projector's under ``_header.*``)."""
    import itertools
    from contrastyou.arch import UNet, UNetFeatureExtractor
    from contrastyou.epocher.contrast_epocher import PretrainEncoderEpoch
    from contrastyou.losses.contrast_loss import SupConLoss
    from contrastyou.trainer._utils import ProjectionHead
    from oracle import unet as OU
    H, B, NB = CONTRAST["H"], CONTRAST["B"], nb or CONTRAST["NB"]
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
    model = model.to(dtype)
    projector = ProjectionHead(input_dim=UNet.dimension_dict[CONTRAST["position"]], output_dim=CONTRAST["output_dim"], head_type="mlp")
    projector.load_state_dict(projector_state())
    projector = projector.to(dtype)
    model.disable_grad_all()
    model.enable_grad(from_="Conv1", util=CONTRAST["position"])
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad] + list(projector.named_parameters())
    assert all(n.startswith("Conv") for n, _ in named[:-4])

    class RecordingAdam(torch.optim.Adam):
        grad_log: list = []

        def step(self, closure=None):
            self.grad_log.append({n: p.grad.detach().clone() for n, p in named})
            return super().step(closure)

    losses, labels_seen = [], []
    criterion = SupConLoss()

    def crit(features, labels=None):
        v = criterion(features, labels=labels)
        losses.append(float(v))
        labels_seen.append(list(labels))
        return v

    def loader():
        tgt = torch.zeros(B, 1, H, H, dtype=torch.long)
        for i in range(NB):
            a, b = views(i)
            yield [[[a.to(dtype), tgt], [b.to(dtype), tgt.clone()]], [f"{p}_{j}" for j, p in enumerate(PATIENTS)], list(PARTITIONS), list(PATIENTS)]

    embeddings = []
    projector.register_forward_hook(lambda mod, args, result: embeddings.append(result.detach().clone()))
    RecordingAdam.grad_log = []
    opt = RecordingAdam(itertools.chain(model.parameters(), projector.parameters()), lr=CONTRAST["lr"], weight_decay=CONTRAST["wd"])
    decoder_before = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    ep = PretrainEncoderEpoch(model, projector, opt, loader(), crit, num_batches=NB, cur_epoch=0, device="cpu", group_option="partition",
                              feature_extractor=UNetFeatureExtractor(CONTRAST["position"]))
    # PretrainEncoderEpoch passes (model, cur_epoch, device) positionally to the wheel's _Epocher(model, num_batches, cur_epoch, device):
    # put the three fields where the wheel's run() reads them (as make_golden_meanteacher.py does for the same base class)
    ep._num_batches, ep._cur_epoch, ep._device = NB, 0, torch.device("cpu")
    ep.run()
    assert all(torch.equal(p, decoder_before[n]) for n, p in model.named_parameters() if n in decoder_before)
    out["labels"] = np.asarray(labels_seen[0], dtype=np.int32)
    out["loss"] = np.asarray(losses, dtype=np.float64)
    out["embeddings_step1"] = np_(embeddings[0]).astype(np.float32)       # the projector's raw output [2 B, output_dim] of iteration 1
    for n, gr in RecordingAdam.grad_log[0].items():
        put_fp32(out, f"grad_step1/{n}", gr)
    for n, p in named:
        if n.startswith("Conv"):
            put_fp32(out, f"param_after/{n}", p)
    out["param_names"] = np.asarray([n for n, _ in named])
    return RecordingAdam.grad_log[0]


def group_distance(ga: dict, gb: dict) -> dict:
    """Relative L2 distance per parameter group on the fingerprint samples -- the test's own measure."""
    num, den = {g: 0.0 for g in GROUPS}, {g: 0.0 for g in GROUPS}
    for n in gb:
        idx = synth.sample_index(gb[n].numel(), f"grad_step1/{n}")
        a, b = np_(ga[n]).reshape(-1).astype(np.float64)[idx], np_(gb[n]).reshape(-1).astype(np.float64)[idx]
        num[group_of(n)] += float(((a - b) ** 2).sum())
        den[group_of(n)] += float((b ** 2).sum())
    return {g: (num[g] / den[g]) ** 0.5 for g in GROUPS}


def own_error(model_seed: int) -> dict:
    g32 = run({}, model_seed, torch.float32, 1)
    g64 = run({}, model_seed, torch.float64, 1)
    return group_distance(g32, g64)


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    torch.set_num_threads(4)
    for model_seed in range(FIRST_MODEL_SEED, FIRST_MODEL_SEED + 32):
        err = own_error(model_seed)
        ok = all(FACTOR * v < CAP for v in err.values())
        print(f"model seed {model_seed}: fp32 against float64 {err} -> {'taken' if ok else 'too far from float64'}")
        if ok:
            break
    else:
        raise SystemExit("no model seed whose fp32 gradients are close enough to the float64 ones")
    out = {f"own_error/{k}": np.asarray(v) for k, v in err.items()}
    CONTRAST["model_seed"] = model_seed
    run(out, model_seed)
    for k, v in CONTRAST.items():
        out[f"cfg/{k}"] = np.asarray(v)
    out["partitions"], out["patients"] = np.asarray(PARTITIONS), np.asarray(PATIENTS)
    save("contrast", **out)


if __name__ == "__main__":
    main()
