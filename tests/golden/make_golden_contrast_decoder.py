#!/usr/bin/env python
"""Golden vectors of the `contrastdecoder` pre-training step (tests/golden/contrast_decoder.npz) from the REFERENCE's own classes:
PretrainDecoderEpoch (contrastyou/epocher/contrast_epocher.py:116-176), LocalProjectionHead (contrastyou/trainer/_utils.py:68-93),
SupConLoss (contrastyou/losses/contrast_loss.py), UNetFeatureExtractor("Up_conv3"), LocalLabelGenerator and unfold_position.

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_contrast_decoder.py

3 iterations at 64^2, B = 4 samples per view, fp32, Adam lr 1e-4 without weight decay over every parameter with the gradients enabled
for Up5 .. Up_conv3 only, as the reference's trainer sets it up (contrast_trainer.py:116-146).  Partitions 0 0 1 0 of patients p1 p1 p1
p2: samples 0 and 1 share a label per block, so such an anchor has three positives.  The model is ``oracle.unet.init_state``; the
projector's weights and the two views come from ``synth`` (tests/contrast_decoder_ref.py rebuilds them from the same tags, so they are
not stored).  Python's ``random`` is seeded with the first seed, from 0 up, whose first-iteration flip masks contain all of 0, 1, 2, 3.

Recorded: the flip masks of every iteration, the labels, the pooled projector output of iteration 1 ([8, 32, 4, 4]), the per-step
loss, the step-1 gradients of every trained parameter and those parameters after the third step (fingerprints, samples stored as
float32).  Only data is written.

The fixture's own error and the choice of the model seed.  Between the second convolution's output and everything in front of it sit
the pool's arg-max and the LeakyReLU: an input within fp32 rounding of a branch takes the other side in fp32 than in exact arithmetic,
and that is not small.  So for the 16 model seeds 83 .. 98 the generator runs iteration 1 in fp32 and in float64 -- the same classes,
the same inputs -- and stores the relative L2 distance per parameter group on the fingerprint samples
(``own_error/<seed>/<group>``; groups projector.2, projector.0, Up_conv3, Up3-5).  It also stores, for the seed it takes, the float64
minimum top-two gap of the pooling windows and the maximum absolute fp32 <-> float64 distance of the second convolution's output over
the three iterations (``pool_gap_min``, ``conv_out_dist_max``; the float64 side is the forward of each iteration evaluated in float64
from the fp32 run's own weights, inputs and flips), and the smallest ratio, over the 3 x 4 096 windows, of a window's top-two gap to
the largest distance inside that window (``pool_margin_min``).  The fixture is built at the first seed where (a) that ratio is at
least 8 -- a rounding difference cannot move an arg-max; if no seed that passes (b) reaches 8, at the one with the largest ratio,
which must exceed 2 (measured: 3.2, 3.9, 2.1, 0.4 for the seeds 86, 87, 95, 98 that pass (b); 87 is taken); the global form, smallest gap >= 8 x largest distance anywhere, holds for
none of the 16 seeds: the smallest of 12 288 gaps is 2e-6 .. 5e-5, the largest distance ~2e-5, at the output's largest entries -- and (b) its own error is at most a quarter of
the largest own error among the 16 in every group, or at most 2e-5, the floor of the test's bound: the last convolution's gradients
sit at ~1.9e-5 for every seed (no branch lies between them and the loss), so a quarter of their largest is below all of them.  The
test's bound per group is max(4 x the seed's own error, the largest own error among the 16 seeds, 2e-5), capped at 3e-2.  Every
criterion looks at the reference only."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402
from contrast_decoder_ref import GROUPS, golden_projector_state, golden_views, group_of  # noqa: E402

CFG = dict(H=64, B=4, NB=3, lr=1e-4, wd=0.0, position="Up_conv3", grad_from="Up5")
PARTITIONS = ["0", "0", "1", "0"]
PATIENTS = ["patient001_00", "patient001_00", "patient001_00", "patient002_00"]
MODEL_SEEDS = list(range(83, 99))
GAP_FACTOR = 8.0
FLOOR = 2e-5


def put_fp32(out, key, tensor):
    fp = synth.fingerprint(np_(tensor), key)
    fp["sample"] = fp["sample"].astype(np.float32)
    out.update(synth.fp_pack(key, fp))


class RecordingFlip:
    """The epocher's TensorRandomFlip, with the decisions of each call noted (peeked from ``random``'s state, which is put back)."""

    def __init__(self, inner):
        self.inner, self.masks = inner, []

    def __call__(self, x):
        state = random.getstate()
        fh, fw = random.random() < 0.5, random.random() < 0.5
        random.setstate(state)
        y = self.inner(x)
        want = x.flip(1) if fh else x
        want = want.flip(2) if fw else want
        assert torch.equal(y, want)
        self.masks.append(int(fh) | (int(fw) << 1))
        return y


def run(out: dict, model_seed: int, py_seed: int, dtype=torch.float32, nb: int = None, shadow: bool = False) -> dict:
    """``nb`` iterations (default: all) of the reference epocher in ``dtype``; fills ``out`` and returns what the seed choice needs.
    ``shadow``: every iteration's forward up to the second convolution's output is also evaluated in float64 from the SAME weights,
    inputs and flips (copies of the modules as they stand at that iteration) -- ``conv_out64``."""
    import copy
    import itertools
    from contrastyou.arch import UNet, UNetFeatureExtractor
    from contrastyou.epocher.contrast_epocher import PretrainDecoderEpoch
    from contrastyou.losses.contrast_loss import SupConLoss
    from contrastyou.trainer._utils import LocalProjectionHead
    from oracle import unet as OU
    H, B, NB = CFG["H"], CFG["B"], nb or CFG["NB"]
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
    model = model.to(dtype)
    projector = LocalProjectionHead(UNet.dimension_dict[CFG["position"]], head_type="mlp", output_size=(4, 4))
    projector.load_state_dict(golden_projector_state())
    projector = projector.to(dtype)
    model.disable_grad_all()
    model.enable_grad(from_=CFG["grad_from"], util=CFG["position"])
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad] + list(projector.named_parameters())
    assert all(n.startswith("Up") for n, _ in named[:-4])

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
        labels_seen.append([int(x) for x in labels])
        return v

    def loader():
        tgt = torch.zeros(B, 1, H, H, dtype=torch.long)
        for i in range(NB):
            a, b = golden_views(i, B, H)
            yield [[[a.to(dtype), tgt], [b.to(dtype), tgt.clone()]], [f"{p}_{j}" for j, p in enumerate(PATIENTS)], list(PARTITIONS), list(PATIENTS)]

    pooled, conv_out = [], []
    projector.register_forward_hook(lambda mod, args, result: pooled.append(result.detach().clone()))
    projector._projector.register_forward_hook(lambda mod, args, result: conv_out.append(result.detach().clone()))
    RecordingAdam.grad_log = []
    opt = RecordingAdam(itertools.chain(model.parameters(), projector.parameters()), lr=CFG["lr"], weight_decay=CFG["wd"])
    frozen_before = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    ep = PretrainDecoderEpoch(model, projector, opt, loader(), crit, num_batches=NB, cur_epoch=0, device="cpu",
                              feature_extractor=UNetFeatureExtractor(CFG["position"]))
    # the epocher passes (model, cur_epoch, device) positionally to the wheel's _Epocher(model, num_batches, cur_epoch, device): put the
    # three fields where the wheel's run() reads them (as make_golden_contrast.py does for the same base class)
    ep._num_batches, ep._cur_epoch, ep._device = NB, 0, torch.device("cpu")
    flips = ep._transformer = RecordingFlip(ep._transformer)
    conv_out64 = []
    if shadow:
        extractor = UNetFeatureExtractor(CFG["position"])

        def exact_forward(mod, args, kwargs):
            twin = UNet(1, 4).double()
            twin.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
            twin.train()
            head = copy.deepcopy(projector._projector)
            head._forward_hooks.clear()
            head = head.double()
            with torch.no_grad():
                _, *features = twin(args[0].double(), return_features=True)
                dn = extractor(features)[0]
                first, second = torch.chunk(dn, 2, dim=0)
                second = torch.stack([x.flip([d + 1 for d in (0, 1) if m >> d & 1]) if m else x for x, m in zip(second, flips.masks[-B:])])
                conv_out64.append(head(torch.cat([first, second])))

        model.register_forward_pre_hook(exact_forward, with_kwargs=True)
    random.seed(py_seed)
    ep.run()
    assert all(torch.equal(p, frozen_before[n]) for n, p in model.named_parameters() if n in frozen_before)
    assert len(flips.masks) == 2 * B * NB
    masks = [flips.masks[2 * B * i: 2 * B * i + B] for i in range(NB)]
    assert all(flips.masks[2 * B * i + B: 2 * B * (i + 1)] == masks[i] for i in range(NB))      # the feature flip replays the image flip
    out["masks"] = np.asarray(masks, dtype=np.int32)
    out["labels"] = np.asarray(labels_seen[0], dtype=np.int32)
    assert all(lab == labels_seen[0] for lab in labels_seen)
    out["loss"] = np.asarray(losses, dtype=np.float64)
    out["pooled_step1"] = np_(pooled[0]).astype(np.float32)
    for n, gr in RecordingAdam.grad_log[0].items():
        put_fp32(out, f"grad_step1/{n}", gr)
    for n, p in named:
        put_fp32(out, f"param_after/{n}", p)
    out["param_names"] = np.asarray([n for n, _ in named])
    return dict(grads=RecordingAdam.grad_log[0], conv_out=conv_out, conv_out64=conv_out64, masks=masks)


def group_distance(ga: dict, gb: dict) -> dict:
    """Relative L2 distance per parameter group on the fingerprint samples -- the test's own measure."""
    num, den = {g: 0.0 for g in GROUPS}, {g: 0.0 for g in GROUPS}
    for n in gb:
        idx = synth.sample_index(gb[n].numel(), f"grad_step1/{n}")
        a, b = np_(ga[n]).reshape(-1).astype(np.float64)[idx], np_(gb[n]).reshape(-1).astype(np.float64)[idx]
        num[group_of(n)] += float(((a - b) ** 2).sum())
        den[group_of(n)] += float((b ** 2).sum())
    return {g: (num[g] / den[g]) ** 0.5 for g in GROUPS}


def pool_margin(model_seed: int, py_seed: int):
    """(float64 minimum top-two gap of the 4 x 4 adaptive windows, maximum |fp32 - float64| of the second convolution's output) over all
    iterations of the fp32 run.  The float64 side is evaluated from the fp32 run's own weights at each iteration (``run(shadow=True)``):
    two separate runs drift apart by Adam's sign-like steps (~lr per step and weight), which is no rounding difference."""
    r32 = run({}, model_seed, py_seed, torch.float32, shadow=True)
    assert len(r32["conv_out"]) == len(r32["conv_out64"]) == CFG["NB"]
    gap, dist, ratio = float("inf"), 0.0, float("inf")

    def windows(t):
        n, c, h, w = t.shape
        return t.view(n, c, 4, h // 4, 4, w // 4).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 4, 4, -1)

    for a, b in zip(r32["conv_out"], r32["conv_out64"]):
        top = windows(b).topk(2, dim=-1).values
        gaps = top[..., 0] - top[..., 1]
        moved = windows((a.double() - b).abs()).max(dim=-1).values
        gap = min(gap, float(gaps.min()))
        dist = max(dist, float(moved.max()))
        ratio = min(ratio, float((gaps / moved).min()))
    return gap, dist, ratio


def first_py_seed() -> int:
    from deepclustering2.decorator import FixRandomSeed
    for s in range(1000):
        random.seed(s)
        with FixRandomSeed(random.randint(0, int(1e5))):
            masks = {int(random.random() < 0.5) | (int(random.random() < 0.5) << 1) for _ in range(CFG["B"])}
        if masks == {0, 1, 2, 3}:
            return s
    raise SystemExit("no seed of Python's random gives all four flip masks in the first iteration")


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    torch.set_num_threads(4)
    py_seed = first_py_seed()
    own = {}
    for model_seed in MODEL_SEEDS:
        g32 = run({}, model_seed, py_seed, torch.float32, 1)["grads"]
        g64 = run({}, model_seed, py_seed, torch.float64, 1)["grads"]
        own[model_seed] = group_distance(g32, g64)
        print(f"model seed {model_seed}: fp32 against float64 {own[model_seed]}")
    worst = {g: max(own[s][g] for s in MODEL_SEEDS) for g in GROUPS}
    margins = {}
    for model_seed in MODEL_SEEDS:
        if not all(own[model_seed][g] <= max(worst[g] / 4, FLOOR) for g in GROUPS):
            print(f"model seed {model_seed}: own error above a quarter of the largest -> skipped")
            continue
        margins[model_seed] = pool_margin(model_seed, py_seed)
        gap, dist, ratio = margins[model_seed]
        print(f"model seed {model_seed}: minimum top-two gap {gap:.3e}, conv output fp32 <-> float64 {dist:.3e}, smallest gap / distance of a "
              f"window {ratio:.2f}")
        if ratio >= GAP_FACTOR:
            break
    else:
        # none of the 16 reaches the factor 8: the seed with the widest margin, which must still exceed 2 (both elements of a pair moving
        # against each other by the window's largest distance do not swap them: the fp32 run's own arg-max equals the exact one)
        if not margins:
            raise SystemExit("no model seed meets criterion (b)")
        model_seed = max(margins, key=lambda s: margins[s][2])
        gap, dist, ratio = margins[model_seed]
        if ratio <= 2.0:
            raise SystemExit("no model seed keeps every arg-max clear of rounding")
        print(f"no seed reaches {GAP_FACTOR}: taking the widest margin, model seed {model_seed} ({ratio:.2f})")
    out = {f"own_error/{s}/{g}": np.asarray(own[s][g]) for s in MODEL_SEEDS for g in GROUPS}
    out["pool_gap_min"], out["conv_out_dist_max"], out["pool_margin_min"] = np.asarray(gap), np.asarray(dist), np.asarray(ratio)
    cfg = dict(CFG, model_seed=model_seed, py_seed=py_seed)
    got = run(out, model_seed, py_seed)
    assert set(got["masks"][0]) == {0, 1, 2, 3}, got["masks"]
    for k, v in cfg.items():
        out[f"cfg/{k}"] = np.asarray(v)
    out["model_seeds"] = np.asarray(MODEL_SEEDS, dtype=np.int32)
    out["partitions"], out["patients"] = np.asarray(PARTITIONS), np.asarray(PATIENTS)
    save("contrast_decoder", **out)


if __name__ == "__main__":
    main()
