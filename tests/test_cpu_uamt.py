"""CPU side of the uncertainty-aware Mean Teacher (``Trainer.name=uamt``): the float64 restatement of its
device work (tests/uamt_ref.py) -- its two gradients against each other and against finite differences, its limits (every pixel
certain: pixel_ref's plain MSE; none: zero), the threshold ramp -- the condition under which the kernel tests may compare masks
pixel by pixel (a half-gap of at least 1e-4 around every case's threshold, a tenth of the pixels on each side), registration and the
``UAMTParameters`` section, the host words and rows, the meter names, the library's new entry points, and config/semi.yaml -- which
documents the section as a comment and must parse as before."""
import math
import os
import types

import numpy as np
import pytest
import torch

import pixel_ref as P
import trainer_harness as th
import uamt_ref as R
from test_cpu_ict import SEMI_YAML
from trainer_harness import PKG

NEW = ("miseg_noise_add", "miseg_softmax_accum", "miseg_softmax_umse")
SHAPE = (3, 4, 5, 7)           # N, C, H, W
DEFAULTS = dict(name="mse", weight=0.1, alpha=0.99, weight_decay=0.000001, passes=8, noise_sigma=0.1, noise_clip=0.2, threshold_start=0.75,
                threshold_end=1.0)


def _inputs(scale=2.0):
    n, c, h, w = SHAPE
    a, b = P.logits("uamt/cpu/a", n, c, h, w, scale), P.logits("uamt/cpu/b", n, c, h, w, scale)
    acc = R.accumulate([P.logits(f"uamt/cpu/pass{p}", n, c, h, w, scale) for p in range(R.PASSES)])
    return a, b, acc


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_the_two_gradients_of_the_reference_agree():
    a, b, acc = _inputs()
    thr, half = R.gap_threshold(R.uncertainty(acc, R.PASSES))
    loss, grad, hand, k, mask, unc = R.umse_value_and_grad(a, b, acc, R.PASSES, thr)
    assert 0 < k < mask.numel() and k == int((unc < thr).sum()) and half > 0
    assert float((grad - hand).abs().max()) <= 1e-12
    assert float(loss) > 0 and bool((grad[~mask.unsqueeze(1).expand_as(grad)] == 0).all())


def test_hand_gradient_equals_central_differences():
    """Central differences with h = 1e-6 in float64 at 24 seeded entries: truncation ~h^2, cancellation ~1e-16 / h, so 1e-7 of the
    largest gradient entry leaves two orders of room."""
    a, b, acc = _inputs()
    thr, _ = R.gap_threshold(R.uncertainty(acc, R.PASSES))
    _, _, hand, _, mask, _ = R.umse_value_and_grad(a, b, acc, R.PASSES, thr)
    a64, b64 = a.to(R.F64), b.to(R.F64)
    h = 1e-6
    for flat in np.random.RandomState(5).choice(a64.numel(), 24, replace=False):
        idx = np.unravel_index(int(flat), a64.shape)
        up, dn = a64.clone(), a64.clone()
        up[idx] += h
        dn[idx] -= h
        fd = (float(R.umse_expr(up, b64, mask)) - float(R.umse_expr(dn, b64, mask))) / (2 * h)
        assert abs(fd - float(hand[idx])) <= 1e-7 * float(hand.abs().max()), (idx, fd, float(hand[idx]))


def test_all_certain_is_the_plain_mse_and_none_certain_is_zero():
    a, b, acc = _inputs()
    c = SHAPE[1]
    loss, grad, hand, k, mask, _ = R.umse_value_and_grad(a, b, acc, R.PASSES, 2.0 * math.log(c))
    want = P.mse_expr(a.to(R.F64), b.to(R.F64))
    want_loss, want_grad = P.value_and_grad("mse", a, b)
    assert k == mask.numel() and bool(mask.all())
    assert abs(float(loss) - float(want)) <= 1e-14 * float(want) and abs(float(loss) - float(want_loss)) <= 1e-14 * float(want)
    assert float((grad - want_grad).abs().max()) <= 1e-13 * float(want_grad.abs().max())
    assert float((hand - want_grad).abs().max()) <= 1e-13 * float(want_grad.abs().max())
    loss, grad, hand, k, mask, _ = R.umse_value_and_grad(a, b, acc, R.PASSES, 0.0)
    assert k == 0 and float(loss) == 0.0 and not bool(grad.any()) and not bool(hand.any())
    assert math.isfinite(float(loss)) and bool(torch.isfinite(hand).all())


def test_uncertainty_of_the_extremes_and_the_noise():
    onehot = torch.zeros(1, 4, 1, 2, dtype=R.F64)
    onehot[:, 0] = 3.0                                         # three passes, all sure of class 0
    uniform = torch.full((1, 4, 1, 2), 0.75, dtype=R.F64)      # three passes, all uniform
    assert float(R.uncertainty(onehot, 3).abs().max()) < 2e-6
    assert float((R.uncertainty(uniform, 3) - math.log(4)).abs().max()) < 1e-5
    x, z = torch.tensor([0.0, 1.0, -1.0, 2.0], dtype=R.F64), torch.tensor([0.5, 5.0, -5.0, 0.0], dtype=R.F64)
    assert R.noise(x, z, 0.1, 0.2).tolist() == [0.05, 1.2, -1.2, 2.0]
    assert torch.equal(R.noise(x, z, 0.0, 0.2), x)
    two = R.accumulate([torch.zeros(1, 2, 1, 1), torch.zeros(1, 2, 1, 1)])
    assert two.flatten().tolist() == [1.0, 1.0]


def test_gap_threshold_picks_the_widest_admissible_gap():
    u = torch.tensor([0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.45, 0.5, 0.9, 1.0], dtype=R.F64)
    thr, half = R.gap_threshold(u, lo_share=0.2)          # the 0.5 | 0.9 gap leaves 2 of 10 above: admissible
    assert abs(thr - 0.7) < 1e-12 and abs(half - 0.2) < 1e-12
    thr, half = R.gap_threshold(u, lo_share=0.3)          # now it is not; the widest of the rest is 0.1 wide (the first of them)
    assert abs(half - 0.05) < 1e-12 and 3 <= int((u < thr).sum()) <= 7


# ---------------------------------------------------------------------------------------------------------------- the ramp
def test_threshold_ramp_end_points_monotone_and_the_two_class_form():
    from semi_seg.epocher import uamt_threshold
    for c in (2, 4, 16):
        assert abs(uamt_threshold(0, 100, 0.75, 1.0, c) - (0.75 + 0.25 * math.exp(-5.0)) * math.log(c)) < 1e-15
        assert uamt_threshold(100, 100, 0.75, 1.0, c) == math.log(c) == uamt_threshold(250, 100, 0.75, 1.0, c)
        values = [uamt_threshold(k, 100, 0.75, 1.0, c) for k in range(0, 130)]
        assert all(y >= x for x, y in zip(values, values[1:])) and values[0] < values[100]
        for k in (0, 1, 37, 99, 100, 140):
            assert uamt_threshold(k, 100, 0.75, 1.0, c) == R.threshold(k, 100, 0.75, 1.0, c)
    for k in (0, 13, 50, 100):
        r = min(k / 100, 1.0)
        assert abs(uamt_threshold(k, 100, 0.75, 1.0, 2) - (0.75 + 0.25 * math.exp(-5 * (1 - r) ** 2)) * math.log(2)) < 1e-15
    assert uamt_threshold(3, 100, 0.5, 0.5, 4) == 0.5 * math.log(4)


# ---------------------------------------------------------------------------------------------------------------- the kernel tests' cases
@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_every_kernel_case_has_a_clear_threshold(name):
    """A half-gap of at least 1e-4 -- two orders above the fp32 error of an entropy of a few units -- and at least a tenth of the
    pixels on each side, on the uncertainties of the accumulator as the kernel reads it (rounded to float32)."""
    thr, half = R.case_threshold(name)
    unc = R.uncertainty(R.case_acc(name).float(), R.PASSES)
    below = int((unc < thr).sum())
    print(f"\nUAMT case {name}: thr {thr:.6f}, half-gap {half:.3e}, {below} of {unc.numel()} pixels certain")
    assert half >= R.MIN_HALF_GAP
    assert below >= 0.1 * unc.numel() and unc.numel() - below >= 0.1 * unc.numel()
    assert float((unc - thr).abs().min()) >= half - thr * 2.0 ** -23         # (thr itself was rounded to float32: an ulp of room)
    n, h, w, c, _ = P.LOSS_CASES[name]
    assert tuple(R.case_acc(name).shape) == (n, c, h, w) and tuple(R.pass_logits(name, 0).shape) == (n, c, h, w)


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_zoo_has_uamt_on_the_mean_teacher():
    from semi_seg import epocher as E
    from semi_seg.trainer import MeanTeacherTrainer, UAMTTrainer, trainer_zoos
    assert trainer_zoos["uamt"] is UAMTTrainer and issubclass(UAMTTrainer, MeanTeacherTrainer) and UAMTTrainer.NAME == "uamt"
    assert issubclass(E.UAMTEpocher, E.MeanTeacherEpocher)
    assert UAMTTrainer._inference_model is MeanTeacherTrainer._inference_model
    assert UAMTTrainer.SINGLE_PROCESS == "the count of certain pixels would have to be all-reduced before the gradient is scaled"
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin", "vat", "ict", "contrast", "contrastdecoder"} <= set(trainer_zoos)
    assert E.MeanTeacherEpocher._TRAIN_FORWARDS == 2 and E.ICTEpocher._TRAIN_FORWARDS == 2      # per instance: the class value stays


def test_parameters_defaults_overrides_and_every_error():
    from semi_seg.trainer import UAMTTrainer
    par = UAMTTrainer.parameters
    assert par({}) == DEFAULTS and par(None) == DEFAULTS and par({"UAMTParameters": None}) == DEFAULTS
    got = par({"UAMTParameters": {"passes": "4", "noise_sigma": 0, "weight": 3, "threshold_start": 0.5, "threshold_end": 0.5}})
    assert got == dict(DEFAULTS, passes=4, noise_sigma=0.0, weight=3.0, threshold_start=0.5, threshold_end=0.5)
    assert isinstance(got["weight"], float) and isinstance(got["passes"], int)
    assert par({"UAMTParameters": {"passes": 1}})["passes"] == 1 and par({"UAMTParameters": {"passes": 32}})["passes"] == 32
    for bad in ({"pases": 4}, {"mix_alpha": 1.0}, {"name": "kl"}, {"name": "l1"}):
        with pytest.raises(KeyError):
            par({"UAMTParameters": bad})
    for bad in ({"passes": 0}, {"passes": 33}, {"passes": -1}, {"noise_sigma": -0.1}, {"noise_clip": -1e-3}, {"threshold_start": 1.1},
                {"threshold_start": 0.8, "threshold_end": 0.7}, {"threshold_start": -0.1}, {"threshold_start": -0.2, "threshold_end": -0.1}):
        with pytest.raises(ValueError):
            par({"UAMTParameters": bad})


def test_trainer_init_reads_the_optional_section_and_hands_k_total_over():
    from semi_seg import epocher as E
    cfg = th.semi_config()
    assert "UAMTParameters" not in cfg
    tr = th.bare_trainer("uamt", cfg)
    assert isinstance(tr._reg_criterion, torch.nn.MSELoss) and tr._reg_weight == 0.1
    assert tr._ema_updater._alpha == 0.99 and tr._ema_updater._weight_decay == 1e-6
    assert tr._teacher_model is not tr._model and all(not p.requires_grad for p in tr._teacher_model.parameters())
    tr = th.bare_trainer("uamt", th.semi_config(["UAMTParameters.passes=2", "UAMTParameters.noise_sigma=0.05", "UAMTParameters.alpha=0.999"]))
    tr._feature_importance, tr.feature_positions = [1.0], ["Conv5"]
    tr._max_epoch, tr._num_batches, tr._cur_epoch = 7, 5, 3
    ep = tr._make_epocher()
    assert type(ep) is E.UAMTEpocher and ep._teacher_model is tr._teacher_model and tr._ema_updater._alpha == 0.999
    assert (ep._passes, ep._noise_sigma, ep._noise_clip, ep._threshold, ep._k_total) == (2, 0.05, 0.2, (0.75, 1.0), 35)
    assert ep._TRAIN_FORWARDS == 4 and E.UAMTEpocher._TRAIN_FORWARDS == 2
    # a function of cur_epoch and i only: a resumed run lands on the same threshold
    assert ep.threshold_at(2) == R.threshold(3 * 5 + 2, 35, 0.75, 1.0, 4)
    for bad, err in ((["UAMTParameters.passes=0"], ValueError), (["UAMTParameters.name=kl"], KeyError), (["UAMTParameters.sigma=2"], KeyError),
                     (["UAMTParameters.noise_clip=-1"], ValueError), (["UAMTParameters.threshold_start=2"], ValueError)):
        with pytest.raises(err):
            th.bare_trainer("uamt", th.semi_config(bad))


# ---------------------------------------------------------------------------------------------------------------- host words, rows
def _bare_epocher(cur_epoch=0, num_batches=4, k_total=8):
    from deepclustering2.models import ema_updater
    from semi_seg import epocher as E
    ep = object.__new__(E.UAMTEpocher)
    ep._model = types.SimpleNamespace(num_classes=4)
    ep._passes, ep._noise_sigma, ep._noise_clip, ep._threshold, ep._k_total = 2, 0.1, 0.2, (0.75, 1.0), k_total
    ep._cur_epoch, ep._num_batches, ep._iteration, ep._thr, ep._thr_sent = cur_epoch, num_batches, 0, 0.0, []
    ep._ema_updater = ema_updater(alpha=0.999, justify_alpha=True, weight_decay=1e-6)
    return ep


def test_words_are_zero_flips_then_the_two_halves_of_the_seed():
    ep = _bare_epocher()
    assert ep._draw_words(1234567, 3) == [0, 0, 0, 1234567, 0]
    assert ep._draw_words(0, 1) == [0, 0, 0]
    words = ep._draw_words((5 << 32) | 0x80000001, 2)            # a high word, and a low word with its top bit set: int32 patterns
    assert words == [0, 0, 0x80000001 - (1 << 32), 5] and all(type(w) is int and -2 ** 31 <= w < 2 ** 31 for w in words)
    lo, hi = (w & 0xFFFFFFFF for w in words[2:])
    assert (hi << 32) | lo == (5 << 32) | 0x80000001


def test_threshold_row_is_staged_behind_the_ema_row_and_follows_the_iteration():
    from semi_seg import epocher as E
    ep = _bare_epocher(cur_epoch=1, num_batches=4, k_total=8)
    seen = []
    for i in range(5):
        ep._draw_words(11 + i, 3)
        rows = ep._own_rows()
        assert len(rows) == 2 and len(rows[0]) == 4 and len(rows[1]) == 1
        seen.append(rows[1][0])
    assert seen == [R.threshold(4 + i, 8, 0.75, 1.0, 4) for i in range(5)] == ep._thr_sent
    assert seen[-1] == math.log(4) and seen[0] < seen[1] < seen[2] < seen[3]
    again = _bare_epocher(cur_epoch=1, num_batches=4, k_total=8)       # the resumed run's epocher
    again._draw_words(99, 3)
    assert again._own_rows()[1] == [seen[0]]
    assert E.UAMTEpocher._tape_signature is not E.MeanTeacherEpocher._tape_signature


def test_meters_sit_beside_the_mean_teachers():
    from deepclustering2.meters2 import MeterInterface
    from semi_seg import epocher as E
    ep = object.__new__(E.UAMTEpocher)
    ep._model = types.SimpleNamespace(num_classes=4)
    names = ep._configure_meters(MeterInterface()).meter_names
    assert names == ["lr", "sup_loss", "reg_loss", "sup_dice", "reg_weight", "uncertainty", "certain", "threshold"]


def test_images_that_are_not_fp32_4d_device_tensors_raise_type_error():
    ep = _bare_epocher()
    flips = torch.zeros(3, dtype=torch.int32)
    for lab, unl in ((torch.rand(2, 1, 4, 5, dtype=torch.float64), torch.rand(3, 1, 4, 5, dtype=torch.float64)),
                     (torch.rand(2, 1, 4, 5).half(), torch.rand(3, 1, 4, 5).half()), (torch.rand(2, 4, 5), torch.rand(3, 4, 5)),
                     (torch.rand(2, 1, 4, 5), torch.rand(3, 1, 4, 5))):          # (the last: fp32 4-D, but not on the GPU)
        with pytest.raises(TypeError, match="uamt"):
            ep._student_batch(lab, unl, flips)


# ---------------------------------------------------------------------------------------------------------------- the library, the config
def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    import test_cpu_tape_table as TABLE
    header, _ = th.assert_entry_points(NEW + ("miseg_softmax_umse_ws_bytes",))
    assert _cabi.lib().miseg_version() >= 418
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "uamt.hip" in makefile and "uamt.o" in makefile.split("-ffp-contract=off")[0]
    for name in NEW:
        ep = TABLE.EPS[name]
        assert ep.file == "uamt.hip" and TABLE.macro_args(ep)[1:] == ep.params
        assert len(_cabi.PROTOTYPES[name][1]) == len(ep.params)
    assert TABLE.EPS["miseg_noise_add"].params == ["stream", "x", "M", "passes", "seed", "sigma", "clip", "out"]
    assert TABLE.EPS["miseg_softmax_accum"].params == ["stream", "logits", "N", "H", "W", "C", "first", "acc"]
    assert TABLE.EPS["miseg_softmax_umse"].params == ["stream", "a", "b", "acc", "N", "H", "W", "C", "inv_passes", "thr", "upstream", "loss", "ga",
                                                      "kept", "stats", "ws", "ws_bytes"]
    # the generator is one header for both units
    csrc = os.path.join(PKG, "csrc")
    assert '#include "philox.h"' in open(os.path.join(csrc, "vat.hip")).read() and '#include "philox.h"' in open(os.path.join(csrc, "uamt.hip")).read()
    assert "philox4x32_10" not in open(os.path.join(csrc, "vat.hip")).read()
    # the workspace: three partials per block of 256 pixels (at most 2048 blocks) and the gradient's scale
    assert _cabi.query("miseg_softmax_umse_ws_bytes", 3, 19, 23) == 16 * P.loss_blocks(3 * 19 * 23) + 16
    assert _cabi.query("miseg_softmax_umse_ws_bytes", 2, 512, 513) == 16 * P.LOSS_MAX_BLOCKS + 16


def test_ops_offers_the_wrappers_in_their_families():
    from miseg_amd import ops
    from miseg_amd.lazy import LinearLoss
    from miseg_amd.ops import batch, losses
    assert ops.noise_add is batch.noise_add
    assert ops.softmax_accum is losses.softmax_accum and ops.softmax_umse is losses.softmax_umse
    assert issubclass(losses._SoftmaxUMSE, losses._ScaledGradLoss) and callable(LinearLoss.of)


def test_semi_yaml_parses_to_the_same_dictionary_and_documents_the_section():
    import yaml
    path = os.path.join(PKG, "config", "semi.yaml")
    assert yaml.safe_load(open(path)) == SEMI_YAML
    text = open(path).read()
    assert "#UAMTParameters:" in text and "#ICTParameters:" in text
    for key, value in DEFAULTS.items():
        shown = {"weight_decay": "0.000001"}.get(key, str(value))
        assert f"#  {key}: {shown}" in text, key
