"""CPU side of the Dice supervised loss (``SupCriterion.name=dice|kldice``): the criterion classes against the
float64 expression and the wheel's own results (tests/golden/dice.npz), the closed form the kernel evaluates against autograd, the
library's new entry point, the class-count query, the configuration section, ``supervised_loss`` on the materialised path and the
tape signature."""
import os
import re

import numpy as np
import pytest
import torch

import dice_ref
import synth
import trainer_harness as th
from trainer_harness import PKG

NEW = ("miseg_softmax_dice", "miseg_softmax_dice_ws_bytes")
DISPATCH = (2, 3, 4, 5, 6, 8, 10, 16)


def _operands(shape, scale=2):
    z, lab = dice_ref.logits(shape, scale), dice_ref.labels(shape)
    onehot = torch.stack([lab == k for k in range(shape[1])], 1).long()
    return z, lab, onehot


# ---------------------------------------------------------------------------------------------------------------- the criterion classes
@pytest.mark.parametrize("pw", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", dice_ref.SHAPES)
def test_forward_equals_the_float64_expression(shape, weighted, pw):
    from deepclustering2.loss import GeneralizedDiceLoss
    z, lab, onehot = _operands(shape)
    weight = dice_ref.class_weights(shape[1]) if weighted else None
    p = z.double().softmax(1)
    dims = (2, 3)
    dices = 1 - (2 * (p * onehot).sum(dims) + 1e-8) / ((p.pow(pw) + onehot.double().pow(pw)).sum(dims) + 1e-8)
    if weighted:
        dices = torch.tensor(weight, dtype=torch.float64) * dices
    for reduction, ref in (("mean", dices.mean()), ("sum", dices.sum()), ("none", dices)):
        got = GeneralizedDiceLoss(pow=pw, weight=weight, reduction=reduction)(p, onehot)
        assert got.dtype == torch.float64 and got.shape == ref.shape
        torch.testing.assert_close(got, ref, rtol=1e-14, atol=0)
    # ... and dice_ref.reference, which the GPU tests use, is that expression
    assert abs(dice_ref.reference(z, lab, pw, 1e-8, weight)[0] - float(dices.mean())) <= 1e-14 * float(dices.mean())


def test_forward_asserts_and_disable_assert():
    from deepclustering2.loss import GeneralizedDiceLoss
    z, lab, onehot = _operands((2, 4, 5, 7))
    crit = GeneralizedDiceLoss()
    with pytest.raises(AssertionError):
        crit(z, onehot)                       # logits are no simplex
    with pytest.raises(AssertionError):
        crit(z.softmax(1), onehot * 2)        # no one-hot
    with pytest.raises(AssertionError):
        crit(z.softmax(1), onehot[:, :3])
    # the reference's EvalEpocher passes disable_assert=True to the supervised criterion: accepted and honoured
    got = crit(z, onehot, disable_assert=True)
    assert torch.isfinite(got)
    assert torch.equal(crit(z.softmax(1), onehot, disable_assert=True), crit(z.softmax(1), onehot))


def test_supports_fused_and_signature():
    from deepclustering2.loss import GeneralizedDiceLoss
    assert GeneralizedDiceLoss().supports_fused() and GeneralizedDiceLoss(pow=2, weight=[1.0, 2.0, 3.0, 4.0]).supports_fused(4)
    assert not GeneralizedDiceLoss(weight=[1.0, 2.0, 3.0]).supports_fused(4)
    assert not GeneralizedDiceLoss(reduction="sum").supports_fused() and not GeneralizedDiceLoss(reduction="none").supports_fused()
    assert not GeneralizedDiceLoss(pow=3).supports_fused()
    assert not GeneralizedDiceLoss(ignore_index=0).supports_fused()
    assert GeneralizedDiceLoss().signature() != GeneralizedDiceLoss(pow=2).signature()
    assert GeneralizedDiceLoss().signature() != GeneralizedDiceLoss(epsilon=1e-6).signature()
    assert GeneralizedDiceLoss().signature() != GeneralizedDiceLoss(weight=[1.0, 1.0]).signature()
    assert GeneralizedDiceLoss().signature() == GeneralizedDiceLoss().signature()
    assert list(GeneralizedDiceLoss(weight=[1.0, 2.0]).state_dict()) == []       # no weight / reduction entries


def test_metrics_are_the_wheels_expression():
    from deepclustering2.loss import MetaDice, dice_batch, dice_coef
    z, lab, onehot = _operands((3, 4, 33, 31))
    p = z.softmax(1)
    t = onehot.float()
    d2 = (2 * (p * t).sum((2, 3)) + 1e-8) / ((p + t).sum((2, 3)) + 1e-8)
    d3 = (2 * (p * t).sum((0, 2, 3)) + 1e-8) / ((p + t).sum((0, 2, 3)) + 1e-8)
    assert torch.equal(dice_coef(p, onehot), d2) and torch.equal(dice_batch(p, onehot), d3)
    assert torch.equal(MetaDice("2d", reduce=True)(p, onehot), d2.mean(0))
    with pytest.raises(AssertionError):
        MetaDice("4d")


def test_kldice_is_the_weighted_sum():
    from deepclustering2.loss import GeneralizedDiceLoss, KL_div
    from semi_seg._utils import KLDiceLoss
    z, lab, onehot = _operands((3, 4, 33, 31))
    p = z.double().softmax(1).requires_grad_()
    crit = KLDiceLoss(kl_weight=0.7, dice_weight=1.3, dice=GeneralizedDiceLoss(pow=2))
    ref = 0.7 * KL_div(verbose=False)(p, onehot) + 1.3 * GeneralizedDiceLoss(pow=2)(p, onehot)
    torch.testing.assert_close(crit(p, onehot), ref, rtol=1e-14, atol=0)
    assert crit.supports_fused(4) and not KLDiceLoss(dice=GeneralizedDiceLoss(pow=3)).supports_fused(4)
    assert crit.signature() != KLDiceLoss(kl_weight=0.7, dice_weight=1.0, dice=GeneralizedDiceLoss(pow=2)).signature()
    sd = crit.state_dict()
    other = KLDiceLoss()
    other.load_state_dict(sd)
    assert (other.kl_weight, other.dice_weight) == (0.7, 1.3)


# ---------------------------------------------------------------------------------------------------------------- the closed form
@pytest.mark.parametrize("pw", [1, 2])
@pytest.mark.parametrize("shape", dice_ref.SHAPES)
def test_closed_form_equals_float64_autograd(shape, pw):
    """What the kernel evaluates (coefficients a, b and the softmax Jacobian) against autograd through the wheel's expression, with
    class weights, a KL part and a few pixels taken out as the kernel takes out a bad label."""
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape)
    bad = torch.zeros(lab.shape, dtype=torch.bool)
    bad[1, 2, :3] = True
    for kw in (dict(), dict(weight=dice_ref.class_weights(shape[1])), dict(kl_weight=0.7, dice_weight=1.3), dict(bad=bad, kl_weight=0.5)):
        ref_loss, ref_grad = dice_ref.reference(z, lab, pw, 1e-8, **kw)
        loss, grad = dice_ref.closed_form(z, lab, pw, 1e-8, **kw)
        assert abs(loss - ref_loss) <= 1e-13 * abs(ref_loss), (kw, loss, ref_loss)
        assert float((grad - ref_grad).abs().max()) <= 1e-13 * float(ref_grad.abs().max()), kw
        if "bad" in kw:
            assert float(grad[1, :, 2, :3].abs().max()) == 0.0 and float(ref_grad[1, :, 2, :3].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- the wheel's own results
@pytest.mark.parametrize("si", range(len(dice_ref.SHAPES)))
def test_forward_and_gradient_match_the_wheels_class(golden, si):
    """tests/golden/dice.npz: the wheel's GeneralizedDiceLoss in float64 on the same inputs (make_golden_dice.py)."""
    from deepclustering2.loss import GeneralizedDiceLoss
    g = golden("dice")
    shape = dice_ref.SHAPES[si]
    z, lab, onehot = _operands(shape)
    for pw in (1, 2):
        for weighted in (0, 1):
            key = f"crit/s{si}_p{pw}_w{weighted}"
            weight = dice_ref.class_weights(shape[1]) if weighted else None
            z64 = z.double().requires_grad_()
            loss = GeneralizedDiceLoss(pow=pw, weight=weight)(z64.softmax(1), onehot)
            loss.backward()
            np.testing.assert_allclose(float(loss.detach()), float(g[key + "/loss"]), rtol=1e-13)
            fp = synth.fp_unpack(g, key + "/grad")
            scale = float(np.abs(fp["sample"]).max())
            synth.check_fingerprint(z64.grad.numpy(), fp, key + "/grad", rtol=1e-11, atol=1e-13 * scale)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    header, _ = th.assert_entry_points(NEW)
    assert re.search(r"\bint\s+miseg_softmax_dice\s*\(", header) and re.search(r"\bint64_t\s+miseg_softmax_dice_ws_bytes\s*\(", header)
    # stream, logits, labels, N, H, W, C, pow, eps, class_weight, kl_weight, dice_weight, upstream, loss, glogits, bad_label, ws, ws_bytes
    assert len(_cabi.PROTOTYPES["miseg_softmax_dice"][1]) == 18 and len(_cabi.PROTOTYPES["miseg_softmax_dice_ws_bytes"][1]) == 4
    assert _cabi.lib().miseg_version() >= 416


def test_refusals_need_no_gpu():
    """Bad arguments are refused before any launch."""
    from miseg_amd import _cabi
    lib = _cabi.lib()
    ws = lib.miseg_softmax_dice_ws_bytes
    assert ws(16, 256, 256, 4) > 0 and ws(0, 8, 8, 4) < 0 and ws(1, 0, 8, 4) < 0 and ws(1, 8, 8, 0) < 0
    assert ws(2, 64, 64, 4) < ws(2, 256, 256, 4) == ws(2, 512, 512, 4)          # the blocks per sample are capped
    assert lib.miseg_softmax_dice(None, None, None, 1, 8, 8, 4, 1, 1e-8, None, 0.0, 1.0, None, None, None, None, None, 0) < 0
    assert b"softmax_dice" in lib.miseg_last_error()


def test_supported_class_counts_mirror_the_dispatch_list():
    from miseg_amd import ops
    assert [c for c in range(0, 40) if ops.softmax_dice_supported(c)] == list(DISPATCH)
    # ... the list of the one switch of the pixel-loss units, which every variant of the Dice launches goes through
    src = open(os.path.join(PKG, "csrc", "dice.hip")).read()
    variant = src[src.index("#define MISEG_DICE_VARIANT"):src.index('extern "C" int miseg_softmax_dice(')]
    assert variant.count("MISEG_DISPATCH_C(C, MACRO, ") == 4 and "switch" not in src
    shared = open(os.path.join(PKG, "csrc", "pixel_loss.h")).read()
    macro = shared[shared.index("#define MISEG_DISPATCH_C"):]
    macro = macro[:macro.index("default:")]
    assert tuple(int(m) for m in re.findall(r"case (\d+):", macro)) == DISPATCH


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_no_section_and_name_kl_yield_a_plain_kl_div():
    import yaml
    from deepclustering2.loss import KL_div
    from semi_seg._utils import build_sup_criterion
    shipped = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert "SupCriterion" not in shipped and "SupCriterion" not in th.semi_config()
    for cfg in (th.semi_config(), th.semi_config(["SupCriterion.name=kl"]), {}, None):
        crit = build_sup_criterion(cfg, 4)
        assert type(crit) is KL_div and crit.supports_fused() and not hasattr(crit, "signature")


def test_cli_overrides_reach_the_criterion():
    from deepclustering2.loss import GeneralizedDiceLoss
    from semi_seg._utils import KLDiceLoss, build_sup_criterion
    crit = build_sup_criterion(th.semi_config(["SupCriterion.name=dice", "SupCriterion.pow=2", "SupCriterion.epsilon=1e-6"]), 4)
    assert type(crit) is GeneralizedDiceLoss and (crit.pow, crit.epsilon, crit.weight, crit.reduction) == (2, 1e-6, None, "mean")
    crit = build_sup_criterion(th.semi_config(["SupCriterion.name=kldice", "SupCriterion.kl_weight=0.7", "SupCriterion.dice_weight=1.3"]), 4)
    assert type(crit) is KLDiceLoss and (crit.kl_weight, crit.dice_weight, crit._dice.pow, crit._dice.epsilon) == (0.7, 1.3, 1, 1e-8)
    crit = build_sup_criterion({"SupCriterion": {"name": "dice", "class_weight": [1, 2, 3, 4]}}, 4)
    assert crit.weight == [1.0, 2.0, 3.0, 4.0] and crit.supports_fused(4)


def test_unknown_key_or_name_raises():
    from semi_seg._utils import build_sup_criterion
    with pytest.raises(KeyError, match="unknown keys"):
        build_sup_criterion(th.semi_config(["SupCriterion.name=dice", "SupCriterion.power=2"]), 4)
    with pytest.raises(KeyError, match="tversky"):
        build_sup_criterion(th.semi_config(["SupCriterion.name=tversky"]), 4)
    with pytest.raises(ValueError):
        build_sup_criterion({"SupCriterion": {"name": "dice", "class_weight": [1, 2, 3]}}, 4)


def test_main_builds_the_trainer_with_the_configured_criterion(tmp_path):
    from deepclustering2.loss import KL_div
    from semi_seg._utils import KLDiceLoss
    from semi_seg.main import build_trainer
    common = ["Trainer.name=partial", "Data.name=synthetic", "Trainer.device=cpu", "Data.size=32", "LabeledData.batch_size=2",
              "UnlabeledData.batch_size=2"]
    tr = build_trainer(common + [f"Trainer.save_dir={tmp_path}/a", "SupCriterion.name=kldice", "SupCriterion.dice_weight=2.0"])
    assert type(tr._sup_criterion) is KLDiceLoss and tr._sup_criterion.dice_weight == 2.0
    assert type(build_trainer(common + [f"Trainer.save_dir={tmp_path}/b"])._sup_criterion) is KL_div


# ---------------------------------------------------------------------------------------------------------------- the epocher's seams
@pytest.mark.parametrize("pw", [1, 2])
def test_supervised_loss_on_cpu_tensors_takes_the_materialised_path(pw):
    from deepclustering2.loss import GeneralizedDiceLoss
    from semi_seg._utils import KLDiceLoss
    from semi_seg.epocher import supervised_loss
    shape = (3, 4, 33, 31)
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape)
    weight = dice_ref.class_weights(4)
    for crit, kw in ((GeneralizedDiceLoss(pow=pw, weight=weight), dict(weight=weight)),
                     (KLDiceLoss(0.7, 1.3, GeneralizedDiceLoss(pow=pw)), dict(kl_weight=0.7, dice_weight=1.3))):
        ref_loss, ref_grad = dice_ref.reference(z, lab, pw, 1e-8, **kw)
        z64 = z.double().requires_grad_()
        loss = supervised_loss(crit, z64, lab, 4)
        loss.backward()
        assert abs(float(loss) - ref_loss) <= 1e-13 * abs(ref_loss)
        assert float((z64.grad - ref_grad).abs().max()) <= 1e-13 * float(ref_grad.abs().max())
        with torch.no_grad():         # the evaluation's call
            assert abs(float(supervised_loss(crit, z.double(), lab, 4, disable_assert=True)) - ref_loss) <= 1e-13 * abs(ref_loss)


def test_tape_signature_carries_the_criterions_constants():
    from deepclustering2.loss import GeneralizedDiceLoss, KL_div
    from semi_seg._utils import KLDiceLoss
    from semi_seg.epocher import TrainEpocher
    sig = TrainEpocher._criterion_signature
    assert sig(KL_div(verbose=False)) == "KL_div"          # what the signature tuple has always held for it
    assert sig(KLDiceLoss(dice_weight=1.0)) != sig(KLDiceLoss(dice_weight=2.0))
    assert sig(GeneralizedDiceLoss()) != sig(GeneralizedDiceLoss(pow=2)) and sig(GeneralizedDiceLoss())[0] == "GeneralizedDiceLoss"

    class _Opt:
        pass

    def full(crit):
        ep = TrainEpocher.__new__(TrainEpocher)
        ep._optimizer, ep._model, ep._sup_criterion, ep._reg_weight = _Opt(), torch.nn.Linear(1, 1), crit, 0.0
        ep._feature_importance, ep._feature_position = [1.0], ["Conv5"]
        return ep._tape_signature()

    kl = full(KL_div(verbose=False))
    assert "KL_div" in kl and kl[6] == "KL_div"
    a, b = full(KLDiceLoss(dice_weight=1.0)), full(KLDiceLoss(dice_weight=2.0))
    assert a[:6] == b[:6] and a[6] != b[6]
