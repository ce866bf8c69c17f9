"""CPU side of the ICT trainer (``Trainer.name=ict``): the float64 restatement of its kernels (tests/ict_ref.py)
against autograd and finite differences, registration and the ``ICTParameters`` section, the host draws, the staged rows, the meter
names, the library's new entry points, and config/semi.yaml -- which documents the section as a comment and must parse as before."""
import os
import random
import types

import numpy as np
import pytest
import torch

import ict_ref as R
import pixel_ref as P
import trainer_harness as th
from trainer_harness import PKG

NEW = ("miseg_cat_mixed", "miseg_softmax_mix_mse", "miseg_softmax_mix_klcons")
SHAPE = (3, 4, 5, 7)           # N, C, H, W
PERM = [1, 2, 0]


def _ab(scale=2.0):
    n, c, h, w = SHAPE
    return P.logits("ict/cpu/a", n, c, h, w, scale), P.logits("ict/cpu/b", n, c, h, w, scale)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kernel", ["mse", "klcons"])
@pytest.mark.parametrize("lam", [0.3, 0.0, 1.0])
def test_hand_gradient_equals_float64_autograd(kernel, lam):
    a, b = _ab()
    c0, c1 = R.coefficients(lam)
    loss, grad = R.loss_and_grad(kernel, a, b, PERM, c0, c1)
    loss_ag, grad_ag = R.autograd_loss_and_grad(kernel, a, b, PERM, c0, c1)
    assert abs(float(loss) - float(loss_ag)) <= 1e-14 * abs(float(loss_ag))
    assert float((grad - grad_ag).abs().max()) <= 1e-13 * float(grad_ag.abs().max())


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
def test_hand_gradient_equals_central_differences(kernel):
    """Central differences with h = 1e-6 in float64 at 24 seeded entries: truncation ~h^2, cancellation ~1e-16 / h, so 1e-7 of the
    largest gradient entry leaves two orders of room."""
    a, b = _ab()
    c0, c1 = R.coefficients(0.3)
    _, grad = R.loss_and_grad(kernel, a, b, PERM, c0, c1)
    a64 = a.to(R.F64)
    rs = np.random.RandomState(5)
    h = 1e-6
    for flat in rs.choice(a64.numel(), 24, replace=False):
        idx = np.unravel_index(int(flat), a64.shape)
        up, dn = a64.clone(), a64.clone()
        up[idx] += h
        dn[idx] -= h
        fd = (float(R.EXPR[kernel](up, b.to(R.F64), PERM, c0, c1)) - float(R.EXPR[kernel](dn, b.to(R.F64), PERM, c0, c1))) / (2 * h)
        assert abs(fd - float(grad[idx])) <= 1e-7 * float(grad.abs().max()), (idx, fd, float(grad[idx]))


@pytest.mark.parametrize("kernel", ["mse", "klcons"])
def test_without_a_partner_it_is_the_plain_consistency_reference(kernel):
    """c0 = 1, identity permutation: pixel_ref's softmax_mse / softmax_klcons reference; so is any permutation at lam = 1."""
    a, b = _ab()
    want_loss, want_grad = P.value_and_grad(kernel, a, b)
    for perm, lam in (([0, 1, 2], 1.0), (PERM, 1.0)):
        c0, c1 = R.coefficients(lam)
        assert (c0, c1) == (1.0, 0.0)
        loss, grad = R.loss_and_grad(kernel, a, b, perm, c0, c1)
        assert abs(float(loss) - float(want_loss)) <= 1e-14 * abs(float(want_loss))
        assert float((grad - want_grad).abs().max()) <= 1e-13 * float(want_grad.abs().max())


def test_the_mix_is_a_gather_and_bad_indices_count_as_their_own():
    b = torch.arange(3.0).view(3, 1, 1, 1)
    assert R.mix_rows(b, [1, 2, 0], 0.0, 1.0).flatten().tolist() == [1.0, 2.0, 0.0]        # row i reads row perm[i]
    assert R.clean_perm([0, 7, -1], 3) == ([0, 1, 2], 2)
    assert torch.equal(R.cat_mixed(b, b, [0, 7, -1], 0.25, 0.75), torch.cat([b, b]).to(R.F64))
    assert R.coefficients(0.3) == (float(np.float32(0.3)), float(np.float32(0.7)))


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_zoo_has_ict_on_the_mean_teacher():
    from semi_seg import epocher as E
    from semi_seg.trainer import ICTTrainer, MeanTeacherTrainer, trainer_zoos
    assert trainer_zoos["ict"] is ICTTrainer and issubclass(ICTTrainer, MeanTeacherTrainer)
    assert issubclass(E.ICTEpocher, E.MeanTeacherEpocher) and E.ICTEpocher._TRAIN_FORWARDS == 2
    assert ICTTrainer._inference_model is MeanTeacherTrainer._inference_model
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin", "vat", "contrast", "contrastdecoder"} <= set(trainer_zoos)


def test_parameters_defaults_unknown_keys_and_mix_alpha():
    from semi_seg.trainer import ICTTrainer
    defaults = dict(name="mse", weight=10.0, alpha=0.999, weight_decay=0.000001, mix_alpha=1.0)
    assert ICTTrainer.parameters({}) == defaults and ICTTrainer.parameters(None) == defaults
    assert ICTTrainer.parameters({"ICTParameters": None}) == defaults
    got = ICTTrainer.parameters({"ICTParameters": {"name": "kl", "mix_alpha": "0.5", "weight": 3}})
    assert got == dict(defaults, name="kl", mix_alpha=0.5, weight=3.0) and isinstance(got["weight"], float)
    with pytest.raises(KeyError):
        ICTTrainer.parameters({"ICTParameters": {"mixalpha": 1.0}})
    with pytest.raises(KeyError):
        ICTTrainer.parameters({"ICTParameters": {"name": "l1"}})
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError):
            ICTTrainer.parameters({"ICTParameters": {"mix_alpha": bad}})


def test_trainer_init_reads_the_optional_section():
    from deepclustering2.loss import KL_div
    from semi_seg import epocher as E
    cfg = th.semi_config()
    assert "ICTParameters" not in cfg
    tr = th.bare_trainer("ict", cfg)
    assert isinstance(tr._reg_criterion, torch.nn.MSELoss) and tr._reg_weight == 10.0 and tr._mix_alpha == 1.0
    assert tr._ema_updater._alpha == 0.999 and tr._ema_updater._weight_decay == 1e-6
    assert tr._teacher_model is not tr._model and all(not p.requires_grad for p in tr._teacher_model.parameters())
    tr = th.bare_trainer("ict", th.semi_config(["ICTParameters.name=kl", "ICTParameters.mix_alpha=0.5", "ICTParameters.alpha=0.99"]))
    assert isinstance(tr._reg_criterion, KL_div) and tr._mix_alpha == 0.5 and tr._ema_updater._alpha == 0.99
    tr._feature_importance, tr.feature_positions = [1.0], ["Conv5"]
    ep = tr._make_epocher()
    assert type(ep) is E.ICTEpocher and ep._mix_alpha == 0.5 and ep._teacher_model is tr._teacher_model
    with pytest.raises(ValueError):
        th.bare_trainer("ict", th.semi_config(["ICTParameters.mix_alpha=0"]))
    with pytest.raises(KeyError):
        th.bare_trainer("ict", th.semi_config(["ICTParameters.beta=2"]))


# ---------------------------------------------------------------------------------------------------------------- host draws, rows
def _bare_epocher(name="ICTEpocher", mix_alpha=0.5):
    from deepclustering2.augment.tensor_augment import TensorRandomFlip
    from deepclustering2.models import ema_updater
    from semi_seg import epocher as E
    ep = object.__new__(getattr(E, name))
    ep._mix_alpha, ep._mix = mix_alpha, (1.0, 0.0)
    ep._affine_transformer = TensorRandomFlip(axis=[1, 2], threshold=0.8)
    ep._ema_updater = ema_updater(alpha=0.999, justify_alpha=True, weight_decay=1e-6)
    return ep


def test_draws_are_reproducible_in_the_stated_order_and_leave_the_generators_alone():
    ep = _bare_epocher()
    random.seed(3)
    np.random.seed(4)
    py_state, np_state = random.getstate(), np.random.get_state()
    for seed, ub in ((11, 3), (11, 3), (4242, 10), (0, 1)):
        words = ep._draw_words(seed, ub)
        lam, perm = R.draws(seed, ub, 0.5)
        assert words == perm and sorted(words) == list(range(ub)) and all(type(w) is int for w in words)
        assert ep._mix == (lam, 1.0 - lam) and 0.0 <= lam <= 1.0
        # the order, spelled out: seed, the Beta draw, then the permutation
        np.random.seed(seed)
        assert float(np.random.beta(0.5, 0.5)) == lam and [int(p) for p in np.random.permutation(ub)] == perm
        np.random.set_state(np_state)
    assert random.getstate() == py_state
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))
    assert R.draws(11, 10, 0.5) != R.draws(12, 10, 0.5)


def test_base_epocher_draws_the_flip_words_as_before():
    """``TrainEpocher._draw_words`` is the code ``_step`` held inline: same draws from Python's generator under the seed, same words."""
    from deepclustering2.augment.tensor_augment import TensorRandomFlip
    from deepclustering2.decorator import FixRandomSeed
    from miseg_amd import ops
    ep = _bare_epocher("MeanTeacherEpocher")
    for seed, ub in ((7, 3), (123456, 10)):
        with FixRandomSeed(seed):
            decisions = TensorRandomFlip(axis=[1, 2], threshold=0.8).decisions(ub)
        want = ops.flip_masks(list(decisions) + [[False, False]] * ub)
        assert ep._draw_words(seed, ub) == want and len(want) == 2 * ub


def test_coefficient_row_is_staged_behind_the_ema_row():
    from semi_seg import epocher as E
    ep = _bare_epocher()
    ep._draw_words(11, 3)
    lam, _ = R.draws(11, 3, 0.5)
    rows = ep._own_rows()
    assert len(rows) == 2 and rows[0] == [0.0, 1.0, 1.0 - 1e-6, 0.0] and rows[1] == [lam, 1.0 - lam]
    assert tuple(float(np.float32(v)) for v in rows[1]) == R.coefficients(lam)
    mt = _bare_epocher("MeanTeacherEpocher")
    assert mt._own_rows() == [[0.0, 1.0, 1.0 - 1e-6, 0.0]]
    sig = E.ICTEpocher._tape_signature
    assert sig is not E.MeanTeacherEpocher._tape_signature


def test_meter_names_are_the_mean_teachers():
    from deepclustering2.meters2 import MeterInterface
    from semi_seg import epocher as E
    names = []
    for klass in (E.ICTEpocher, E.MeanTeacherEpocher):
        ep = object.__new__(klass)
        ep._model = types.SimpleNamespace(num_classes=4)
        names.append(ep._configure_meters(MeterInterface()).meter_names)
    assert names[0] == names[1] == ["lr", "sup_loss", "reg_loss", "sup_dice", "reg_weight"]


def test_mixed_batch_and_loss_fallbacks_on_materialised_operands():
    """Images the kernel does not take (here: float64 on the CPU) are mixed by torch; a criterion that is neither ``nn.MSELoss`` nor the
    fused ``KL_div`` is called once on materialised operands."""
    from miseg_amd import stepio
    from semi_seg import epocher as E
    ep = _bare_epocher()
    ep._ema_row = 1
    coef = torch.tensor([0.25, 0.75])
    fake = types.SimpleNamespace(hyper=lambda gi: torch.cat([coef, torch.zeros(6)]) if gi == 2 else None)
    lab, unl = torch.rand(2, 1, 4, 5, dtype=torch.float64), torch.rand(3, 1, 4, 5, dtype=torch.float64)
    perm = torch.tensor(PERM, dtype=torch.int32)
    stepio.CURRENT = fake
    try:
        batch = ep._student_batch(lab, unl, perm)
    finally:
        stepio.CURRENT = None
    assert batch.dtype == torch.float64 and torch.equal(batch[:2], lab)
    torch.testing.assert_close(batch[2:], R.mix_rows(unl, PERM, 0.25, 0.75), rtol=1e-14, atol=0)
    a, b = _ab()
    calls = []

    def criterion(p, q):
        calls.append((p, q))
        return ((p - q) ** 2).mean()

    out = E.mix_consistency_loss(criterion, a.requires_grad_(True), b, perm, coef)
    assert len(calls) == 1 and calls[0][0].requires_grad and not calls[0][1].requires_grad
    want, _ = R.loss_and_grad("mse", a, b, PERM, 0.25, 0.75)
    assert abs(float(out) - float(want)) <= 1e-5 * float(want)


# ---------------------------------------------------------------------------------------------------------------- the library, the config
def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    import test_cpu_tape_table as TABLE
    header, _ = th.assert_entry_points(NEW)
    assert _cabi.lib().miseg_version() >= 417
    assert "ict.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    for name in NEW:
        ep = TABLE.EPS[name]
        assert ep.file == "ict.hip" and TABLE.macro_args(ep)[1:] == ep.params
        assert len(_cabi.PROTOTYPES[name][1]) == len(ep.params)
    assert TABLE.EPS["miseg_cat_mixed"].params == ["stream", "a", "Na", "b", "Nb", "C", "H", "W", "perm", "coef", "out", "bad"]
    loss = ["stream", "a", "b", "perm", "coef", "N", "H", "W", "C", "upstream", "loss", "ga", "bad", "ws", "ws_bytes"]
    assert TABLE.EPS["miseg_softmax_mix_mse"].params == TABLE.EPS["miseg_softmax_mix_klcons"].params == loss


def test_ops_offers_the_wrappers_in_their_families():
    from miseg_amd import ops
    from miseg_amd.ops import batch, losses
    assert ops.cat_mixed is batch.cat_mixed
    assert ops.softmax_mix_mse is losses.softmax_mix_mse and ops.softmax_mix_kl_consistency is losses.softmax_mix_kl_consistency
    assert issubclass(losses._SoftmaxMixMSE, losses._ScaledGradLoss) and issubclass(losses._SoftmaxMixKLCons, losses._SoftmaxMixMSE)


SEMI_YAML = {
    "RandomSeed": 10,
    "Arch": {"input_dim": 1, "num_classes": 4},
    "Optim": {"name": "Adam", "lr": 0.0000001, "weight_decay": 0.00001},
    "Scheduler": {"multiplier": 400, "warmup_max": 10},
    "Data": {"name": "acdc", "labeled_data_ratio": 0.05, "unlabeled_data_ratio": 0.95},
    "LabeledData": {"shuffle": True, "batch_size": 4, "num_workers": 4},
    "UnlabeledData": {"shuffle": True, "batch_size": 10, "num_workers": 4},
    "Trainer": {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "feature_importance": [1, 0.5, 0.5], "name": "partial", "save_dir": "tmp",
                "device": "cuda", "num_batches": 500, "max_epoch": 100},
    "UDARegCriterion": {"name": "mse", "weight": 5.0},
    "IICRegParameters": {"EncoderParams": {"num_clusters": 20, "num_subheads": 5, "head_types": "linear", "normalize": False},
                         "DecoderParams": {"num_clusters": 20, "num_subheads": 5, "head_types": "linear", "normalize": False},
                         "LossParams": {"paddings": [1, 3], "patch_sizes": 1024}, "weight": 0.1},
    "EntropyMinParameters": {"weight": 0.00001},
    "MeanTeacherParameters": {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 0.000001},
    "MIDLPaperParameters": {"iic_weight": 0.1, "padding": 1, "patch_size": 1024},
}


def test_semi_yaml_parses_to_the_same_dictionary_and_documents_the_section():
    import yaml
    path = os.path.join(PKG, "config", "semi.yaml")
    assert yaml.safe_load(open(path)) == SEMI_YAML
    text = open(path).read()
    assert "#ICTParameters:" in text
    for key, value in (("name", "mse"), ("weight", "10.0"), ("alpha", "0.999"), ("weight_decay", "0.000001"), ("mix_alpha", "1.0")):
        assert f"#  {key}: {value}" in text, key
