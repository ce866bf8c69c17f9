"""CPU side of the cross pseudo supervision trainer (``Trainer.name=cps``): the float64 restatement of its kernel
(tests/cps_ref.py) against float64 autograd of ``F.cross_entropy`` on fixed labels, the condition under which the GPU test may compare
labels exactly, registration and the ``CPSParameters`` section, the host side of the epocher, the library's new entry points, and
config/semi.yaml -- which documents the section as a comment and must parse as before."""
import os
import types

import pytest
import torch

import cps_ref as R
import pixel_ref as P
import trainer_harness as th
from trainer_harness import PKG

NEW = ("miseg_softmax_cross_pseudo", "miseg_softmax_cross_pseudo_ws_bytes")
SHAPE = (3, 4, 5, 7)           # N, C, H, W


def _ab(scale=2.0):
    n, c, h, w = SHAPE
    return P.logits("cps/cpu/a", n, c, h, w, scale), P.logits("cps/cpu/b", n, c, h, w, scale)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("scale", [2.0, 30.0])
def test_hand_gradient_equals_float64_autograd_of_cross_entropy(scale):
    a, b = _ab(scale)
    (la, lb), (ga, gb), agree = R.loss_grads_agree(a, b)
    for z, y, loss, grad in ((a, R.labels(b), la, ga), (b, R.labels(a), lb, gb)):
        want_loss, want_grad = R.autograd_one_sided(z, y)
        assert abs(float(loss) - float(want_loss)) <= 1e-13 * abs(float(want_loss))
        assert float((grad - want_grad).abs().max()) <= 1e-13 * float(want_grad.abs().max())
    n, c, h, w = SHAPE
    assert 0 < agree < n * h * w and agree == int((a.argmax(1) == b.argmax(1)).sum())
    if scale == 2.0:         # (bounded logits: no softmax entry rounds to 1)
        assert torch.equal(R.implied_labels(ga), R.labels(b)) and torch.equal(R.implied_labels(-2.5 * gb, -2.5), R.labels(a))


def test_the_labels_are_detached_and_the_loss_is_plain_cross_entropy():
    """Nothing flows through the argmax: a's gradient is that of CE(a, fixed labels); identical operands agree everywhere and the loss
    is then the mean of -log max softmax."""
    a, _ = _ab()
    (la, lb), (ga, gb), agree = R.loss_grads_agree(a, a.clone())
    n, c, h, w = SHAPE
    assert agree == n * h * w and float(la) == float(lb) and torch.equal(ga, gb)
    want = -(a.to(R.F64).softmax(1).max(1).values.log()).mean()
    assert abs(float(la) - float(want)) <= 1e-13 * float(want)
    assert float(ga.sum(1).abs().max()) <= 1e-14 * float(ga.abs().max())         # softmax - one-hot sums to zero over the classes


@pytest.mark.parametrize("name", list(P.LOSS_CASES))
def test_no_loss_case_has_a_tied_pixel(name):
    """The GPU test compares ``agree`` exactly on these cases.  No pixel of any of them is a tie, so that comparison does not depend
    on the tie rule; the rule itself is pinned on ``pixel_ref.tie_logits``."""
    a, b = P.case_inputs("mse", name)
    assert float(R.top_two_gap(a).min()) > 0.0 and float(R.top_two_gap(b).min()) > 0.0


@pytest.mark.parametrize("c", [3, 4, 16])
def test_tie_rule_of_the_reference_is_the_first_maximum(c):
    a, b = P.tie_logits(f"cps/tie/a{c}", 3, c, 19, 23), P.tie_logits(f"cps/tie/b{c}", 3, c, 19, 23)
    assert float((R.top_two_gap(a) == 0).float().mean()) > 0.3          # ties at a large share of the pixels
    y = R.labels(a)
    top = a.max(1, keepdim=True).values
    first = (a == top).float().argmax(1)              # -0.0 == 0.0: both count as the maximum
    assert torch.equal(y, first) and torch.equal(y, P.first_argmax(a))
    _, (ga, gb), agree = R.loss_grads_agree(a, b)
    assert torch.equal(R.implied_labels(ga), R.labels(b)) and torch.equal(R.implied_labels(gb), y)
    assert agree == int((y == R.labels(b)).sum())


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_zoo_has_cps():
    from semi_seg import epocher as E
    from semi_seg.trainer import CPSTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["cps"] is CPSTrainer and issubclass(CPSTrainer, SemiTrainer) and CPSTrainer.NAME == "cps"
    assert CPSTrainer.SINGLE_PROCESS is None
    assert issubclass(E.CPSEpocher, E.TrainEpocher) and E.CPSEpocher._TRAIN_FORWARDS == 2
    assert CPSTrainer._inference_model is SemiTrainer._inference_model            # validation, test and inference: network A
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin", "vat", "ict", "uamt", "contrast", "contrastdecoder"} <= set(trainer_zoos)


def test_parameters_defaults_unknown_keys_and_negative_weight():
    from semi_seg.trainer import CPSTrainer
    defaults = dict(weight=1.5, on_labeled=True)
    assert CPSTrainer.parameters({}) == defaults and CPSTrainer.parameters(None) == defaults
    assert CPSTrainer.parameters({"CPSParameters": None}) == defaults
    got = CPSTrainer.parameters({"CPSParameters": {"weight": 3, "on_labeled": False}})
    assert got == dict(weight=3.0, on_labeled=False) and isinstance(got["weight"], float) and got["on_labeled"] is False
    assert CPSTrainer.parameters({"CPSParameters": {"weight": 0}})["weight"] == 0.0
    with pytest.raises(KeyError):
        CPSTrainer.parameters({"CPSParameters": {"threshold": 0.9}})
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            CPSTrainer.parameters({"CPSParameters": {"weight": bad}})


def test_trainer_init_builds_the_second_network_and_hands_both_to_the_optimiser():
    from contrastyou.arch import UNet
    from semi_seg import epocher as E
    cfg = th.semi_config()
    assert "CPSParameters" not in cfg
    tr = th.bare_trainer("cps", cfg)
    assert tr._reg_weight == 1.5 and tr._on_labeled is True
    assert isinstance(tr._model_b, UNet) and tr._model_b is not tr._model and tr._model_b.training
    assert all(p.requires_grad for p in tr._model_b.parameters())
    names = [n for n, _ in tr._model.named_parameters()]
    assert [n for n, _ in tr._model_b.named_parameters()] == names
    assert any(not torch.equal(p, q) for p, q in zip(tr._model.parameters(), tr._model_b.parameters()))       # its own initialisation
    both = list(tr._trainable())
    assert len(both) == 2 * len(names) and [id(p) for p in both] == [id(p) for p in tr._model.parameters()] + [id(p) for p in tr._model_b.parameters()]
    tr = th.bare_trainer("cps", th.semi_config(["CPSParameters.weight=0.5", "CPSParameters.on_labeled=false"]))
    assert tr._reg_weight == 0.5 and tr._on_labeled is False
    tr._feature_importance, tr.feature_positions = [1.0], ["Conv5"]
    ep = tr._make_epocher()
    assert type(ep) is E.CPSEpocher and ep._model_b is tr._model_b and ep._on_labeled is False and ep._reg_weight == 0.5
    with pytest.raises(ValueError):
        th.bare_trainer("cps", th.semi_config(["CPSParameters.weight=-1"]))
    with pytest.raises(KeyError):
        th.bare_trainer("cps", th.semi_config(["CPSParameters.alpha=0.99"]))


def test_checkpoint_state_gains_the_second_network():
    """The generic ``Trainer.state_dict`` walks the trainer's attributes: ``_model_b`` is one of them, with ``_model``'s keys."""
    from deepclustering2.trainer import Trainer
    tr = th.bare_trainer("cps", th.semi_config())
    state = {name: module.state_dict() for name, module in tr.__dict__.items() if callable(getattr(module, "state_dict", None))}
    assert set(state["_model_b"]) == set(state["_model"]) and type(tr).state_dict is Trainer.state_dict


# ---------------------------------------------------------------------------------------------------------------- the epocher's host side
def _bare_epocher(on_labeled=True):
    from semi_seg import epocher as E
    ep = object.__new__(E.CPSEpocher)
    ep._on_labeled, ep._pixels_sent = on_labeled, []
    return ep


def test_no_flips_are_staged_and_the_pixel_count_follows_on_labeled():
    for on_labeled, want in ((True, (2 + 3) * 6 * 10), (False, 3 * 6 * 10)):
        ep = _bare_epocher(on_labeled)
        ep._batch_shapes = ((2, 1, 6, 10), (3, 1, 6, 10))
        assert ep._draw_words(11, 3) == [0, 0, 0] and ep._draw_words(12, 3) == [0, 0, 0]
        assert ep._pixels_sent == [want, want]


def test_meter_names():
    from deepclustering2.meters2 import MeterInterface
    from semi_seg import epocher as E
    ep = object.__new__(E.CPSEpocher)
    ep._model = types.SimpleNamespace(num_classes=4)
    assert ep._configure_meters(MeterInterface()).meter_names == ["lr", "sup_loss", "reg_loss", "sup_dice", "sup_loss_b", "agreement", "reg_weight"]


def test_a_plain_optimiser_is_refused_as_the_mean_teacher_refuses_it():
    ep = _bare_epocher()
    ep._optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with pytest.raises(RuntimeError, match="Trainer.name=cps needs a fused optimiser"):
        ep._stage(None, [0])


def test_operands_off_the_device_or_not_fp32_raise_type_error():
    from miseg_amd import ops
    a, b = _ab()
    with pytest.raises(TypeError, match="softmax_cross_pseudo"):
        ops.softmax_cross_pseudo(a, b)                    # CPU tensors: no torch fallback
    with pytest.raises(TypeError, match="softmax_cross_pseudo"):
        ops.softmax_cross_pseudo(a.double(), b.double())


# ---------------------------------------------------------------------------------------------------------------- the library, the config
def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    import test_cpu_tape_table as TABLE
    header, _ = th.assert_entry_points(NEW)
    assert _cabi.lib().miseg_version() >= 419
    assert "cps.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()
    ep = TABLE.EPS["miseg_softmax_cross_pseudo"]
    assert ep.file == "cps.hip" and TABLE.macro_args(ep)[1:] == ep.params
    assert ep.params == ["stream", "a", "b", "N", "H", "W", "C", "upstream", "loss", "ga", "gb", "agree", "ws", "ws_bytes"]
    assert len(_cabi.PROTOTYPES["miseg_softmax_cross_pseudo"][1]) == len(ep.params)
    assert "DESIGN.md section 30" in header


def test_ops_offers_the_wrapper_in_the_loss_family():
    from miseg_amd import ops
    from miseg_amd.ops import losses
    assert ops.softmax_cross_pseudo is losses.softmax_cross_pseudo


def test_semi_yaml_parses_to_the_same_dictionary_and_documents_the_section():
    import yaml
    from test_cpu_ict import SEMI_YAML
    path = os.path.join(PKG, "config", "semi.yaml")
    assert yaml.safe_load(open(path)) == SEMI_YAML
    text = open(path).read()
    assert "#CPSParameters:" in text
    for key, value in (("weight", "1.5"), ("on_labeled", "true")):
        assert f"#  {key}: {value}" in text, key
