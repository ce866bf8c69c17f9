"""CPU side of the `entmin` trainer (``Trainer.name=entmin``, the ``EntropyMinParameters`` section): registration, the section it
reads (CLI override included), the epocher it builds, the library's new entry point, the class-count query, the checkpoint tree and
``Entropy.supports_fused``."""
import os
import re

import trainer_harness as th
from trainer_harness import PKG, ROOT

NEW = "miseg_softmax_entropy"
DISPATCH = (2, 3, 4, 5, 6, 8, 10, 16)          # MISEG_DISPATCH_C of csrc/pixel_loss.h


def test_trainer_zoo_has_entmin_reading_its_section():
    import yaml
    from semi_seg import epocher as E
    from semi_seg.trainer import EntropyMinTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["entmin"] is EntropyMinTrainer and issubclass(EntropyMinTrainer, SemiTrainer)
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl"} <= set(trainer_zoos)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert cfg["EntropyMinParameters"] == {"weight": 0.00001}          # the shipped default stays
    tr = th.bare_trainer("entmin", cfg)
    assert tr._reg_weight == cfg["EntropyMinParameters"]["weight"] == 1e-5
    ep = tr._make_epocher()
    assert type(ep) is E.EntropyMinEpocher and issubclass(E.EntropyMinEpocher, E.TrainEpocher)
    assert ep._reg_weight == 1e-5
    from deepclustering2.meters2 import MeterInterface
    assert sorted(ep._configure_meters(MeterInterface()).meter_names) == ["entropy", "lr", "reg_loss", "sup_dice", "sup_loss"]
    assert getattr(ep.regularization, "_miseg_fused", False)
    # no module of its own on the trainer: the checkpoint tree stays the partial one
    assert not any(hasattr(v, "state_dict") for k, v in vars(tr).items() if k not in ("_model", "_sup_criterion"))


def test_cli_override_reaches_the_epocher():
    tr = th.bare_trainer("entmin", th.semi_config(["Trainer.name=entmin", "EntropyMinParameters.weight=0.5"]))
    assert tr._reg_weight == 0.5
    assert tr._make_epocher()._reg_weight == 0.5


def test_library_exports_and_header_declares_the_new_entry_point():
    from miseg_amd import _cabi
    header, _ = th.assert_entry_points([NEW])
    assert re.search(r"\bint\s+" + NEW + r"\s*\(", header)
    restype, argtypes = _cabi.PROTOTYPES[NEW]
    assert len(argtypes) == 11                     # stream, logits, N, H, W, C, upstream, loss, glogits, ws, ws_bytes


def test_supported_class_counts_mirror_the_dispatch_list():
    from miseg_amd import ops
    assert [c for c in range(0, 40) if ops.softmax_entropy_supported(c)] == list(DISPATCH)
    # ... which is the list the library's source dispatches on: the one switch of the pixel-loss units, which the entry point's unit uses
    assert "MISEG_DISPATCH_C(C, L)" in open(os.path.join(PKG, "csrc", "losses.hip")).read()
    src = open(os.path.join(PKG, "csrc", "pixel_loss.h")).read()
    macro = src[src.index("#define MISEG_DISPATCH_C"):]
    macro = macro[:macro.index("default:")]
    assert tuple(int(m) for m in re.findall(r"case (\d+):", macro)) == DISPATCH


def test_checkpoint_key_tree_after_init_is_the_partial_trainers(golden, tmp_path):
    """No module of its own: ``trainer.state_dict()`` after ``init()`` has the partial trainer's key tree line for line (the REFERENCE
    partial trainer's, tests/golden/trainer_io.npz)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    from test_cpu_host import _build_trainer
    tr = _build_trainer("entmin", tmp_path / "run")
    mine = sorted(synth.tree_lines(tr.state_dict()))
    assert mine == [str(x) for x in golden("trainer_io")["partial/tree_after_init"]]


def test_entropy_supports_fused_for_the_defaults_only():
    from deepclustering2.loss import Entropy
    assert Entropy().supports_fused() and Entropy(reduction="mean", eps=1e-16).supports_fused()
    assert not Entropy(reduction="sum").supports_fused()
    assert not Entropy(reduction="none").supports_fused()
    assert not Entropy(eps=1e-8).supports_fused()


def test_entropy_forward_is_unchanged():
    """``forward`` stays the wheel's expression."""
    import torch
    from deepclustering2.loss import Entropy
    p = torch.randn(3, 5, 7, 6, generator=torch.Generator().manual_seed(0)).softmax(1)
    ref = -(p * (p + 1e-16).log()).sum(1)
    assert torch.equal(Entropy()(p), ref.mean()) and torch.equal(Entropy(reduction="sum")(p), ref.sum())
    assert torch.equal(Entropy(reduction="none")(p), ref)
