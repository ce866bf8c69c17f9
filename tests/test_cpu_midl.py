"""CPU side of the `midl` trainer (``Trainer.name=midl``, the ``MIDLPaperParameters`` section): registration, the sections it reads
(CLI overrides included), its criterion's patch and step sizes, and the library's new entry points."""
import os

import trainer_harness as th
from trainer_harness import PKG, ROOT

NEW = ("miseg_iic_out_joint_fwd", "miseg_iic_out_bwd")


def test_trainer_zoo_has_midl_reading_its_sections():
    import yaml
    from semi_seg import epocher as E
    from semi_seg.trainer import MIDLTrainer, UDATrainer, trainer_zoos
    assert trainer_zoos["midl"] is MIDLTrainer and issubclass(MIDLTrainer, UDATrainer)
    assert {"partial", "uda", "iic", "udaiic", "meanteacher"} <= set(trainer_zoos)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert cfg["MIDLPaperParameters"] == {"iic_weight": 0.1, "padding": 1, "patch_size": 1024}
    tr = th.bare_trainer("midl", cfg)
    assert isinstance(tr._reg_criterion, __import__("torch").nn.MSELoss)
    assert tr._uda_weight == 5.0 and tr._reg_weight == 1.0 and tr._iic_weight == 0.1
    assert (tr._mi_padding, tr._mi_patch_size) == (1, 1024)
    crit = tr.mi_criterion()
    from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    assert isinstance(crit, IIDSegmentationSmallPathLoss)
    assert crit.padding == 1 and crit.lamda == 1.0 and crit._patch_size == (1024, 1024) and crit._step_size == (512, 512)
    assert issubclass(E.MIDLTrainEpocher, E.UDATrainEpocher)
    # no module of its own on the trainer: the checkpoint tree stays the uda one
    assert not any(hasattr(v, "state_dict") for k, v in vars(tr).items() if k not in ("_model", "_reg_criterion", "_sup_criterion"))


def test_cli_overrides_reach_the_trainer():
    cfg = th.semi_config(["Trainer.name=midl", "MIDLPaperParameters.padding=3", "MIDLPaperParameters.patch_size=32",
                          "MIDLPaperParameters.iic_weight=0.5", "UDARegCriterion.name=kl", "UDARegCriterion.weight=2.0"])
    tr = th.bare_trainer("midl", cfg)
    from deepclustering2.loss import KL_div
    assert isinstance(tr._reg_criterion, KL_div) and tr._uda_weight == 2.0 and tr._iic_weight == 0.5
    crit = tr.mi_criterion()
    assert crit.padding == 3 and crit._patch_size == (32, 32) and crit._step_size == (16, 16)


def test_epocher_windows_follow_the_reference_patch_generator():
    """The windows the epocher hands the kernel: the reference's patch_generator (step patch // 2, clamped last windows)."""
    import numpy as np
    from semi_seg.epocher import MIDLTrainEpocher
    ep = MIDLTrainEpocher.__new__(MIDLTrainEpocher)
    from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
    ep._mi_criterion = IIDSegmentationSmallPathLoss(padding=3, patch_size=32)
    wins = ep.windows(64, 64)
    assert len(wins) == 9 and wins[0] == (0, 32, 0, 32) and wins[-1] == (32, 64, 32, 64)
    wins = ep.windows(37, 53)
    hs = list(np.append(np.arange(0, 37 - 32, 16), max(37 - 32, 0)))
    ws = list(np.append(np.arange(0, 53 - 32, 16), max(53 - 32, 0)))
    assert wins == [(h, min(h + 32, 37), w, min(w + 32, 53)) for h in hs for w in ws]
    ep._mi_criterion = IIDSegmentationSmallPathLoss(padding=1, patch_size=1024)
    assert ep.windows(256, 256) == [(0, 256, 0, 256)]


def test_library_exports_and_header_declares_the_new_entry_points():
    th.assert_entry_points(NEW + ("miseg_iic_out_joint_ws_bytes",))


def test_envelope_query():
    """2 <= C <= 8, 0 <= pad <= 3 have a fused path; anything else is refused by the workspace query (the epocher then composes)."""
    from miseg_amd import ops
    assert all(ops.output_local_mi_supported(c, p) for c in range(2, 9) for p in range(4))
    assert not any(ops.output_local_mi_supported(c, p) for c, p in ((1, 1), (9, 1), (12, 1), (4, 4), (4, 5), (4, -1)))


def test_checkpoint_key_tree_after_init_is_the_uda_trainers(golden, tmp_path):
    """No module of its own: ``trainer.state_dict()`` after ``init()`` has the uda trainer's key tree line for line (the REFERENCE uda
    trainer's, tests/golden/trainer_io.npz)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    from test_cpu_host import _build_trainer
    tr = _build_trainer("midl", tmp_path / "run")
    mine = sorted(synth.tree_lines(tr.state_dict()))
    assert mine == [str(x) for x in golden("trainer_io")["uda/tree_after_init"]]
