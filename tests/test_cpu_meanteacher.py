"""CPU side of the Mean Teacher trainer (``Trainer.name=meanteacher``): registration and config section, the updater's alpha schedule
and state, the library's new entry points."""
import os
import re

import pytest

import trainer_harness as th
from trainer_harness import PKG

NEW = ("miseg_ema_update", "miseg_cat_flipped")


def test_trainer_zoo_has_meanteacher_reading_its_section():
    import yaml
    from semi_seg import epocher as E
    from semi_seg.trainer import MeanTeacherTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["meanteacher"] is MeanTeacherTrainer and issubclass(MeanTeacherTrainer, SemiTrainer)
    assert {"partial", "uda", "iic", "udaiic"} <= set(trainer_zoos)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    sec = cfg["MeanTeacherParameters"]
    assert sec == {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 1e-6}
    tr = MeanTeacherTrainer.__new__(MeanTeacherTrainer)
    tr._config = {**cfg, "Trainer": dict(cfg["Trainer"]), "MeanTeacherParameters": dict(sec, name="kl", weight=3.5, alpha=0.99)}
    tr._model = __import__("contrastyou.arch", fromlist=["UNet"]).UNet(**cfg["Arch"])
    tr._init()
    from deepclustering2.loss import KL_div
    assert isinstance(tr._reg_criterion, KL_div) and tr._reg_weight == 3.5
    assert tr._ema_updater._alpha == 0.99 and tr._ema_updater._weight_decay == 1e-6 and not tr._ema_updater._update_bn
    assert all(not p.requires_grad for p in tr._teacher_model.parameters()) and tr._teacher_model.training
    assert tr._teacher_model is not tr._model
    assert E.MeanTeacherEpocher._TRAIN_FORWARDS == 2 and E.TrainEpocher._TRAIN_FORWARDS == 1


def test_ema_updater_schedule_and_state_round_trip(golden):
    """alpha_k = min(1 - 1/(k+1), alpha) of the wheel's updater, as recorded from the reference run; the call count round-trips."""
    from deepclustering2.models import ema_updater
    g = golden("meanteacher")
    u = ema_updater(alpha=0.999, justify_alpha=True, weight_decay=1e-6)
    got = [u.host_step()[0] for _ in range(len(g["alpha"]))]
    assert got == [float(a) for a in g["alpha"]]
    v = ema_updater(alpha=0.999, justify_alpha=True, weight_decay=1e-6)
    v.load_state_dict(u.state_dict())
    assert v.global_step == u.global_step == len(got)
    assert v.host_step() == u.host_step()
    a, b, d = ema_updater(alpha=0.5, justify_alpha=False, weight_decay=0).host_step()
    assert (a, b, d) == (0.5, 0.5, 1.0)


def test_library_exports_and_header_declares_the_new_entry_points():
    header, _ = th.assert_entry_points(NEW)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name


def test_step_block_sizes():
    from miseg_amd import stepio
    assert stepio.block_bytes(1) == stepio.PARAM_BYTES
    assert (stepio.block_bytes(2) - stepio.ACC_OFF) // 8 >= 2 * 3468
