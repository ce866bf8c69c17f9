"""CPU side of virtual adversarial training (``Trainer.name=vat``): the float64 restatement against the wheel's
own run (tests/golden/vat.npz), the Python Philox against the published known answer, the configuration section, the registration,
``VATLoss``'s refusals and the library's new entry points."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402
import trainer_harness as th  # noqa: E402
import vat_ref  # noqa: E402
from oracle import unet as OU  # noqa: E402
from trainer_harness import PKG  # noqa: E402

NEW = {"miseg_conv3x3_stem_dgrad": 11, "miseg_conv3x3_stem_dgrad_supported": 3, "miseg_conv3x3_stem_dgrad_ws_bytes": 1,
       "miseg_l2_perturb": 12, "miseg_l2_perturb_ws_bytes": 2, "miseg_normal_fill": 5, "miseg_philox_fill": 5}
T = torch.from_numpy


def _state(seed, dtype):
    sd = OU.init_state(1, 4, seed=seed)
    trainable = OU.trainable_keys(sd)
    for k in sd:
        if sd[k].is_floating_point():
            sd[k] = sd[k].to(dtype)
    for k in trainable:
        sd[k].requires_grad_()
    return sd, trainable


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_restatement_reproduces_the_wheels_run(golden, case):
    """float64 ``vat_ref.vat`` over the oracle U-Net against what the wheel's ``VATLoss`` produced on the same ``d0``: the clean
    prediction, every direction, ``r_adv``, ``lds``, the parameter gradients (norms of all, two whole tensors) and the BatchNorm
    statistics after the call -- one tracked pass, whatever ``ip``.  Both are float64: 1e-9."""
    g = golden("vat")
    shape = tuple(int(v) for v in g["cfg/shape"])
    x, d0 = T(synth.uniform("vat/x", shape)).double(), T(synth.normal("vat/d0", shape)).double()
    sd, trainable = _state(int(g["cfg/model_seed"]), torch.float64)
    eps = g[f"{case}/eps"]
    eps = float(eps) if eps.ndim == 0 else T(eps)
    res = vat_ref.vat(vat_ref.oracle_model(sd), x, d0, float(g[f"{case}/xi"]), eps, float(g["cfg/prop_eps"]), int(g[f"{case}/ip"]))
    res["lds"].backward()
    assert len(res["d"]) == int(g[f"{case}/ip"]) + 1
    np.testing.assert_allclose(res["pred"].softmax(1).numpy(), g[f"{case}/pred"], rtol=1e-9, atol=1e-12)
    for i, d in enumerate(res["d"]):
        assert vat_ref.rel_l2_per_sample(d, T(g[f"{case}/d{i}"])) < 1e-9, i
        np.testing.assert_allclose(d.reshape(shape[0], -1).norm(dim=1).numpy(), 1.0, rtol=1e-12)
    assert vat_ref.rel_l2_per_sample(res["r_adv"], T(g[f"{case}/r_adv"])) < 1e-9
    np.testing.assert_allclose(float(res["lds"]), float(g[f"{case}/lds"]), rtol=1e-9)
    names = [str(n) for n in g[f"{case}/grad_names"]]
    assert names == trainable
    np.testing.assert_allclose([float(sd[n].grad.norm()) for n in names], g[f"{case}/grad_norms"], rtol=1e-8)
    for n in (str(w) for w in g["whole"]):
        assert vat_ref.rel_l2(sd[n].grad, T(g[f"{case}/grad/{n}"])) < 1e-9, n
    np.testing.assert_allclose(sd["Conv1.conv.1.running_mean"].numpy(), g[f"{case}/bn/running_mean"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sd["Conv1.conv.1.running_var"].numpy(), g[f"{case}/bn/running_var"], rtol=1e-9)
    assert int(sd["Conv1.conv.1.num_batches_tracked"]) == int(g[f"{case}/bn/num_batches_tracked"]) == 1


def test_tensor_eps_scales_each_sample():
    g = torch.Generator().manual_seed(0)
    x, d0 = torch.rand(3, 1, 8, 8, generator=g, dtype=torch.float64), torch.randn(3, 1, 8, 8, generator=g, dtype=torch.float64)
    w = torch.randn(4, 1, 3, 3, generator=g, dtype=torch.float64)
    model = lambda t, tracked: torch.nn.functional.conv2d(t, w, padding=1)  # noqa: E731
    res = vat_ref.vat(model, x, d0, eps=torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64), prop_eps=0.25, ip=1)
    np.testing.assert_allclose(res["r_adv"].reshape(3, -1).norm(dim=1).numpy(), [0.125, 0.25, 0.5], rtol=1e-12)


def test_philox_known_answers():
    """Philox4x32-10: the published vectors (Random123 kat_vectors): zero counter and key; all ones; the digits of pi."""
    def hexes(v):
        return " ".join(f"{w:08x}" for w in v)
    assert hexes(vat_ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(vat_ref.philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(vat_ref.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_words_depend_on_seed_and_position_only():
    a = vat_ref.philox_words(5, 0, 12)
    assert np.array_equal(np.concatenate([vat_ref.philox_words(5, 0, 5), vat_ref.philox_words(5, 5, 7)]), a)
    assert not np.array_equal(vat_ref.philox_words(6, 0, 12), a)
    z = vat_ref.normals_from_words(a, 0)
    assert z.shape == (12,) and np.isfinite(z).all()


def test_config_section_parses_with_its_defaults():
    import yaml
    from deepclustering2.configparser import ConfigManger
    from semi_seg.trainer import VATTrainer
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    # the section is optional and the shipped file does not carry it (the other trainers' saved config.yaml keeps the reference's keys)
    assert "VATParameters" not in cfg
    assert VATTrainer.parameters(cfg) == {"weight": 1.0, "xi": 10.0, "eps": 1.0, "prop_eps": 0.25, "ip": 1}
    assert VATTrainer.parameters({}) == VATTrainer.parameters(cfg) == VATTrainer.parameters({"VATParameters": None})
    # ... a partial one is completed from the class's defaults, which are VATLoss's
    from deepclustering2.utils.VAT import VATLoss
    crit = VATLoss()
    assert {"xi": crit.xi, "eps": crit.eps, "prop_eps": crit.prop_eps, "ip": crit.ip} == {k: v for k, v in VATTrainer.DEFAULTS.items() if k != "weight"}
    assert VATTrainer.parameters({"VATParameters": {"ip": 2, "weight": 0.5}}) == {"weight": 0.5, "xi": 10.0, "eps": 1.0, "prop_eps": 0.25, "ip": 2}
    with pytest.raises(KeyError, match="unknown keys"):
        VATTrainer.parameters({"VATParameters": {"epsilon": 1.0}})
    over = ConfigManger(os.path.join(PKG, "config", "semi.yaml"), verbose=False, argv=["Trainer.name=vat", "VATParameters.eps=2.5",
                                                                                        "VATParameters.ip=2"]).config
    assert VATTrainer.parameters(over)["eps"] == 2.5 and VATTrainer.parameters(over)["ip"] == 2


def test_trainer_zoo_has_vat_and_builds_its_epocher():
    import yaml
    from deepclustering2.meters2 import MeterInterface
    from deepclustering2.utils.VAT import VATLoss
    from semi_seg import epocher as E
    from semi_seg.trainer import SemiTrainer, VATTrainer, trainer_zoos
    assert trainer_zoos["vat"] is VATTrainer and issubclass(VATTrainer, SemiTrainer)
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin", "contrast", "contrastdecoder"} <= set(trainer_zoos)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    cfg["VATParameters"] = dict(weight=0.5, ip=2, eps=2.0)
    tr = th.bare_trainer("vat", cfg)
    ep = tr._make_epocher()
    assert type(ep) is E.VATEpocher and issubclass(E.VATEpocher, E.TrainEpocher)
    assert ep._reg_weight == 0.5 and isinstance(ep._vat, VATLoss)
    assert (ep._vat.xi, ep._vat.eps, ep._vat.prop_eps, ep._vat.ip) == (10.0, 2.0, 0.25, 2)
    assert ep._TRAIN_FORWARDS == 1                     # accumulator room for the labeled pass; the loss's passes use float sums
    assert sorted(ep._configure_meters(MeterInterface()).meter_names) == ["lr", "reg_loss", "reg_weight", "sup_dice", "sup_loss"]
    ep.enable_step_tape()                              # a documented no-op: the iteration runs eagerly
    assert ep._step_tape is None
    # no module of its own on the trainer: the checkpoint tree stays the partial one
    assert not any(hasattr(v, "state_dict") for k, v in vars(tr).items() if k not in ("_model", "_sup_criterion"))


def test_float16_storage_is_refused():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    cfg["Arch"]["compute_dtype"] = "float16"
    with pytest.raises(NotImplementedError, match="float32 or bfloat16"):
        th.bare_trainer("vat", cfg)


def test_checkpoint_key_tree_after_init_is_the_partial_trainers(golden, tmp_path):
    from test_cpu_host import _build_trainer
    tr = _build_trainer("vat", tmp_path / "run")
    mine = sorted(synth.tree_lines(tr.state_dict()))
    assert mine == [str(x) for x in golden("trainer_io")["partial/tree_after_init"]]


def test_vatloss_refuses_bad_arguments():
    from deepclustering2.utils.VAT import VATLoss
    for ip in (0, -1, 1.5):
        with pytest.raises(ValueError, match="ip must be an integer >= 1"):
            VATLoss(ip=ip)
    with pytest.raises(NotImplementedError, match="eps should be tensor or float"):
        VATLoss(eps="1.0")
    x = torch.zeros(3, 1, 8, 8)

    def model(_):
        raise AssertionError("the model must not run before the arguments are checked")
    for eps in (torch.ones(2), torch.ones(4), torch.ones(3, 1, 1, 1), torch.ones(1, 3)):
        with pytest.raises(ValueError, match=r"one value per sample, shape \[3\]"):
            VATLoss(eps=eps)(model, x)
    with pytest.raises(ValueError, match="float32 batch"):
        VATLoss()(model, x.double())
    crit = VATLoss()
    assert (crit.xi, crit.eps, crit.prop_eps, crit.ip) == (10.0, 1.0, 0.25, 1) and crit.distance_func.supports_fused()


def test_l2_normalize_on_the_cpu():
    from deepclustering2.utils.VAT import _l2_normalize
    d = torch.randn(3, 2, 5, 7, generator=torch.Generator().manual_seed(1))
    out = _l2_normalize(d)
    torch.testing.assert_close(out.reshape(3, -1).norm(dim=1), torch.ones(3))
    torch.testing.assert_close(out, vat_ref.l2_normalize(d))


def test_header_declares_and_library_exports_the_new_entry_points():
    from miseg_amd import _cabi
    _, exported = th.assert_entry_points(NEW)
    for name, nargs in NEW.items():
        assert len(_cabi.PROTOTYPES[name][1]) == nargs, (name, len(_cabi.PROTOTYPES[name][1]))
    assert re.search(r"\bT f16_miseg_conv3x3_stem_dgrad$", exported, re.M)        # the fp16 twin of the storage-typed entry point
    assert _cabi.lib().miseg_version() >= 414


def test_stem_dgrad_query_and_workspace_sizes():
    """Pure host functions: which shapes the stem's data-gradient kernel takes (the rest goes through the generic path)."""
    from miseg_amd import _cabi
    q = _cabi.lib().miseg_conv3x3_stem_dgrad_supported
    for dt in (_cabi.F32, _cabi.BF16, _cabi.F16):
        assert q(dt, 16, 53) and q(dt, 16, 300) and q(dt, 16, 1022) and q(dt, 64, 256) and q(dt, 8, 5)
        assert not q(dt, 16, 1023) and not q(dt, 16, 0) and not q(dt, 72, 64)
        assert bool(q(dt, 12, 64)) == (dt == _cabi.F32)            # whole 16-byte vectors: 4 floats, 8 halves
    assert q(_cabi.F32, 4, 64) and not q(_cabi.BF16, 4, 64) and not q(3, 16, 64)
    assert _cabi.lib().miseg_conv3x3_stem_dgrad_ws_bytes(16) == 16 * 9 * 4
    assert _cabi.lib().miseg_l2_perturb_ws_bytes(3, 1) == 3 * 8
    assert _cabi.lib().miseg_l2_perturb_ws_bytes(2, 256 * 256) == 2 * 16 * 8
    assert _cabi.lib().miseg_l2_perturb_ws_bytes(1, 10 ** 7) == 64 * 8


def test_bf16_rounded_restatement_is_the_oracles_in_float32_and_runs_in_float64():
    """``vat_ref.unet_bf16_rounded`` -- the yardstick of the bf16 comparison on the GPU -- gives the bits of the oracle's
    ``unet_forward_bf16_autograd`` in float32 (value and image gradient), and runs in float64, where every stored value is still a
    bf16 number."""
    sd, _ = _state(13, torch.float32)
    x = T(synth.uniform("vat/x", (3, 1, 32, 48))).requires_grad_()
    mine, theirs = vat_ref.unet_bf16_rounded(sd, x), OU.unet_forward_bf16_autograd(sd, x)[0]
    assert torch.equal(mine, theirs)
    (ga,), (gb,) = torch.autograd.grad(mine.square().sum(), x), torch.autograd.grad(theirs.square().sum(), x)
    assert torch.equal(ga, gb)
    sd64, _ = _state(13, torch.float64)
    out = vat_ref.unet_bf16_rounded(sd64, x.detach().double())
    assert out.dtype == torch.float64 and torch.isfinite(out).all()
    r = vat_ref._RoundBF16.apply(torch.tensor([1.0 + 2.0 ** -9, 3.14159], dtype=torch.float64), True)
    assert r.dtype == torch.float64 and torch.equal(r, r.bfloat16().double()) and float(r[0]) == 1.0
