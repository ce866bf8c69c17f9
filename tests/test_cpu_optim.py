"""RAdam, AdaBound and AdaBoundW behind ``Optim.name``, without a GPU: the restatement of the three rules (tests/optim_ref.py)
against vectors recorded from the wheel's own classes (tests/golden/optim.npz, optim_adabound{,2,3}.npz), the library's two entry points,
the name lookup, the constructors, the checkpoint layout and the host half of a step (``host_step``) -- everything up to the launch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_ref as R

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
STATE = (("p", "p"), ("m", "m"), ("v", "v"), ("vmax", "vmax"))


def _inputs(golden):
    g = golden("optim")
    return T(g["p0"]), [T(g[f"g{t}"]) for t in range(1, R.STEPS + 1)]


# ------------------------------------------------------------------------------------------------ the restatement against the wheel
@pytest.mark.parametrize("name", list(R.RADAM_CASES))
def test_float32_restatement_is_bit_equal_to_the_wheels_radam(golden, name):
    """The wheel's RAdam computes in float32 whatever the parameter's dtype (``p.data.float()``): the float32 restatement must give
    its bits -- parameter and both moments, after each of the 8 steps (1-5 unrectified, 6-8 rectified)."""
    g = golden("optim")
    p0, grads = _inputs(golden)
    assert [R.scalars(name, t)[1] for t in range(1, R.STEPS + 1)] == [0.0] * 5 + [1.0] * 3
    for t, st in enumerate(R.run(name, p0, grads, torch.float32), 1):
        for key in ("p", "m", "v"):
            np.testing.assert_array_equal(st[key].numpy(), g[f"{name}/{key}{t}"], err_msg=f"{name} {key} after step {t}")


@pytest.mark.parametrize("name", list(R.ADABOUND_CASES))
def test_float64_restatement_equals_the_wheels_adabound(golden, name):
    """The AdaBound goldens are float64 runs of the wheel's classes (they compute in the parameter's dtype): 1e-12, every step, every
    state tensor; the clamp is at work in all three of its regimes (the recorded counts)."""
    g = golden(R.golden_file(name))
    p0, grads = _inputs(golden)
    for t, st in enumerate(R.run(name, p0, grads, torch.float64), 1):
        assert ("vmax" in st) == bool(R.ADABOUND_CASES[name]["amsbound"]) == (f"{name}/vmax{t}" in g.files)
        for key in st:
            np.testing.assert_allclose(st[key].numpy(), g[f"{name}/{key}{t}"], rtol=0, atol=1e-12, err_msg=f"{name} {key} after step {t}")
    counts = g[f"{name}/clamp_counts"]
    assert counts.shape == (R.STEPS, 3) and (counts.sum(1) == R.NUMEL).all() and (counts[-1] > 100).all(), counts


# ------------------------------------------------------------------------------------------------ library and lookup
def test_library_declares_and_exports_the_two_steps():
    from miseg_amd import _cabi
    lib = _cabi.lib()
    for sym in ("miseg_radam_step", "miseg_adabound_step"):
        assert sym in _cabi.declared_symbols() and hasattr(lib, sym), sym
    assert lib.miseg_version() >= 415
    # null pointers / bad scalars are refused before any launch (no GPU needed to see that)
    assert lib.miseg_radam_step(None, None, None, None, None, 8, 0.9, 0.999, None, 1.0, None, 0) < 0
    assert b"radam_step" in lib.miseg_last_error()
    assert lib.miseg_adabound_step(None, None, None, None, None, None, 8, 0.9, 0.999, None, 0, 1.0, None, 0) < 0
    assert b"adabound_step" in lib.miseg_last_error()


def test_optim_name_lookup_resolves_to_the_fused_classes():
    from deepclustering2 import optim
    from miseg_amd import flat
    assert optim.__dict__["RAdam"] is flat.FusedRAdam and optim.__dict__["AdaBound"] is flat.FusedAdaBound
    assert optim.__dict__["AdaBoundW"] is flat.FusedAdaBoundW and optim.__dict__["Adam"] is flat.FusedAdam
    assert issubclass(flat.FusedAdaBoundW, flat.FusedAdaBound)
    for cls in (flat.FusedAdam, flat.FusedRAdam, flat.FusedAdaBound):
        assert issubclass(cls, flat.FusedFlatOptimizer) and issubclass(cls, torch.optim.Optimizer)
    assert optim.__dict__["SGD"] is torch.optim.SGD and torch.optim.RAdam is not flat.FusedRAdam      # torch's own stays under its module


@pytest.mark.parametrize("kind", ["AdaBound", "AdaBoundW"])
def test_constructor_errors_are_the_wheels(kind):
    from deepclustering2 import optim
    cls = optim.__dict__[kind]

    def make(**kw):
        return cls([torch.nn.Parameter(torch.zeros(3))], **kw)

    for kw, msg in ((dict(lr=-1e-3), "Invalid learning rate: -0.001"), (dict(eps=-1.0), "Invalid epsilon value: -1.0"),
                    (dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
                    (dict(final_lr=-0.1), "Invalid final learning rate: -0.1"), (dict(gamma=1.0), "Invalid gamma parameter: 1.0")):
        with pytest.raises(ValueError) as e:
            make(**kw)
        assert str(e.value) == msg
    opt = make(lr=2e-3)
    assert opt.base_lrs == [2e-3] and opt.defaults["final_lr"] == 0.1 and opt.defaults["gamma"] == 1e-3 and opt.defaults["amsbound"] is False


# ------------------------------------------------------------------------------------------------ the host half of a step
def _make(name):
    from deepclustering2 import optim
    cfg = {**R.RADAM_CASES, **R.ADABOUND_CASES}[name]
    cls = optim.__dict__[cfg.get("kind", "RAdam")]
    params = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    return cls(params, **R.ctor_args(cfg)), cfg, params


@pytest.mark.parametrize("name", list(R.RADAM_CASES) + list(R.ADABOUND_CASES))
def test_host_step_rows_are_the_restatements_scalars(name):
    """Steps 1-8, in double, value for value -- the learning rate moved between steps as a scheduler moves it."""
    opt, cfg, _ = _make(name)
    for t in range(1, R.STEPS + 1):
        opt.param_groups[0]["lr"] = R.lr_of(cfg, t)
        rows = opt.host_step()
        assert len(rows) == 1 and rows[0] == R.scalars(name, t), (t, rows[0], R.scalars(name, t))
        assert len(rows[0]) <= 7
    opt.step_skipped()                    # a skipped update (fp16 overflow) does not count
    assert opt._steps == [R.STEPS - 1]
    assert opt.host_step()[0] == R.scalars(name, R.STEPS)


def test_adam_rows_are_unchanged():
    import math
    from deepclustering2.optim import Adam
    opt = Adam([torch.nn.Parameter(torch.randn(4))], lr=1e-3, weight_decay=1e-5)
    for t in range(1, 4):
        assert opt.host_step() == [[1e-3 / (1 - 0.9 ** t), 1 / math.sqrt(1 - 0.999 ** t), 1e-8, 1e-5]]
    assert opt._HYPER_WORDS == 4 and opt._hyper[0].numel() == 4 and isinstance(opt.state_dict()["state"][0]["step"], torch.Tensor)


@pytest.mark.parametrize("name", list(R.RADAM_CASES)[:1] + list(R.ADABOUND_CASES))
def test_state_dict_has_the_wheels_keys(golden, name):
    """On CPU tensors, as far as the classes go without a launch: empty state before the first step, then -- the flat buffers and
    the moments exist from ``host_step`` on -- per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` (/ ``max_exp_avg_sq``) and exactly the
    wheel's ``param_groups`` keys; a fresh optimiser takes the state back, also before its own buffers exist (deferred)."""
    g = golden(R.golden_file(name))
    opt, cfg, params = _make(name)
    sd = opt.state_dict()
    assert sd["state"] == {} and sorted(sd["param_groups"][0]) == [str(k) for k in g[f"{name}/group_keys"]]
    assert sd["param_groups"][0]["params"] == [0, 1]
    opt.host_step(), opt.host_step()
    with torch.no_grad():
        opt._m[0].copy_(torch.arange(opt._m[0].numel()))
        if cfg.get("amsbound"):
            opt._vmax[0].fill_(3.0)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1] and "loss_scaler" not in sd
    for i, p in enumerate(params):
        st = sd["state"][i]
        assert sorted(st) == [str(k) for k in g[f"{name}/state_keys"]]
        assert type(st["step"]).__name__ == str(g[f"{name}/step_type"]) == "int" and st["step"] == 2
        assert all(st[k].shape == p.shape and st[k].dtype == torch.float32 for k in st if k != "step")
    other, _, other_params = _make(name)
    other.load_state_dict(sd)             # CPU parameters: kept until the buffers are built
    assert other._pending_state is not None and other._steps == [0]
    other.host_step()
    assert other._steps == [3] and torch.equal(other._m[0][:15], opt._m[0][:15])
    if cfg.get("amsbound"):
        assert float(other._vmax[0][:15].min()) == 3.0


def test_amsbound_from_a_checkpoint_brings_its_buffer():
    """``amsbound`` is a ``param_groups`` key, so a checkpoint can switch it on in an optimiser built without it."""
    from deepclustering2.optim import AdaBound
    src = AdaBound([torch.nn.Parameter(torch.randn(6))], amsbound=True)
    src.host_step()
    src._vmax[0].fill_(2.0)
    dst = AdaBound([torch.nn.Parameter(torch.randn(6))])
    dst.host_step()
    assert dst._vmax[0] is None
    dst.load_state_dict(src.state_dict())
    dst.host_step()
    assert dst.param_groups[0]["amsbound"] is True and float(dst._vmax[0][:6].min()) == 2.0


def test_launch_without_a_gpu_is_an_error_not_a_fallback():
    from deepclustering2.optim import RAdam
    from miseg_amd._cabi import MisegError
    p = torch.nn.Parameter(torch.randn(9))
    opt = RAdam([p])
    p.grad = torch.ones(9)
    with pytest.raises(MisegError):
        opt.step()


# ------------------------------------------------------------------------------------------------ data-parallel attachment
def _ddp_worker(rank, world, port, out_dir, optim_name):
    """``build_trainer`` in a 2-rank gloo job on CPU tensors (the pattern of tests/test_cpu_ddp.py): ``ddp.attach`` takes the fused
    optimiser's flat gradient buffer and the mean of the ranks' surrogate gradients lands in it."""
    sys.path.insert(0, SRC)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MISEG_PROGRESS="0")
    from miseg_amd import flat
    from semi_seg.main import build_trainer
    trainer = build_trainer(["Trainer.name=partial", "Trainer.device=cpu", f"Trainer.save_dir={os.path.join(out_dir, 'run')}",
                             "Trainer.max_epoch=1", "Trainer.num_batches=1", "Data.name=synthetic", "Data.size=32",
                             "LabeledData.batch_size=1", "UnlabeledData.batch_size=1", f"Optim.name={optim_name}"])
    opt, red = trainer._optimizer, trainer._grad_reducer
    assert type(opt) is getattr(flat, "Fused" + optim_name) and red is not None and red.world == world and red.flat is opt.flat
    opt.zero_grad()
    red.prepare()
    sum(((rank + 1.0) * 0.5 * (p ** 2).sum()) for p in trainer._model.parameters()).backward()
    red.finish()
    torch.save({"grad": opt.flat.flat_grad.clone(), "param": opt.flat.flat_param.clone()}, os.path.join(out_dir, f"o{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("optim_name", ["RAdam", "AdaBound"])
def test_data_parallel_attach_accepts_the_fused_optimisers(tmp_path, optim_name):
    world, port = 2, 33500 + (os.getpid() + len(optim_name)) % 2000
    mp.spawn(_ddp_worker, args=(world, port, str(tmp_path), optim_name), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f"o{r}.pt") for r in range(world))
    assert torch.equal(r0["param"], r1["param"]) and torch.equal(r0["grad"], r1["grad"])
    torch.testing.assert_close(r0["grad"], 1.5 * r0["param"], rtol=1e-6, atol=1e-9)
