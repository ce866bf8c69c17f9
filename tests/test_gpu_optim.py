"""RAdam, AdaBound and AdaBoundW on the device: ``miseg_radam_step`` / ``miseg_adabound_step`` against the float64 restatement of
the wheel's rules (tests/optim_ref.py, itself pinned to the wheel's classes by tests/test_cpu_optim.py) on the recorded cases, the
grid-stride loop and unaligned views, the guard flags, the loss scale, and the fused optimisers inside the train step: launch tape
against eager iterations across RAdam's sixth step, Mean Teacher, fp16 storage, checkpoints.

Bounds.  Steps 1-3 of every case: the project's Adam bound (rtol 1e-6, atol 1e-7; tests/test_gpu_losses.py::test_adam_matches_oracle).
Steps 4-8: the restatement's own float32 error against float64, measured in the test per case, step and tensor (max |difference|);
the kernel is allowed twice that (run with -s: every case prints both figures at step 8; DESIGN.md section 24 has the table
measured on an MI355X)."""
import random
import warnings

import numpy as np
import pytest
import torch

import optim_ref as R
import trainer_harness as th

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
FEATURES = ["Conv5", "Up_conv3", "Up_conv2"]
FLAT = 2_190_880                  # the flat buffer of the shipped configuration: more than the elementwise grid covers in one pass
ALL_CASES = list(R.RADAM_CASES) + list(R.ADABOUND_CASES)


def _hyper(row, scale=1.0):
    """A step block's 8-word row: values 0-3, 1 / loss scale, values 4-6."""
    row = list(row) + [0.0] * (7 - len(row))
    return torch.tensor(row[:4] + [1.0 / scale] + row[4:], dtype=torch.float32, device=DEV)


def _launch(name, st, g, t, grad_scale=1.0, guard=None, hyper_scale=1.0):
    """One kernel step of case ``name`` on the state dict ``st`` (p, m, v[, vmax]: device fp32), step number ``t``."""
    from miseg_amd import unet_ops
    cfg = {**R.RADAM_CASES, **R.ADABOUND_CASES}[name]
    hyper = _hyper(R.scalars(name, t), hyper_scale)
    b1, b2 = cfg["betas"]
    if name in R.RADAM_CASES:
        unet_ops.radam_step(st["p"], g, st["m"], st["v"], hyper, b1, b2, grad_scale, guard)
    else:
        unet_ops.adabound_step(st["p"], g, st["m"], st["v"], st.get("vmax"), hyper, b1, b2, cfg["kind"] == "AdaBoundW", grad_scale, guard)


def _zero_state(name, p0):
    cfg = {**R.RADAM_CASES, **R.ADABOUND_CASES}[name]
    st = {"p": p0.to(DEV).clone(), "m": torch.zeros(p0.numel(), device=DEV), "v": torch.zeros(p0.numel(), device=DEV)}
    if cfg.get("amsbound"):
        st["vmax"] = torch.zeros(p0.numel(), device=DEV)
    return st


@pytest.fixture(scope="module")
def inputs(golden):
    g = golden("optim")
    return T(g["p0"]), [T(g[f"g{t}"]) for t in range(1, R.STEPS + 1)]


@pytest.fixture(scope="module")
def references(inputs):
    """Per case: the float64 and the float32 restatement after every step (computed once, never written to)."""
    p0, grads = inputs
    return {name: (R.run(name, p0, grads, torch.float64), R.run(name, p0, grads, torch.float32)) for name in ALL_CASES}


# ---------------------------------------------------------------------------------------------------- 1. the kernels on the recorded cases
@pytest.mark.parametrize("name", ALL_CASES)
def test_kernel_follows_the_float64_restatement(inputs, references, name):
    p0, grads = inputs
    ref64, ref32 = references[name]
    st = _zero_state(name, p0)
    for t, g in enumerate(grads, 1):
        _launch(name, st, g.to(DEV), t)
        for key, got in st.items():
            want = ref64[t - 1][key].numpy()
            have = got.cpu().numpy().astype(np.float64)
            if t <= 3:
                np.testing.assert_allclose(have, want, rtol=1e-6, atol=1e-7, err_msg=f"{name} {key} after step {t}")
                continue
            own = float(np.abs(ref32[t - 1][key].numpy().astype(np.float64) - want).max())      # the float32 restatement's error
            err = float(np.abs(have - want).max())
            if t == R.STEPS:
                print(f"{name:28s} {key:5s} step {t}: float32 restatement {own:.3e}   kernel {err:.3e}   ratio {err / own:.2f}")
            assert own > 0 and err <= 2 * own, f"{name} {key} after step {t}: kernel {err:.3e} against twice the restatement's {own:.3e}"


# ---------------------------------------------------------------------------------------------------- 2. sizes and views
KINDS = {"radam": ("radam/b999_wd1e-2", 6), "adabound": ("adabound/wd1e-2_ams", 3), "adaboundw": ("adaboundw/wd1e-2", 3)}
_BIG = {}


def _big(kind):
    """FLAT elements in the regime after a few steps (|m| ~ 0.1 |g|, v ~ 1e-3 g^2, so that no sum cancels beyond the Adam bound's
    atol), one float64 reference step of them (RAdam: step 6, rectified) -- shared by every size."""
    if kind not in _BIG:
        name, t = KINDS[kind]
        gen = torch.Generator().manual_seed(sum(map(ord, kind)))
        st = {"p": torch.randn(FLAT, generator=gen), "m": 0.1 * torch.randn(FLAT, generator=gen),
              "v": 1e-3 * torch.randn(FLAT, generator=gen) ** 2}
        if "ams" in name:
            st["vmax"] = st["v"] * (0.5 + torch.rand(FLAT, generator=gen))        # above v for one half of the elements, below for the other
        g = torch.randn(FLAT, generator=gen)
        ref = {k: x.double().clone() for k, x in st.items()}
        cfg = {**R.RADAM_CASES, **R.ADABOUND_CASES}[name]
        if kind == "radam":
            R.radam_step(ref["p"], g.double(), ref["m"], ref["v"], t, **cfg)
        else:
            a = R.ctor_args(cfg)
            R.adabound_step(ref["p"], g.double(), ref["m"], ref["v"], ref.get("vmax"), t, a["lr"], a["lr"], a["betas"], a["final_lr"], a["gamma"],
                            a["eps"], a["weight_decay"], cfg["kind"] == "AdaBoundW")
        _BIG[kind] = (st, g, ref)
    return _BIG[kind]


@pytest.mark.parametrize("n", [1, 257, 1000, FLAT])
@pytest.mark.parametrize("kind", list(KINDS))
def test_sizes_up_to_the_flat_buffer(kind, n):
    name, t = KINDS[kind]
    st0, g, ref = _big(kind)
    st = {k: x[:n].to(DEV) for k, x in st0.items()}
    _launch(name, st, g[:n].to(DEV), t)
    for key, got in st.items():
        np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref[key][:n].numpy(), rtol=1e-6, atol=1e-7, err_msg=f"{kind} {key} n={n}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_offset_view_with_an_odd_length(kind):
    """Views 4 bytes past a 16-byte boundary, 1003 elements long: the same values, and nothing written outside them."""
    name, t = KINDS[kind]
    st0, g, ref = _big(kind)
    n, off = 1003, 1
    base = {k: torch.full((n + 8,), 7.0, device=DEV) for k in st0}
    st = {k: b[off:off + n] for k, b in base.items()}
    for k in st:
        st[k].copy_(st0[k][:n])
        assert st[k].data_ptr() % 16 == 4
    gv = torch.zeros(n + 8, device=DEV)[off:off + n]
    gv.copy_(g[:n])
    _launch(name, st, gv, t)
    for key, got in st.items():
        np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref[key][:n].numpy(), rtol=1e-6, atol=1e-7, err_msg=f"{kind} {key}")
        rest = torch.cat([base[key][:off], base[key][off + n:]])
        assert bool((rest == 7.0).all()), f"{kind} {key}: written outside the view"


# ---------------------------------------------------------------------------------------------------- 3. guard flags, 4. loss scale
@pytest.mark.parametrize("kind", list(KINDS))
def test_guard_flags_and_nonfinite_gradients_leave_everything_untouched(kind):
    """A flag of 1.0 or NaN, or an inf / NaN in the gradient counted by ``count_nonfinite`` and handed over as the guard: parameters,
    both moments and the running maximum stay bit-identical; zero flags and a clean gradient step."""
    from miseg_amd import unet_ops
    name, t = KINDS[kind]
    st0, g, _ = _big(kind)
    n = 100_003
    start = {k: x[:n].to(DEV) for k, x in st0.items()}
    grad = g[:n].to(DEV)

    def attempt(guard, gr=grad):
        st = {k: x.clone() for k, x in start.items()}
        _launch(name, st, gr, t, guard=guard)
        return {k: torch.equal(st[k], start[k]) for k in st}

    for flags in ([1.0], [0.0, 0.0, float("nan")], [0.0, -2.0, 0.0]):
        assert all(attempt(torch.tensor(flags, device=DEV)).values()), flags
    assert not any(attempt(torch.zeros(3, device=DEV)).values())
    for poison in (float("inf"), float("-inf"), float("nan")):
        gr = grad.clone()
        gr[5] = gr[n - 7] = poison
        bad = unet_ops.count_nonfinite(gr)
        assert float(bad) == 2.0 and all(attempt(bad, gr).values()), poison
    bad = unet_ops.count_nonfinite(grad)
    assert float(bad) == 0.0 and not any(attempt(bad).values())


@pytest.mark.parametrize("kind", list(KINDS))
def test_power_of_two_loss_scale_gives_the_same_bits(kind):
    """``grad * s`` read with ``grad_scale = s`` (by value), or with -1 and 1 / s in word 4 of the row (a step block's way)."""
    name, t = KINDS[kind]
    st0, g, _ = _big(kind)
    n, s = 4099, 1024.0
    plain = {k: x[:n].to(DEV) for k, x in st0.items()}
    by_value = {k: x.clone() for k, x in plain.items()}
    by_word = {k: x.clone() for k, x in plain.items()}
    grad = g[:n].to(DEV)
    _launch(name, plain, grad, t)
    _launch(name, by_value, grad * s, t, grad_scale=s)
    _launch(name, by_word, grad * s, t, grad_scale=-1.0, hyper_scale=s)
    for k in plain:
        assert torch.equal(plain[k], by_value[k]) and torch.equal(plain[k], by_word[k]), k
    from miseg_amd._cabi import MisegError
    with pytest.raises(MisegError, match="grad_scale"):
        _launch(name, plain, grad, t, grad_scale=0.0)


def test_step_block_carries_seven_values_per_row():
    """``StepIO.stage`` / ``hyper``: words 0-3 and 5-7 are the row's, word 4 stays 1 / loss scale; a four-value row (Adam's) reads as before."""
    from miseg_amd import _cabi, stepio
    io = stepio.StepIO(DEV)
    io.begin([], [[1.0, 2.0, 3.0, 4.0], [1.5, 2.5, 3.5, 4.5, 5.5], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]], scale=8.0)
    torch.cuda.synchronize()
    assert io.hyper(0).tolist() == [1.0, 2.0, 3.0, 4.0, 0.125, 0.0, 0.0, 0.0]
    assert io.hyper(1).tolist() == [1.5, 2.5, 3.5, 4.5, 0.125, 5.5, 0.0, 0.0]
    assert io.hyper(2).tolist() == [1.0, 2.0, 3.0, 4.0, 0.125, 5.0, 6.0, 7.0]
    with pytest.raises(_cabi.MisegError):
        io.stage([], [[0.0] * 8])


# ---------------------------------------------------------------------------------------------------- the optimiser classes by themselves
def _optimiser(name, params):
    from deepclustering2 import optim
    cfg = {**R.RADAM_CASES, **R.ADABOUND_CASES}[name]
    return optim.__dict__[cfg.get("kind", "RAdam")](params, **R.ctor_args(cfg)), cfg


@pytest.mark.parametrize("name", ["radam/b999_wd1e-2", "adabound/wd1e-2_ams", "adaboundw/wd1e-2_ams_lr"])
def test_optimiser_step_reaches_the_recorded_state(inputs, references, name):
    """``step()`` (host scalars -> device row -> launch, outside a step block) on two parameters that together hold the recorded one,
    with the learning rate moved between steps as a scheduler moves it: step 8 within twice the float32 restatement's error."""
    p0, grads = inputs
    ref64, ref32 = references[name]
    a, b = torch.nn.Parameter(p0[:600].to(DEV)), torch.nn.Parameter(p0[600:].to(DEV))
    opt, cfg = _optimiser(name, [a, b])
    for t, g in enumerate(grads, 1):
        opt.param_groups[0]["lr"] = R.lr_of(cfg, t)
        opt.zero_grad()
        a.grad, b.grad = g[:600].to(DEV), g[600:].to(DEV)
        opt.step()
    want = ref64[-1]["p"].numpy()
    own = float(np.abs(ref32[-1]["p"].numpy().astype(np.float64) - want).max())
    have = torch.cat([a.detach(), b.detach()]).cpu().numpy().astype(np.float64)
    assert float(np.abs(have - want).max()) <= 2 * own
    assert opt.state_dict()["state"][1]["step"] == R.STEPS


@pytest.mark.parametrize("name", ["radam/b999_wd1e-2", "adabound/wd1e-2_ams", "adaboundw/wd1e-2"])
def test_checkpoint_round_trip_gives_the_same_next_step(inputs, name):
    """Six steps, ``state_dict()`` into a fresh optimiser over copies of the parameters, the seventh step on both: the same bits."""
    p0, grads = inputs

    def params(src=None):
        src = [p0[:600], p0[600:]] if src is None else src
        return [torch.nn.Parameter(x.detach().clone().to(DEV)) for x in src]

    def step(opt, ps, g):
        opt.zero_grad()
        ps[0].grad, ps[1].grad = g[:600].to(DEV), g[600:].to(DEV)
        opt.step()

    ps = params()
    opt, _ = _optimiser(name, ps)
    for g in grads[:6]:
        step(opt, ps, g)
    sd = opt.state_dict()
    ps2 = params(ps)
    opt2, _ = _optimiser(name, ps2)
    opt2.load_state_dict(sd)
    assert opt2._steps == [6]
    step(opt, ps, grads[6])
    step(opt2, ps2, grads[6])
    for x, y in zip(ps, ps2):
        assert torch.equal(x, y)
    for x, y in ((opt._m[0], opt2._m[0]), (opt._v[0], opt2._v[0])) + (((opt._vmax[0], opt2._vmax[0]),) if "ams" in name else ()):
        assert torch.equal(x, y)
    assert opt.state_dict()["state"].keys() == opt2.state_dict()["state"].keys()


# ---------------------------------------------------------------------------------------------------- 5. inside the train step
def _optim(kind, params, lr=1e-3):
    from deepclustering2 import optim
    if kind == "RAdam":
        return optim.RAdam(params, lr=lr, weight_decay=1e-5)
    return optim.__dict__[kind](params, lr=lr, weight_decay=1e-5, final_lr=2e-3, gamma=0.5, amsbound=True)


def _build(trainer, kind, dtype):
    """The smoke shape (LB = UB = 2, 64 x 64, 4 classes) of ``partial`` / ``udaiic`` / ``meanteacher`` with the optimiser ``kind``."""
    from itertools import chain
    from contrastyou.arch import UNet
    from deepclustering2.loss import KL_div
    from semi_seg import epocher as E
    from semi_seg._utils import IICLossWrapper, ProjectorWrapper
    from semi_seg.synthetic import SyntheticPairs
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4, compute_dtype=dtype).to(DEV)
    lab, unl = iter(SyntheticPairs(2, 64, 4, seed=0, device=DEV)), iter(SyntheticPairs(2, 64, 4, seed=1, device=DEV))
    common = dict(num_batches=1, cur_epoch=0, device=DEV, feature_position=FEATURES, feature_importance=[0.5, 0.25, 0.25])
    if trainer == "udaiic":
        pw = ProjectorWrapper()
        pw.init_encoder(feature_names=FEATURES, num_clusters=20, num_subheads=5, head_types="linear", normalize=False)
        pw.init_decoder(feature_names=FEATURES, num_clusters=20, num_subheads=5, head_types="linear", normalize=False)
        pw = pw.to(DEV)
        opt = _optim(kind, chain(model.parameters(), pw.parameters()))
        lw = IICLossWrapper(feature_names=FEATURES, paddings=[1, 3], patch_sizes=1024)
        return E.UDAIICEpocher(model, pw, opt, lab, unl, KL_div(verbose=False), torch.nn.MSELoss(), lw, cons_weight=5.0, iic_weight=0.1,
                               **common), opt
    opt = _optim(kind, model.parameters())
    if trainer == "meanteacher":
        from deepclustering2.models import ema_updater
        teacher = UNet(input_dim=1, num_classes=4, compute_dtype=dtype).to(DEV)
        for p in teacher.parameters():
            p.detach_().requires_grad_(False)
        upd = ema_updater(alpha=0.999, justify_alpha=True, weight_decay=1e-6)
        ep = E.MeanTeacherEpocher(model, teacher, opt, lab, unl, KL_div(verbose=False), torch.nn.MSELoss(), 10.0, ema_updater=upd, **common)
        return ep, opt
    return E.TrainEpocher(model, opt, lab, unl, KL_div(verbose=False), 0, **common), opt


def _run_steps(trainer, kind, dtype, tape, steps=8):
    def build():
        random.seed(7)
        return _build(trainer, kind, dtype)

    def extra(built):
        opt = built[1]
        return {"steps": list(opt._steps), **({} if kind == "RAdam" else {"vmax": opt._vmax[0].detach().clone()})}

    return th.run_steps(build, steps, tape, mi_precision="fp32" if dtype == "float32" else "f16f8", extra_state=extra)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("kind", ["RAdam", "AdaBound"])
@pytest.mark.parametrize("trainer", ["partial", "udaiic"])
def test_launch_tape_equals_eager_iterations_across_step_six(trainer, kind, dtype):
    """2 eager + 1 recorded + 5 replayed iterations against 8 eager ones, bit for bit: parameters, moments, running maximum, meters.
    The tape is recorded at step 3, where RAdam is not yet rectified, and replayed through steps 6-8, where it is: the step's scalars
    must come from the step block, not from the recorded call."""
    got, info = _run_steps(trainer, kind, dtype, True)
    ref, _ = _run_steps(trainer, kind, dtype, False)
    th.assert_replayed(info, 5)
    names = info.op_names
    assert names.count("miseg_radam_step" if kind == "RAdam" else "miseg_adabound_step") == 1 and "miseg_adam_step_guarded" not in names
    assert got["steps"] == ref["steps"] == [8]
    th.assert_same_state(got, ref, ("param", "m", "v", "meters") + (() if kind == "RAdam" else ("vmax",)))
    assert float(ref["m"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 6. Mean Teacher, 7. fp16 storage
def test_meanteacher_with_radam_guards_the_ema_with_the_same_flags(monkeypatch):
    import bench
    from miseg_amd import unet_ops
    seen = {"radam": [], "ema": []}
    real_radam, real_ema = unet_ops.radam_step, unet_ops.ema_update

    def spy_radam(*a):
        seen["radam"].append(a[-1])
        return real_radam(*a)

    def spy_ema(teacher, student, coef, guard=None):
        seen["ema"].append(guard)
        return real_ema(teacher, student, coef, guard)

    monkeypatch.setattr(unet_ops, "radam_step", spy_radam)
    monkeypatch.setattr(unet_ops, "ema_update", spy_ema)
    ep, opt = _build("meanteacher", "RAdam", "float32")
    ep._TAPE_DEFAULT = False
    student0 = [p.detach().clone() for p in ep._model.parameters()]
    teacher0 = [p.detach().clone() for p in ep._teacher_model.parameters()]
    drv = bench.StepDriver(ep)
    for _ in range(2):
        drv.step()
    drv.close()
    assert len(seen["radam"]) == len(seen["ema"]) == 2 and opt._steps == [2]
    for a, b in zip(seen["radam"], seen["ema"]):
        assert a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.numel() == b.numel() > 0
    assert any(not torch.equal(x, p) for x, p in zip(student0, ep._model.parameters()))
    assert any(not torch.equal(x, p) for x, p in zip(teacher0, ep._teacher_model.parameters()))


def test_fp16_overflow_with_radam_skips_the_update_and_takes_the_step_back(monkeypatch):
    """IEEE-half storage with an absurd loss scale (2^40): every iteration's gradient overflows, the count guards the RAdam launch --
    no weight, no moment moves --, the scale halves and ``step_skipped`` keeps the step counter at the applied updates: none."""
    import bench
    monkeypatch.setenv("MISEG_LOSS_SCALE", repr(2.0 ** 40))
    from miseg_amd import ops
    ops.set_mi_precision("f16f8")
    try:
        ep, opt = _build("udaiic", "RAdam", "float16")
        ep._TAPE_DEFAULT = False
        opt.flat.ensure()
        before = opt.flat.flat_param.detach().clone()
        drv = bench.StepDriver(ep)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(3):
                drv.step()
            drv.close()
        sc = opt.loss_scaler
        assert sc is not None and sc.overflows == 3 and sc.scale == 2.0 ** 38, (sc.overflows, sc.scale)
        assert any("overflow" in str(w.message) for w in caught)
        assert torch.equal(opt.flat.flat_param.detach(), before) and opt._steps == [0]
        assert float(opt._m[0].abs().max()) == 0 and float(opt._v[0].abs().max()) == 0
    finally:
        ops.set_mi_precision("fp32")
