"""GPU: the Mean Teacher trainer (``Trainer.name=meanteacher``, ref contrastyou/epocher/base_epocher.py:129-216) -- the EMA kernel
against torch's eager update, the step under the launch tape, resume, evaluation of the teacher, the step block's accumulator room,
the packed-weight cache with two networks, two data-parallel ranks and the CLI."""
import gc
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import synth
import trainer_harness as th
from oracle import unet as OU
from trainer_harness import DEV, FEATURES, PKG, ROOT

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MT = dict(H=64, LB=2, UB=2, lr=1e-3, wd=1e-5, weight=10.0, alpha=0.999, ema_wd=1e-6)


def build(dtype="float32", num_batches=3, reg="mse"):
    """Student and teacher from different seeded states, the trainer's optimiser / updater, synthetic device loaders."""
    from deepclustering2.loss import KL_div
    from deepclustering2.models import ema_updater
    from deepclustering2.optim import Adam
    from semi_seg.epocher import MeanTeacherEpocher
    from semi_seg.synthetic import SyntheticPairs
    model, teacher = th.unet(dtype, 31), th.unet(dtype, 32)
    for p in teacher.parameters():
        p.detach_().requires_grad_(False)
    opt = Adam(model.parameters(), lr=MT["lr"], weight_decay=MT["wd"])
    upd = ema_updater(alpha=MT["alpha"], justify_alpha=True, weight_decay=MT["ema_wd"])
    lab = SyntheticPairs(MT["LB"], MT["H"], 4, seed=0, device=DEV)
    unl = SyntheticPairs(MT["UB"], MT["H"], 4, seed=1, device=DEV)
    crit = torch.nn.MSELoss() if reg == "mse" else KL_div(verbose=False)
    ep = MeanTeacherEpocher(model, teacher, opt, iter(lab), iter(unl), KL_div(verbose=False), crit, MT["weight"], num_batches, 0, DEV,
                            feature_position=FEATURES, feature_importance=th.IMPORTANCE, ema_updater=upd)
    return ep, model, teacher, opt, upd


def _teacher_state(built):
    ep, model, teacher, opt, upd = built
    return {"teacher": upd._mirror.flat_param.detach().clone(), "teacher_bn": [b.detach().clone() for b in teacher.buffers()]}


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def test_ema_kernel_is_bit_equal_to_torch_eager_update():
    """Several calls of the updater's schedule (ramp, then the capped alpha, weight decay on) over random flat buffers: the kernel
    equals torch's ``t.mul_(a).add_(s, alpha=1 - a).mul_(1 - wd)`` on this device bit for bit; a set guard flag changes nothing."""
    from deepclustering2.models import ema_updater
    from miseg_amd import unet_ops
    g = torch.Generator().manual_seed(0)
    n = 2_161_092          # not a multiple of 4: the scalar tail too
    t0 = torch.randn(n + 3, generator=g)[:n].to(DEV)
    t_ref, t_k = t0.clone(), torch.empty(n + 4, device=DEV)[:n]
    t_k.copy_(t0)
    upd = ema_updater(alpha=0.9, justify_alpha=True, weight_decay=1e-4)
    for k in range(14):                      # alpha 0, 1/2, 2/3, ... then 0.9
        s = torch.randn(n, generator=g).to(DEV)
        a, b, d = upd.host_step()
        t_ref.mul_(a).add_(s, alpha=b).mul_(d)
        coef = torch.tensor([a, b, d], dtype=torch.float32, device=DEV)
        unet_ops.ema_update(t_k, s, coef)
        assert torch.equal(t_k, t_ref), (k, a, int((t_k != t_ref).sum()))
    before = t_k.clone()
    guard = torch.tensor([0.0, 1.0], device=DEV)
    unet_ops.ema_update(t_k, s, coef, guard)
    assert torch.equal(t_k, before)
    unet_ops.ema_update(t_k, s, coef, torch.tensor([float("nan")], device=DEV))
    assert torch.equal(t_k, before)
    unet_ops.ema_update(t_k, s, coef, torch.zeros(3, device=DEV))
    t_ref.mul_(a).add_(s, alpha=b).mul_(d)
    assert torch.equal(t_k, t_ref)


def test_ema_updater_call_matches_the_wheels_loop():
    """``ema_updater(teacher, student)`` on two networks: the wheel's per-tensor loop on copies, in torch on this device, bit-equal."""
    from deepclustering2.models import ema_updater
    student, teacher = th.unet("float32", 3), th.unet("float32", 4)
    ref = {k: v.clone() for k, v in teacher.state_dict().items()}
    upd = ema_updater(alpha=0.99, justify_alpha=True, weight_decay=1e-6)
    names = [n for n, _ in teacher.named_parameters()]
    for k in range(3):
        with torch.no_grad():
            for p in student.parameters():
                p.add_(0.01 * torch.randn_like(p))
        alpha = min(1 - 1 / (k + 1), 0.99)
        sd = dict(student.named_parameters())
        for n in names:
            ref[n].mul_(alpha).add_(sd[n].detach(), alpha=1 - alpha).mul_(1 - 1e-6)
        upd(teacher, student)
    got = teacher.state_dict()
    for n in names:
        assert torch.equal(got[n], ref[n]), n
    assert upd.state_dict()["global_step"] == 3


# ---------------------------------------------------------------------------------------------------------------- 3. the tape
def _run_steps(dtype, tape, steps=7):
    return th.run_steps(lambda: build(dtype), steps, tape, mi_precision="fp32" if dtype == "float32" else "f16f8",
                        extra_state=_teacher_state)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_meanteacher_tape_replay_equals_eager_steps(dtype):
    """7 iterations, alpha changing every one: 2 eager + 1 recorded + 4 replayed iterations give the student, Adam's moments, the
    teacher's flat buffer and BatchNorm buffers and the meters of 7 eager iterations, bit for bit.  The recorded iteration has one
    EMA launch and packs the teacher's weights in the student's single pack launch."""
    got, info = _run_steps(dtype, True)
    ref, _ = _run_steps(dtype, False)
    th.assert_replayed(info, 4)
    names = info.op_names
    assert names.count("miseg_ema_update") == 1 and names.count("miseg_cat_flipped") == 1, names
    assert "miseg_pack_conv3x3_weights" not in names and names.count("miseg_pack_conv3x3_weights_multi") <= 1, names
    th.assert_same_state(got, ref, ("param", "m", "v", "teacher", "teacher_bn", "meters"))


# ---------------------------------------------------------------------------------------------------------------- 4. resume
def _trainer(save_dir, max_epoch):
    sys.path.insert(0, PKG)
    from semi_seg.main import build_trainer
    return build_trainer(["Trainer.name=meanteacher", f"Trainer.save_dir={save_dir}", "Trainer.device=cuda", f"Trainer.max_epoch={max_epoch}",
                          "Trainer.num_batches=1", "Data.size=64", "Data.name=synthetic", "LabeledData.batch_size=2",
                          "UnlabeledData.batch_size=2", "Optim.lr=0.001"])


def test_resume_continues_the_ema_schedule(tmp_path):
    """2 steps, checkpoint, a new trainer loads it and takes 1 step: bit-equal to 3 uninterrupted steps (the call count travels in the
    checkpoint, so alpha continues; the reference's stateless updater would snap the teacher back to the student)."""
    os.environ["MISEG_PROGRESS"] = "0"

    def run(tr, n):
        tr.to(tr._device)
        for _ in range(n):
            tr._run_epoch()
            tr._cur_epoch += 1
        torch.cuda.synchronize()

    save = f"pytest_mt_resume_{os.getpid()}"
    run_dir = os.path.join(PKG, "semi_seg", "runs", save)
    try:
        random.seed(5)
        a = _trainer(save, 3)
        run(a, 3)
        full = (a._optimizer.flat.flat_param.detach().clone(), a._ema_updater._mirror.flat_param.detach().clone())
        random.seed(5)
        b = _trainer(save + "_b", 3)
        run(b, 2)
        ck = tmp_path / "mid.pth"
        torch.save(b.state_dict(), ck)
        sd = torch.load(ck, map_location="cpu", weights_only=False)
        assert "_teacher_model" in sd and "_ema_updater" in sd and sd["_ema_updater"]["global_step"] == 2
        state = random.getstate()
        c = _trainer(save + "_c", 3)
        c.load_state_dict(sd)
        c._cur_epoch = 2
        c._labeled_loader, c._unlabeled_loader = b._labeled_loader, b._unlabeled_loader      # the loaders' position travels with them
        random.setstate(state)
        run(c, 1)
        assert c._ema_updater.global_step == 3
        assert torch.equal(c._optimizer.flat.flat_param, full[0])
        assert torch.equal(c._ema_updater._mirror.flat_param, full[1])
    finally:
        for s in (save, save + "_b", save + "_c"):
            shutil.rmtree(os.path.join(PKG, "semi_seg", "runs", s), ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- 5. evaluation
def test_evaluation_reports_the_teacher():
    """``eval_epoch`` / ``inference()`` evaluate the teacher (ref contrast_trainer.py:261): equal to EvalEpocher(teacher), different
    from the student's Dice when the two networks differ."""
    from deepclustering2.loss import KL_div
    from semi_seg.epocher import EvalEpocher
    os.environ["MISEG_PROGRESS"] = "0"
    save = f"pytest_mt_eval_{os.getpid()}"
    try:
        tr = _trainer(save, 1)
        tr.to(tr._device)
        tr._teacher_model.load_state_dict(OU.init_state(1, 4, seed=77))
        with torch.no_grad():
            _, got = tr._eval_epoch(loader=tr._val_loader)
            _, teacher = EvalEpocher(tr._teacher_model, tr._val_loader, KL_div(), device=tr._device).run()
            _, student = EvalEpocher(tr._model, tr._val_loader, KL_div(), device=tr._device).run()
            _, teacher_test = EvalEpocher(tr._teacher_model, tr._test_loader, KL_div(), device=tr._device).run()
        assert got == teacher and teacher != student, (got, teacher, student)
        tr.save(got)
        _, score = tr.inference()            # on the test loader
        assert score == teacher_test, (score, teacher_test)
    finally:
        shutil.rmtree(os.path.join(PKG, "semi_seg", "runs", save), ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- 6. accumulator room
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_training_forward_with_an_exhausted_accumulator_block(dtype):
    """A training forward inside an iteration whose step block has no accumulator room left (the third forward of an iteration):
    every layer, the stem included, must take a path that computes its batch statistics -- same running statistics and output as a
    forward with room.  At the parent the stem ran with no accumulator and read its statistics from uninitialised memory."""
    from miseg_amd import stepio
    x = T(synth.uniform("mt/acc/x", (2, 1, 64, 64))).to(DEV)
    outs = []
    for exhausted in (False, True):
        net = th.unet(dtype, 41).train()
        io = stepio.StepIO(DEV)
        io.upload(io.stage([], []))
        if exhausted:
            io._cursor_acc = io.acc_cap
        stepio.CURRENT = io
        try:
            with torch.no_grad():
                y = net(x).float()
        finally:
            stepio.CURRENT = None
        torch.cuda.synchronize()
        outs.append((y, [b.detach().clone() for n, b in net.named_buffers() if "running" in n]))
    (y0, b0), (y1, b1) = outs
    assert torch.isfinite(y1).all()
    for u, v in zip(b0, b1):
        torch.testing.assert_close(v, u, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(y1, y0, rtol=2e-2 if dtype == "bfloat16" else 1e-3, atol=2e-2 if dtype == "bfloat16" else 1e-3)


def test_meanteacher_block_has_room_for_both_forwards():
    """The Mean Teacher's step block holds both training forwards' accumulators; the udaiic block is the shipped size."""
    from miseg_amd import stepio
    ep, *_ = build("float32", num_batches=1)
    ep.run()
    assert ep._io.param_bytes == stepio.block_bytes(2) > stepio.PARAM_BYTES
    assert 3468 * 2 <= ep._io._cursor_acc <= ep._io.acc_cap, ep._io._cursor_acc


# ---------------------------------------------------------------------------------------------------------------- 7. pack cache
def test_freeing_a_registered_network_rerecords_the_tape():
    """Two networks' weights in the packed-weight cache, a tape recorded over one of them; freeing the other bumps
    ``PACK_CACHE.generation`` at once, the next step drops the tape (its job table named the freed weights) and a later one records
    a new tape that replays."""
    import bench
    from miseg_amd import packcache
    from miseg_amd.flat import FlatBuffers
    ep, model, teacher, opt, upd = build("float32")
    other = th.unet("float32", 51).train()
    fb = FlatBuffers(list(other.parameters()))
    fb.ensure()
    with torch.no_grad():
        other(T(synth.uniform("mt/pack/x", (2, 1, 64, 64))).to(DEV))     # its weights now sit in the cache
    ep._TAPE_DEFAULT = False
    drv = bench.StepDriver(ep)
    ep.enable_step_tape(warmup=2)
    random.seed(3)
    for _ in range(4):
        drv.step()
    tp = ep._step_tape
    assert tp.handle and tp.replays == 1, (tp.handle, tp.replays, tp.disabled)
    gen = packcache.PACK_CACHE.generation
    del other, fb
    gc.collect()
    assert packcache.PACK_CACHE.generation != gen
    drv.step()
    assert tp.replays == 1 and not tp.handle          # released, not replayed
    for _ in range(4):
        drv.step()
    drv.close()
    assert tp.handle and tp.replays >= 1 and tp.disabled is None, (tp.handle, tp.replays, tp.disabled)
    ep.disable_step_tape()


# ---------------------------------------------------------------------------------------------------------------- 8. two ranks
def test_two_ranks_keep_identical_teachers(tmp_path):
    """Two processes on the one GPU over gloo: the teacher is broadcast from rank 0 at attach, and after 3 steps the teachers' flat
    buffers are bit-equal across ranks (each rank trains on its own data; the student is all-reduced)."""
    worker = os.path.join(ROOT, "tests", "_meanteacher_ddp_worker.py")
    base = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    port = 34500 + os.getpid() % 2000
    procs = []
    for r in range(2):
        env = dict(base, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MISEG_DDP_BACKEND="gloo", MISEG_PROGRESS="0")
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path / f"r{r}.pt"), f"pytest_mt_ddp_{os.getpid()}_{r}"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt") for r in range(2))
    assert r0["steps"] == r1["steps"] == 3
    assert torch.equal(r0["student"], r1["student"])
    assert torch.equal(r0["teacher"], r1["teacher"])
    assert not torch.equal(r0["teacher"], r0["teacher_init"])


# ---------------------------------------------------------------------------------------------------------------- 9. the CLI
def test_main_cli_runs_meanteacher():
    """``python semi_seg/main.py Trainer.name=meanteacher``: one tiny synthetic epoch; the checkpoint holds the teacher and the
    updater."""
    save = f"pytest_cli_meanteacher_{os.getpid()}"
    run_dir = th.run_dir(save)
    shutil.rmtree(run_dir, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=meanteacher", f"Trainer.save_dir={save}", "Trainer.device=cuda", "Trainer.max_epoch=1",
                     "Trainer.num_batches=5", "Data.size=64", "LabeledData.batch_size=2", "UnlabeledData.batch_size=2",
                     "Arch.compute_dtype=bfloat16"])
        sd = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert "_teacher_model" in sd and "_ema_updater" in sd and sd["_ema_updater"]["global_step"] == 5
        assert set(sd["_teacher_model"]) == set(sd["_model"])
        assert any(not torch.equal(sd["_teacher_model"][k], sd["_model"][k]) for k in sd["_model"] if "weight" in k)
    finally:
        shutil.rmtree(run_dir, ignore_errors=True)


# ---------------------------------------------------------------------------------------------------------------- 2. vs the reference
def _golden_run(g, dtype, monkeypatch):
    """The golden's 3 iterations through MeanTeacherEpocher: same initial states, batches and flip seeds as the reference run."""
    from deepclustering2.loss import KL_div
    from deepclustering2.models import ema_updater
    from deepclustering2.optim import Adam
    from semi_seg import epocher as E
    cfg = th.golden_cfg(g)
    H, LB, NB = int(cfg["H"]), int(cfg["LB"]), int(cfg["NB"])
    model, teacher = th.unet(dtype, int(cfg["student_seed"])), th.unet(dtype, int(cfg["teacher_seed"]))
    for p in teacher.parameters():
        p.detach_().requires_grad_(False)
    opt = Adam(model.parameters(), lr=float(cfg["lr"]), weight_decay=float(cfg["wd"]))
    upd = ema_updater(alpha=float(cfg["alpha"]), justify_alpha=True, weight_decay=float(cfg["ema_wd"]))
    batches = [(T(synth.uniform(f"mt/lab{i}", (LB, 1, H, H))), T(synth.integers(f"mt/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]

    def loader():
        return th.reference_batches([a for a, _ in batches], [b for _, b in batches], LB)

    th.replay_seeds(monkeypatch, g["seeds"])
    teachers, real_apply = [], upd.apply

    def apply_spy(*a, **k):
        real_apply(*a, **k)
        teachers.append(upd._mirror.flat_param.detach().clone())

    upd.apply = apply_spy
    with th.adam_gradients(monkeypatch) as grads:
        ep = E.MeanTeacherEpocher(model, teacher, opt, loader(), loader(), KL_div(verbose=False), torch.nn.MSELoss(), float(cfg["weight"]),
                                  NB, 0, DEV, feature_position=FEATURES, feature_importance=th.IMPORTANCE, ema_updater=upd)
        ep._TAPE_DEFAULT = False
        per_step = th.keep_records(ep)
        res = ep.run()
    return res, grads[0].cpu(), teachers, per_step, opt, upd, teacher


def test_epocher_matches_the_reference_run(golden, monkeypatch):
    """fp32, 3 iterations against the reference's own MeanTeacherEpocher with the wheel's updater (tests/golden/meanteacher.npz):
    step-1 gradients at the first-iteration bounds of test_gpu_step, per-step losses, the teacher after the first and last EMA and
    its running statistics, the meter names (the reference's ``ds`` is ``sup_dice`` here, as in every epocher of semi_seg)."""
    g = golden("meanteacher")
    res, grad, teachers, per_step, opt, upd, teacher = _golden_run(g, "float32", monkeypatch)
    named = dict(zip((str(n) for n in g["param_names"]), opt.flat.given))
    assert len(named) == len(opt.flat.given)
    # 1. step-1 gradients
    worst = th.sampled_rel_l2(g, "grad_step1", grad, named, opt.flat.offset_of)
    assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
    tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
    assert tail[len(tail) // 2] < 5e-3 and tail[-1] < 1.5e-2, tail
    assert max(worst.values()) < 3e-2, worst
    # 2. per-step losses
    assert len(per_step) == 3
    np.testing.assert_allclose(per_step[0]["sup_loss"], g["sup_loss"][0], rtol=2e-5)
    np.testing.assert_allclose(per_step[0]["reg_loss"], g["reg_loss"][0], rtol=2e-4)
    np.testing.assert_allclose([s["sup_loss"] for s in per_step], g["sup_loss"], rtol=3e-3)
    np.testing.assert_allclose([s["reg_loss"] for s in per_step], g["reg_loss"], rtol=2e-2)
    # 3. the teacher after the first (alpha 0: a copy of the student) and the last EMA: Adam's first steps move near-zero gradients' signs
    # by 2 lr, so the bound is in units of lr
    mirror = upd._mirror
    for p in opt.flat.given:
        assert mirror.offsets[[id(q) for q in opt.flat.params].index(id(p))] == opt.flat.offset_of(p)
    for i, flat in ((1, teachers[0]), (3, teachers[2])):
        for n, d in th.sampled_max_abs(g, f"teacher{i}", flat, named, opt.flat.offset_of).items():
            assert d <= 2.5e-3 * i, (i, n, d)
    errs = {}
    for n, b in teacher.named_buffers():
        if "running" in n:
            got, ref = th.sampled(b, 0, b.numel(), f"teacher3/{n}"), synth.fp_unpack(g, f"teacher3/{n}")["sample"]
            errs[n] = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))
    # measured: relative L2 1.5e-4 (Conv1) .. 1.4e-2 (Up5, behind the most ReLUs): the teacher's weights carry Adam's sign flips
    assert max(errs.values()) < 2e-2, errs
    # 4. meters
    ref_keys = [str(k).replace("ds/", "sup_dice/") for k in g["meter_keys"]]
    got = th.meter_items(res)
    assert sorted(got) == sorted(ref_keys), (sorted(got), sorted(ref_keys))
    ref = dict(zip(ref_keys, (float(v) for v in g["meter_values"])))
    assert got["reg_weight/mean"] == ref["reg_weight/mean"] == 10.0
    np.testing.assert_allclose(got["sup_loss/mean"], ref["sup_loss/mean"], rtol=3e-3)
    np.testing.assert_allclose(got["reg_loss/mean"], ref["reg_loss/mean"], rtol=2e-2)


def test_bf16_run_tracks_the_fp32_reference(golden, monkeypatch):
    g = golden("meanteacher")
    res, *_ = _golden_run(g, "bfloat16", monkeypatch)
    np.testing.assert_allclose(res["sup_loss"]["mean"], np.mean(g["sup_loss"]), rtol=2e-2)
    np.testing.assert_allclose(res["reg_loss"]["mean"], np.mean(g["reg_loss"]), rtol=0.25)
