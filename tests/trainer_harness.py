"""What every trainer's tests share: the golden run's scaffolding, the comparison against a fixture's fingerprints, the launch-tape
parity run, the command-line run and the ``MISEG_ERROR_DUMP`` writer.

A plain module, imported the way ``tape_harness`` is.  It imports without a device and without the built library: ``miseg_amd``,
``semi_seg``, ``bench`` and ``contrastyou`` are imported inside the functions that need them.

No bound lives here.  The comparison functions return errors and the test that calls them keeps its own literal bounds; the two
functions that assert (``assert_replayed``, ``assert_same_state``) take the expected count and the keys as arguments without defaults.
"""
import contextlib
import json
import os
import random
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np

import synth

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
FEATURES = ["Conv5", "Up_conv3", "Up_conv2"]
IMPORTANCE = [0.5, 0.25, 0.25]


def error_dump(prefix, tag, rows, sort_keys=False):
    """With MISEG_ERROR_DUMP=<dir>, the achieved errors are written there as ``<prefix>_<tag>.json`` (the numbers DESIGN.md quotes)."""
    out = os.environ.get("MISEG_ERROR_DUMP")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"{prefix}_{tag}.json"), "w") as f:
        json.dump(rows, f, indent=1, sort_keys=sort_keys)


# ---------------------------------------------------------------------------------------------------------------- the golden run
def unet(dtype, seed):
    """The 1-channel, 4-class U-Net from the oracle's seeded initial state, on the device."""
    from contrastyou.arch import UNet
    from oracle import unet as OU
    m = UNet(1, 4, compute_dtype=dtype)
    m.load_state_dict(OU.init_state(1, 4, seed=seed))
    return m.to(DEV)


def golden_cfg(g):
    """The fixture's ``cfg/*`` entries as Python scalars."""
    return {k[4:]: g[k].item() for k in g.files if k.startswith("cfg/")}


def reference_batches(images, targets, batch):
    """The reference loaders' nested structure, one item per (image, target): two views (the second an independent clone), the slice
    names, the partitions and the patient groups."""
    for img, tgt in zip(images, targets):
        yield [[[img, tgt], [img.clone(), tgt.clone()]], [f"patient{j:03d}_00_{j}" for j in range(batch)], ["0"] * batch,
               [f"patient{j:03d}_00" for j in range(batch)]]


def replay_seeds(monkeypatch, seeds):
    """``semi_seg.epocher.random.randint`` hands out the fixture's flip seeds, in order."""
    from semi_seg import epocher as E
    it = iter(int(s) for s in seeds)
    monkeypatch.setattr(E.random, "randint", lambda a, b: next(it))


@contextlib.contextmanager
def adam_gradients(monkeypatch):
    """Yields the list that receives a clone of the flat gradient of every ``unet_ops.adam_step`` call made inside the block.  Patched
    at that address (``flat`` looks it up there at call time) and put back on the way out."""
    from miseg_amd import unet_ops
    grads, real = [], unet_ops.adam_step

    def spy(param, grad, *a, **k):
        grads.append(grad.detach().clone())
        return real(param, grad, *a, **k)

    monkeypatch.setattr(unet_ops, "adam_step", spy)
    try:
        yield grads
    finally:
        monkeypatch.setattr(unet_ops, "adam_step", real)


def keep_records(ep):
    """Wraps ``ep._record``; returns the list that receives a copy of each step's host dict."""
    per_step, record = [], ep._record

    def keep(host, *a):
        per_step.append(dict(host))
        record(host, *a)

    ep._record = keep
    return per_step


# ---------------------------------------------------------------------------------------------------------------- against a fixture
def sampled(flat, offset, numel, tag):
    """``flat[offset:offset + numel]`` as float64 at ``synth.sample_index(numel, tag)``: what a fingerprint's ``sample`` holds."""
    part = flat[offset:offset + numel]
    if hasattr(part, "detach"):
        part = part.detach().cpu().numpy()
    return np.asarray(part).reshape(-1).astype(np.float64)[synth.sample_index(numel, tag)]


def _pairs(g, prefix, flat, named, offset_of):
    for n, p in named.items():
        got = sampled(flat, offset_of(p), p.numel(), f"{prefix}/{n}")
        yield n, got, synth.fp_unpack(g, f"{prefix}/{n}")["sample"].astype(np.float64)


def sampled_rel_l2(g, prefix, flat, named, offset_of):
    """{name: relative L2 distance, in float64, of the tensor's sample in ``flat`` from the fingerprint ``<prefix>/<name>``} for every
    ``name: parameter`` of ``named``; ``offset_of(parameter)`` is where the tensor starts in ``flat``."""
    return {n: float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30)) for n, got, ref in _pairs(g, prefix, flat, named, offset_of)}


def sampled_max_abs(g, prefix, flat, named, offset_of):
    """As ``sampled_rel_l2``, the largest absolute distance."""
    return {n: float(np.abs(got - ref).max()) for n, got, ref in _pairs(g, prefix, flat, named, offset_of)}


def meter_items(res):
    """An epocher's result, flattened to {"<meter>/<statistic>": float}."""
    return {f"{k}/{kk}": float(vv) for k, v in res.items() for kk, vv in dict(v).items()}


# ---------------------------------------------------------------------------------------------------------------- tape parity
TapeInfo = namedtuple("TapeInfo", "replays disabled recorded op_names n_ops")


def run_steps(build, steps, tape, mi_precision=None, extra_state=None):
    """``steps`` iterations of the epocher ``build()`` returns (alone or first in a tuple) under ``bench.StepDriver``; with ``tape``:
    2 eager, 1 recorded, the rest replayed.  Returns the state to compare -- the flat parameters, Adam's moments, the meters' repr and
    whatever ``extra_state(built)`` adds -- and the tape's ``TapeInfo`` (None without a tape).  ``mi_precision`` is set before the
    build and put back to fp32 after the run."""
    import bench
    from miseg_amd import ops
    if mi_precision is not None:
        ops.set_mi_precision(mi_precision)
    try:
        built = build()
        ep = built[0] if isinstance(built, tuple) else built
        opt = ep._optimizer
        ep._TAPE_DEFAULT = False
        drv = bench.StepDriver(ep)
        if tape:
            ep.enable_step_tape(warmup=2)
        random.seed(11)
        for _ in range(steps):
            drv.step()
        drv.close()
        tp = ep._step_tape
        info = None if tp is None else TapeInfo(tp.replays, tp.disabled, bool(tp.handle), tp.op_names(), tp.n_ops)
        state = {"param": opt.flat.flat_param.detach().clone(), "m": opt._m[0].detach().clone(), "v": opt._v[0].detach().clone(),
                 "meters": repr(dict(ep.meters.tracking_status()))}
        if extra_state is not None:
            state.update(extra_state(built))
        ep.disable_step_tape()
        return state, info
    finally:
        if mi_precision is not None:
            ops.set_mi_precision("fp32")


def assert_replayed(info, replays):
    """The tape was taken (not refused), holds a recording and was replayed ``replays`` times."""
    assert info is not None and info.disabled is None, f"the tape was refused: {info and info[:3]}"
    assert info.recorded and info.replays == replays, f"expected 2 eager + 1 recorded + {replays} replayed iterations: {info[:3]}"


def assert_same_state(got, ref, keys):
    """``got[k]`` equals ``ref[k]`` bit for bit for every key: tensors, lists of tensors, anything else by ``==``."""
    import torch
    for k in keys:
        a, b = got[k], ref[k]
        if torch.is_tensor(a):
            assert torch.equal(a, b), (k, float((a - b).abs().max()))
        elif isinstance(a, (list, tuple)) and a and torch.is_tensor(a[0]):
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), k
        else:
            assert a == b, (k, a, b)


# ---------------------------------------------------------------------------------------------------------------- the CLI
def run_main(args, timeout=600, code=None, env=None):
    """``python semi_seg/main.py <args>`` -- or ``python -c <code> <args>`` -- in a fresh process from the package directory, ``env``
    added to the environment; the exit status must be 0.  Returns the completed process."""
    head = ["semi_seg/main.py"] if code is None else ["-c", code]
    res = subprocess.run([sys.executable] + head + list(args), cwd=PKG, capture_output=True, text=True, timeout=timeout,
                         env=None if env is None else {**os.environ, **env})
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res


_INFERENCE = ("import os, sys; from semi_seg.main import build_trainer; tr = build_trainer(sys.argv[1:]); "
              "res, score = tr.inference(os.environ['MISEG_TEST_CKPT']); print('inference', repr(float(score)))")


def run_inference(args, checkpoint, timeout=600):
    """``build_trainer(args).inference(checkpoint)`` in a fresh process; returns the score."""
    res = run_main(args, timeout, code=_INFERENCE, env={"MISEG_TEST_CKPT": checkpoint})
    found = re.findall(r"^inference (\S+)$", res.stdout, re.M)
    assert found, res.stdout[-2000:] + res.stderr[-4000:]
    return float(found[-1])


def run_dir(save):
    """Where ``Trainer.save_dir=<save>`` writes."""
    return os.path.join(PKG, "semi_seg", "runs", save)


def checkpoint_tree(path):
    """The checkpoint's key tree, as ``synth.tree_lines`` flattens it."""
    import torch
    return synth.tree_lines(torch.load(path, map_location="cpu", weights_only=False))


def own_lines_removed(lines, prefixes):
    """The tree's lines without those that start with one of the trainer's own ``prefixes``, sorted."""
    return sorted(l for l in lines if not l.startswith(tuple(prefixes)))


# ---------------------------------------------------------------------------------------------------------------- the CPU side
def assert_entry_points(names):
    """Every name is declared in include/miseg_hip.h (returning int or int64_t), known to ``_cabi`` and defined in the built library.
    Returns the header's text and ``nm``'s list of the library's symbols for what a test checks beyond that."""
    from miseg_amd import _cabi
    header = open(os.path.join(ROOT, "include", "miseg_hip.h")).read()
    lib = os.path.join(PKG, "lib", "libmiseg_hip.so")
    assert os.path.exists(lib), "build() makes the library"
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for name in names:
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", header), name
        assert name in _cabi.declared_symbols(), name
        assert re.search(r"\bT " + name + r"$", exported, re.M), name
    return header, exported


def semi_config(argv=()):
    """config/semi.yaml with the command line's overrides."""
    from deepclustering2.configparser import ConfigManger
    return ConfigManger(os.path.join(PKG, "config", "semi.yaml"), verbose=False, argv=list(argv)).config


def bare_trainer(name, cfg):
    """``trainer_zoos[name]`` after ``_init()`` on a fresh U-Net, without a run directory, with what ``_make_epocher`` reads besides
    the trainer's section."""
    from contrastyou.arch import UNet
    from deepclustering2.loss import KL_div
    from semi_seg.trainer import trainer_zoos
    tr = trainer_zoos[name].__new__(trainer_zoos[name])
    tr._config = cfg
    tr._model = UNet(**cfg["Arch"])
    tr._init()
    tr._optimizer, tr._labeled_loader, tr._unlabeled_loader, tr._sup_criterion = None, iter(()), iter(()), KL_div(verbose=False)
    tr._num_batches, tr._cur_epoch, tr._device = 1, 0, "cpu"
    return tr
