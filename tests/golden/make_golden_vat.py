#!/usr/bin/env python
"""Golden vectors of virtual adversarial training (tests/golden/vat.npz) from the WHEEL's own ``VATLoss``
(deepclustering2/utils/VAT.py:32-93), run at generation time.

Run in the build container only (needs the reference tree; see make_golden.py):

    python tests/golden/make_golden_vat.py

The wheel's class draws its initial direction with ``torch.randn_like``; the generator replaces that one call (in the wheel's VAT
module only) with a function that returns the fixed ``d0`` of the case, so that the repository's implementations -- which take
``d0`` as an argument -- can be compared on the same direction.  The model is the reference's ``contrastyou.arch.UNet(1, 4)`` on the
oracle's seeded initialisation, in train mode, wrapped to return ``[softmax(logits)]``: the wheel's class reads ``model(x)[0]`` and
expects a simplex.  float64 throughout.  The wheel's ``adv_distance.backward()`` leaves the direction pass's parameter gradients in
``param.grad``; they are cleared before ``lds.backward()``, so the recorded parameter gradients are those of ``lds`` alone (DESIGN.md
section 23 lists this among the deliberate differences).

Three cases on ``x = synth.uniform('vat/x', [3, 1, 32, 48])``:
  a: ip = 1, eps = 1.0 (float), xi = 10;    b: ip = 2, eps = tensor [0.5, 1.0, 2.0], xi = 10;    c: as b with xi = 0.1.
All: prop_eps = 0.25, ``d0 = synth.normal('vat/d0', ...)``.  Case c is there because the second iteration of case b is ill-conditioned
in float32 at the class's default xi (below): at xi = 0.1 the perturbed point stays close to x, float32 is stable over both iterations and
the second iteration with a tensor ``eps`` is pinned at bounds that can fail.

Recorded per case: ``pred`` (softmax of the clean logits), the direction after the initial normalisation and after each iteration
(captured from ``_l2_normalize``), ``r_adv``, ``lds``, the per-tensor L2 norms of the parameter gradients, two whole small gradient
tensors (``DeConv_1x1.weight``, ``Conv1.conv.1.weight``), and the BatchNorm statistics of ``Conv1.conv.1`` after the call with its
batch counter (one tracked pass).  The weights are not stored: the tests rebuild them from the seed (``cfg/model_seed``).  Only data
is written.

The model seed.  tests/test_gpu_vat.py bounds the kernels' distance from this file by ten times the distance of a float32 evaluation
of tests/vat_ref.py from its float64 evaluation, measured on these inputs.  That measure is only meaningful where float32 itself is
stable: a ReLU that flips between the two precisions moves the direction by far more than rounding does.  The generator takes the first
seed, counting up from ``FIRST_MODEL_SEED``, whose float32 evaluation stays within ``OWN_ERROR_LIMITS`` of the float64 one in both cases;
the criterion looks at the restatement alone.  The measured distances are stored under ``own_error/``.

bf16.  ``own_error_bf16/`` holds the same distances for the restatement with the bf16 kernels' rounding points
(``vat_ref.unet_bf16_rounded``), float32 against float64, at the same model seed.  They are large on EVERY seed: a value that sits
within float32 rounding of a bf16 rounding boundary lands on the other side, a jump of 2^-8 of that value, and on a randomly
initialised network those jumps grow through 22 layers (the clean prediction alone moves by 5e-2; the first direction by 20-50 %).
No seed makes bf16 stable, so none is searched for; the numbers say how little a bf16 comparison of directions can pin."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference, np_, save  # noqa: E402
import synth  # noqa: E402

SHAPE = (3, 1, 32, 48)
CASES = {"a": dict(ip=1, eps=1.0, xi=10.0), "b": dict(ip=2, eps=[0.5, 1.0, 2.0], xi=10.0), "c": dict(ip=2, eps=[0.5, 1.0, 2.0], xi=0.1)}
PROP_EPS = 0.25
FIRST_MODEL_SEED = 7
WHOLE = ("DeConv_1x1.weight", "Conv1.conv.1.weight")
# float32 against float64, tests/vat_ref.py alone (the quantities of ``distances``).  One iteration (case a, and the first of case b)
# is as stable as the forward pass; the SECOND iteration differentiates at x + 10 d1, a perturbation of 0.25 per pixel, where a
# direction that moved by 2e-5 meets other ReLU masks: float32 lands a few per cent from float64 there on every seed tried, and
# the limits of case b only keep out the seeds where it lands tens of per cent away.
OWN_ERROR_LIMITS = {"a": {"pred": 5e-5, "d0": 1e-6, "d1": 1e-3, "r_adv": 1e-3, "lds": 1e-4, "grad_norms": 1e-2, "grad/DeConv_1x1.weight": 1e-3,
                          "grad/Conv1.conv.1.weight": 1e-2},
                    "b": {"pred": 5e-5, "d0": 1e-6, "d1": 1e-3, "d2": 6e-2, "r_adv": 6e-2, "lds": 1e-2, "grad_norms": 0.25,
                          "grad/DeConv_1x1.weight": 0.1, "grad/Conv1.conv.1.weight": 0.25},
                    "c": {"pred": 5e-5, "d0": 1e-6, "d1": 1e-3, "d2": 2e-2, "r_adv": 2e-2, "lds": 1e-3, "grad_norms": 0.25,
                          "grad/DeConv_1x1.weight": 1e-2, "grad/Conv1.conv.1.weight": 0.25}}


def inputs():
    return torch.from_numpy(synth.uniform("vat/x", SHAPE)).double(), torch.from_numpy(synth.normal("vat/d0", SHAPE)).double()


def eps_of(case):
    e = CASES[case]["eps"]
    return torch.tensor(e, dtype=torch.float64) if isinstance(e, list) else float(e)


def import_wheel_vat():
    """``deepclustering2.utils.VAT`` of the wheel.  As shipped the module does not import: it names two modules by the names they had
    before the wheel was cut -- ``..loss.loss`` (now ``loss/kl_losses.py``) and ``..model`` (now ``models/``) -- and builds its default
    distance as ``KL_div(reduce=True)``, a keyword the wheel's ``KL_div`` no longer has (``reduction='mean'``, its default, is what
    it meant).  The two names are aliased to the wheel's own modules; nothing of ``VATLoss`` itself is touched."""
    import types
    import deepclustering2.loss.kl_losses as kl
    if "deepclustering2.loss.loss" not in sys.modules:
        loss = types.ModuleType("deepclustering2.loss.loss")
        loss.KL_div = lambda reduce=True, **kw: kl.KL_div(reduction="mean" if reduce else "none", verbose=False, **kw)
        model = types.ModuleType("deepclustering2.model")
        model.Model = object
        sys.modules["deepclustering2.loss.loss"], sys.modules["deepclustering2.model"] = loss, model
    import deepclustering2.utils.VAT as ref_vat
    return ref_vat


def run_wheel(case: str, model_seed: int) -> dict:
    from contrastyou.arch import UNet
    ref_vat = import_wheel_vat()
    from oracle import unet as OU
    x, d0 = inputs()
    model = UNet(1, 4)
    model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
    model = model.double().train()
    names = [n for n, _ in model.named_parameters()]

    def simplex_model(inp):
        return [model(inp).softmax(1)]

    simplex_model.apply = model.apply            # _disable_tracking_bn_stats walks the modules
    directions, real_norm, real_randn = [], ref_vat._l2_normalize, ref_vat.torch.randn_like

    def spy_normalize(d):
        out = real_norm(d)
        directions.append(out.detach().clone())
        return out

    class _Torch:                                # the wheel's module sees torch with ONE function replaced
        def __getattr__(self, k):
            return (lambda t, **kw: d0.clone()) if k == "randn_like" else getattr(torch, k)

    ref_vat._l2_normalize, saved_torch, ref_vat.torch = spy_normalize, ref_vat.torch, _Torch()
    torch.set_default_dtype(torch.float64)       # the wheel's _l2_normalize compares the norms with a default-dtype torch.ones
    try:
        crit = ref_vat.VATLoss(xi=CASES[case]["xi"], eps=eps_of(case), prop_eps=PROP_EPS, ip=CASES[case]["ip"])
        with torch.no_grad():
            pred = simplex_model(x)[0]
        # (that call moved the running statistics once more than VATLoss itself will: restore the state the tests start from)
        model.load_state_dict(OU.init_state(1, 4, seed=model_seed))
        model.double()
        lds, x_adv, r_adv = crit(simplex_model, x)
        model.zero_grad()
        for p in model.parameters():
            p.grad = None
        lds.backward()
    finally:
        torch.set_default_dtype(torch.float32)
        ref_vat._l2_normalize, ref_vat.torch = real_norm, saved_torch
    assert len(directions) == CASES[case]["ip"] + 1, len(directions)
    sd = model.state_dict()
    return {"pred": pred, "d": directions, "r_adv": r_adv, "lds": lds.detach(),
            "grads": {n: p.grad.detach().clone() for n, p in zip(names, model.parameters())},
            "bn": {k: sd[f"Conv1.conv.1.{k}"].clone() for k in ("running_mean", "running_var", "num_batches_tracked")}}


def run_restatement(case: str, model_seed: int, dtype, bf16: bool = False) -> dict:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vat_ref
    from oracle import unet as OU
    x, d0 = inputs()
    sd = OU.init_state(1, 4, seed=model_seed)             # float32 values, as the tests load them; widened exactly below
    trainable = OU.trainable_keys(sd)
    for k in sd:
        if sd[k].is_floating_point():
            sd[k] = sd[k].to(dtype)
    for k in trainable:
        sd[k].requires_grad_()
    eps = eps_of(case)
    res = vat_ref.vat(vat_ref.oracle_model(sd, bf16), x.to(dtype), d0.to(dtype), CASES[case]["xi"], eps, PROP_EPS, CASES[case]["ip"])
    res["lds"].backward()
    res["grads"] = {k: sd[k].grad.detach().clone() for k in trainable}
    res["pred"] = res["pred"].softmax(1)
    res["lds"] = res["lds"].detach()
    return res


def distances(got: dict, ref: dict) -> dict:
    """What tests/test_gpu_vat.py compares, as distances of ``got`` from ``ref``: ``pred`` and ``lds`` relative, each direction and
    ``r_adv`` as the worst sample's relative L2, the parameter gradients as the worst tensor's relative difference of the L2 norm and
    the relative L2 of the two whole tensors."""
    import vat_ref
    out = dict(pred=float((got["pred"].double() - ref["pred"].double()).abs().max() / ref["pred"].double().abs().max()),
               r_adv=vat_ref.rel_l2_per_sample(got["r_adv"], ref["r_adv"]),
               lds=abs(float(got["lds"]) - float(ref["lds"])) / abs(float(ref["lds"])),
               grad_norms=max(abs(float(got["grads"][n].double().norm()) - float(ref["grads"][n].double().norm())) /
                              float(ref["grads"][n].double().norm()) for n in ref["grads"]))
    for i, (a, b) in enumerate(zip(got["d"], ref["d"])):
        out[f"d{i}"] = vat_ref.rel_l2_per_sample(a, b)
    for n in WHOLE:
        out[f"grad/{n}"] = vat_ref.rel_l2(got["grads"][n], ref["grads"][n])
    return out


def main():
    import_reference()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    torch.set_num_threads(4)
    for model_seed in range(FIRST_MODEL_SEED, FIRST_MODEL_SEED + 64):
        own = {c: distances(run_restatement(c, model_seed, torch.float32), run_restatement(c, model_seed, torch.float64)) for c in CASES}
        ok = all(own[c][k] < OWN_ERROR_LIMITS[c][k] for c in CASES for k in OWN_ERROR_LIMITS[c])
        print(f"model seed {model_seed}: float32 against float64 {own} -> {'taken' if ok else 'float32 is not stable here'}")
        if ok:
            break
    else:
        raise SystemExit("no model seed whose float32 evaluation is within the limits of the float64 one")
    out = {"cfg/model_seed": np.asarray(model_seed), "cfg/prop_eps": np.asarray(PROP_EPS),
           "cfg/shape": np.asarray(SHAPE), "whole": np.asarray(WHOLE)}
    for c in CASES:
        wheel = run_wheel(c, model_seed)
        rest = run_restatement(c, model_seed, torch.float64)
        agree = distances(rest, wheel)
        print(f"case {c}: restatement (float64) against the wheel (float64) {agree}")
        assert all(v < 1e-9 for v in agree.values()), agree
        out[f"{c}/ip"], out[f"{c}/eps"] = np.asarray(CASES[c]["ip"]), np.asarray(CASES[c]["eps"], dtype=np.float64)
        out[f"{c}/xi"] = np.asarray(CASES[c]["xi"])
        # the bf16 storage mode: how far a float32 evaluation of the bf16-ROUNDED restatement (vat_ref.unet_bf16_rounded) lands from
        # its float64 evaluation -- the yardstick of the bf16 comparison; the float64 values themselves are recomputed by the test
        own16 = distances(run_restatement(c, model_seed, torch.float32, True), run_restatement(c, model_seed, torch.float64, True))
        print(f"case {c}: bf16-rounded restatement, float32 against float64 {own16}")
        for k, v in own16.items():
            out[f"own_error_bf16/{c}/{k}"] = np.asarray(v)
        out[f"{c}/pred"], out[f"{c}/r_adv"], out[f"{c}/lds"] = np_(wheel["pred"]), np_(wheel["r_adv"]), np_(wheel["lds"])
        for i, d in enumerate(wheel["d"]):
            out[f"{c}/d{i}"] = np_(d)
        names = list(wheel["grads"])
        out[f"{c}/grad_names"] = np.asarray(names)
        out[f"{c}/grad_norms"] = np.asarray([float(wheel["grads"][n].norm()) for n in names], dtype=np.float64)
        for n in WHOLE:
            out[f"{c}/grad/{n}"] = np_(wheel["grads"][n])
        for k, v in wheel["bn"].items():
            out[f"{c}/bn/{k}"] = np_(v)
        for k, v in own[c].items():
            out[f"own_error/{c}/{k}"] = np.asarray(v)
    save("vat", **out)


if __name__ == "__main__":
    main()
