"""GPU: the mlp / normalize cluster-head kernels (csrc/heads_var.hip, ``ops.local_head_var`` / ``ops.global_head_var``) at the shapes
where their untested paths run -- the local backward's grid-stride loop, launches above 64 KiB of dynamic LDS up to the 150 KiB limit,
T != 1, fp16 and bf16 storage, M > 64 in the global head, K = 64, the zero-norm branch -- (a) against the float64 reference of
tests/heads_var_ref.py, (b) in properties that hold bit for bit, (c) in every refusal of the five entry points; and (d) the global
IID-loss kernels (csrc/mi_global.hip) at K = 64 and N = 300.  The case tables, and why each shape is the smallest that reaches its
branch, are in heads_var_ref.py; tests/test_cpu_heads_var.py checks the reference itself."""
from functools import partial

import numpy as np
import pytest
import torch

import heads_var_ref as V
import synth
import trainer_harness as th
from oracle import iic as OI

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_ = torch.from_numpy
_dump = partial(th.error_dump, "heads_var")          # the numbers DESIGN.md section 8, "Head variants against float64", quotes


def _run(kind, case, feat, params, cot=None, src=None, flips="case", feat_grad=True, module=None):
    """One forward (+ backward with the cotangent ``cot``) of the kernels on ``feat`` [B,C,H,W] (already in its storage type) ->
    {prob, gfeat [B,C,H,W] in the storage type | None, gw1, gb1[, gw2, gb2]} on the CPU.  ``module``: through that head's
    forward_gathered instead of the op, the gradients read from its parameters and restacked."""
    from miseg_amd import ops
    src = case["src"] if src is None else src
    flips = case["flips"] if flips == "case" else flips
    fd = feat.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(feat_grad)
    srcd = torch.tensor(src, dtype=torch.int32, device=DEV)
    fld = None if flips is None else torch.tensor(flips, dtype=torch.int32, device=DEV)
    if module is None:
        p = {k: (None if v is None else v.to(DEV).requires_grad_(True)) for k, v in params.items()}
        if kind == "local":
            prob = ops.local_head_var(fd, p["w1"], p["b1"], p["w2"], p["b2"], srcd, fld, case["T"], case["normalize"])
        else:
            prob = ops.global_head_var(fd, p["w1"], p["b1"], p["w2"], p["b2"], srcd, case["T"], case["normalize"])
    else:
        prob = module.forward_gathered(fd, srcd, fld) if kind == "local" else module.forward_gathered(fd, srcd)
    out = {"prob": prob.detach().cpu()}
    if cot is not None:
        (prob * cot.to(DEV)).sum().backward()
        out["gfeat"] = None if fd.grad is None else fd.grad.cpu()
        if module is None:
            out.update(("g" + k, v.grad.cpu()) for k, v in p.items() if v is not None)
        else:
            sd = module.state_dict(keep_vars=True)
            first, second = (0, 2) if kind == "local" else (2, 4)
            stack = lambda i, leaf: torch.stack([sd[f"_headers.{s}.{i}.{leaf}"].grad for s in range(case["S"])]).flatten(2 if leaf == "weight" else 1).cpu()   # noqa: E731,E501
            out["gw1"], out["gb1"] = stack(first, "weight"), stack(first, "bias")
            if case["HID"]:
                out["gw2"], out["gb2"] = stack(second, "weight"), stack(second, "bias")
    torch.cuda.synchronize()
    return out


def _params(kind, name):
    x = V.inputs(kind, name)
    return {k: x[k] for k in ("w1", "b1", "w2", "b2")}


def _module(kind, case, params):
    from contrastyou.trainer._utils import ClusterHead, LocalClusterHead
    head_type = "mlp" if case["HID"] else "linear"
    if kind == "local":
        head = LocalClusterHead(input_dim=case["C"], head_type=head_type, num_clusters=case["K"], num_subheads=case["S"], T=case["T"],
                                interm_dim=case["HID"] or 64, normalize=case["normalize"])
    else:
        assert case["HID"] in (0, 128)                # the pooled mlp head's hidden width is fixed
        head = ClusterHead(input_dim=case["C"], num_clusters=case["K"], num_subheads=case["S"], head_type=head_type, T=case["T"],
                           normalize=case["normalize"])
    head.load_state_dict({k: v.clone() for k, v in V.state_dict(kind, params["w1"], params["b1"], params["w2"], params["b2"]).items()})
    return head.to(DEV)


# ------------------------------------------------------------------------------------------------------------ (a) against float64
# Error = max |got - ref| / max |ref| per output tensor (_rel of test_gpu_contrast.py); bound = 10 x the error of the same composition
# in torch fp32 on the CPU against the same float64 reference, capped at 1e-4 (the loosest fp32 gradient bound of test_gpu_mi.py; the
# CPU test shows the cap never decides).  No bound comes from the kernel's output.  The probabilities and the parameter gradients are
# fp32 results of fp32 arithmetic on the stored features: the storage type does not loosen them.  gfeat is rounded once to the storage
# type: element-wise |got - ref| <= bound * max |ref| + half an ulp of the storage type at |ref|; "half an ulp at |ref|" is 2^(floor(log2 |ref|) - p), p = 8 significand bits for bf16 and 11 for fp16, i.e. between 2^-9 and 2^-8
# (2^-12 and 2^-11) of |ref|: a correctly rounded result reaches it, so nothing tighter can be asked (heads_var_ref.half_ulp).
# Measured ("Head variants against float64"), kernel / torch fp32: prob and parameter gradients <= 2.1e-6 / 4.1e-6
# (the 79 200-pixel sums of `stride`; every other case <= 8.4e-7 / 5.7e-7), fp32 gfeat <= 8.9e-7 / 7.6e-7, 16-bit gfeat inside its
# element-wise allowance everywhere (closest: 1.2e-9 absolute, global featcap bf16).
def _check(tag, got, kind, name, dtype):
    r = V.reference(kind, name, dtype)
    ref, bound = r["ref"], r["bound"]
    rows, bad = {}, []
    for k in ref:
        g = got[k].double()
        err = V.rel(g, ref[k])
        rows[k] = {"kernel": err, "torch_fp32": r["fp32"][k], "bound": bound[k]}
        if k == "gfeat":
            slack = bound[k] * float(ref[k].abs().max()) + V.half_ulp(ref[k], dtype)
            over = float(((g - ref[k]).abs() - slack).max())
            rows[k]["over_elementwise"] = over
            ok = over <= 0
        else:
            ok = err <= bound[k]
        if not ok:
            bad.append(k)
    print(f"\nheads_var {tag}: " + "  ".join(f"{k} {v['kernel']:.2e}/{v['torch_fp32']:.2e}" for k, v in rows.items()))
    _dump(tag, rows)
    assert set(got) >= set(ref) and not bad, {k: rows[k] for k in bad}
    assert bool(torch.isfinite(got["prob"]).all())


@pytest.mark.parametrize("name,dtype", V.pairs("local"), ids=V.pair_ids("local"))
def test_local_var_against_float64(name, dtype):
    case = V.LOCAL_CASES[name]
    got = _run("local", case, V.stored_feat("local", name, dtype), _params("local", name), None if case["fwd_only"] else V.inputs("local", name)["cot"])
    _check(f"local_{name}_{V.tname(dtype)}", got, "local", name, dtype)


@pytest.mark.parametrize("name,dtype", V.pairs("global"), ids=V.pair_ids("global"))
def test_global_var_against_float64(name, dtype):
    case = V.GLOBAL_CASES[name]
    got = _run("global", case, V.stored_feat("global", name, dtype), _params("global", name), V.inputs("global", name)["cot"])
    _check(f"global_{name}_{V.tname(dtype)}", got, "global", name, dtype)


@pytest.mark.parametrize("kind,name,dtype", V.MODULE_CASES, ids=[f"{k}-{n}-{V.tname(d)}" for k, n, d in V.MODULE_CASES])
def test_modules_against_float64_and_the_op(kind, name, dtype):
    """LocalClusterHead / ClusterHead loaded from the reference's state-dict keys: the stacked views of the per-sub-head parameters and
    the per-parameter gradients are on the path.  Same bounds; and the same bits as the op on the stacked tensors."""
    case, params, cot = V.TABLES[kind][name], _params(kind, name), V.inputs(kind, name)["cot"]
    feat = V.stored_feat(kind, name, dtype)
    got = _run(kind, case, feat, params, cot, module=_module(kind, case, params))
    _check(f"module_{kind}_{name}_{V.tname(dtype)}", got, kind, name, dtype)
    op = _run(kind, case, feat, params, cot)
    for k in op:
        assert torch.equal(op[k], got[k]), k


# ------------------------------------------------------------------------------------------------------------ (b) bit-exact properties
# one case per kernel path: the grid-stride loop, > 64 KiB LDS, HID = 0; the m0 loop, K = 64
BIT_CASES = [("local", "stride_mlp_norm", V.BF16), ("local", "stride_lin_norm", V.F32), ("local", "upconv5", V.F16), ("local", "plain", V.F32),
             ("global", "conv5", V.F16), ("global", "mloop_mlp", V.F32), ("global", "mloop_lin", V.BF16), ("global", "kmax", V.F32)]
BIT_IDS = [f"{k}-{n}-{V.tname(d)}" for k, n, d in BIT_CASES]


def _same(a, b, keys=None):
    for k in (a if keys is None else keys):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind,name,dtype", BIT_CASES, ids=BIT_IDS)
def test_two_calls_give_identical_bits(kind, name, dtype):
    """Deterministic per-block partials and a fixed-order reduce: no atomics anywhere."""
    case, feat, cot = V.TABLES[kind][name], V.stored_feat(kind, name, dtype), V.inputs(kind, name)["cot"]
    a, b = (_run(kind, case, feat, _params(kind, name), cot) for _ in range(2))
    _same(a, b)


@pytest.mark.parametrize("kind,name,dtype", BIT_CASES, ids=BIT_IDS)
def test_gather_and_flip_replay_equal_the_materialised_tensor(kind, name, dtype):
    """(src, flips) on feat against identity src and no flips on feat2[m] = flip(feat[src[m]]): the same bits for the probabilities and
    every parameter gradient, gfeat[src[m]] the un-flipped gfeat2[m], and exactly zero in the rows src does not name."""
    case, feat, cot = V.TABLES[kind][name], V.stored_feat(kind, name, dtype), V.inputs(kind, name)["cot"]
    flips = case["flips"] if kind == "local" else None
    if flips is not None:
        assert set(flips) == {0, 1, 2, 3} or case["M"] < 4
    mirror = lambda t, f: t.flip([d for d, on in ((1, f & 1), (2, f & 2)) if on]) if f else t      # noqa: E731
    feat2 = torch.stack([mirror(feat[i], 0 if flips is None else flips[m]) for m, i in enumerate(case["src"])])
    a = _run(kind, case, feat, _params(kind, name), cot)
    b = _run(kind, case, feat2, _params(kind, name), cot, src=list(range(case["M"])), flips=None)
    _same(a, b, [k for k in a if k != "gfeat"])
    for m, i in enumerate(case["src"]):
        assert torch.equal(a["gfeat"][i], mirror(b["gfeat"][m], 0 if flips is None else flips[m])), (m, i)
    unnamed = sorted(set(range(case["B"])) - set(case["src"]))
    if name.startswith(("stride", "conv5", "mloop")):
        assert unnamed
    for i in unnamed:
        assert int((a["gfeat"][i] != 0).sum()) == 0, i


@pytest.mark.parametrize("kind,name,dtype", BIT_CASES, ids=BIT_IDS)
def test_no_feature_gradient_and_a_scaled_cotangent(kind, name, dtype):
    """A feature that does not require grad: null gfeat, the same parameter-gradient bits.  A cotangent scaled by 0.25 (a power of two):
    every gradient scaled by exactly 0.25."""
    case, feat, cot = V.TABLES[kind][name], V.stored_feat(kind, name, dtype), V.inputs(kind, name)["cot"]
    a = _run(kind, case, feat, _params(kind, name), cot)
    b = _run(kind, case, feat, _params(kind, name), cot, feat_grad=False)
    assert b["gfeat"] is None
    _same(a, b, [k for k in a if k != "gfeat"])
    q = _run(kind, case, feat, _params(kind, name), 0.25 * cot)
    assert torch.equal(q["prob"], a["prob"])
    for k in a:
        if k != "prob":
            assert float(a[k].abs().max()) > 0
            if a[k].dtype == torch.float16:           # a quarter of an fp16 value below 4 x the smallest normal is not an fp16 value
                big = a[k].abs() >= 2.0 ** -12
                assert torch.equal(q[k][big], a[k][big] * 0.25) and float((q[k].double() - 0.25 * a[k].double()).abs().max()) <= 2.0 ** -24, k
            else:
                assert torch.equal(q[k], a[k] * 0.25), k


# ------------------------------------------------------------------------------------------------------------ (c) refusals
SENTINEL = -7.25
_BASE = dict(B=1, H=2, W=2, C=2, M=1, HID=2, S=1, K=2, T=1.0, dt=0, normalize=1)


class _Raw:
    """Buffers of exactly the sizes a shape needs (so that a call that should have been refused, but ran, stays in bounds), outputs
    and workspaces filled with a sentinel."""

    def __init__(self, **kw):
        from miseg_amd import _cabi
        self.c = c = dict(_BASE, **kw)
        B, H, W, C, M, HID, S, K = (c[k] for k in ("B", "H", "W", "C", "M", "HID", "S", "K"))
        r1 = HID if HID else K
        el = {1: torch.bfloat16, 2: torch.float16}.get(c["dt"], torch.float32)
        z = lambda *s: torch.zeros(*s, device=DEV)              # noqa: E731
        f = lambda *s, dtype=torch.float32: torch.full(s, SENTINEL, device=DEV, dtype=dtype)       # noqa: E731
        self.feat, self.src, self.flips = z(B, H, W, C).to(el), torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
        self.w1, self.b1, self.w2, self.b2 = z(S, r1, C) + 0.5, z(S, r1), z(S, K, max(HID, 1)) + 0.25, z(S, K)
        self.gprob_l, self.gprob_g, self.pooled_in = z(S, M, K, H, W) + 1, z(S, M, K) + 1, z(M, C) + 0.5
        self.out = dict(prob_l=f(S, M, K, H, W), prob_g=f(S, M, K), pooled=f(M, C), gfeat=f(B, H, W, C, dtype=el), gw1=f(S, r1, C), gb1=f(S, r1),
                        gw2=f(S, K, max(HID, 1)), gb2=f(S, K), dpool=f(S * M * C))
        self.ws_bytes = V.local_bwd_ws_bytes(M, H, W, C, HID, S, K)
        self.out["ws"] = f(self.ws_bytes // 4)
        self.before = {k: v.clone() for k, v in self.out.items()}
        self.stream = torch.cuda.current_stream().cuda_stream
        self.cabi = _cabi

    def call(self, entry, **over):
        c, o, p = dict(self.c, **{k: v for k, v in over.items() if k in self.c}), self.out, (lambda t: t.data_ptr())
        w2, b2 = (None, None) if over.get("null_w2") or not c["HID"] else (p(self.w2), p(self.b2))
        gw2, gb2 = (p(o["gw2"]), p(o["gb2"])) if c["HID"] else (None, None)
        shape = (c["B"], c["H"], c["W"], c["C"])
        head = (p(self.w1), p(self.b1), c["HID"], w2, b2)
        tail = (c["S"], c["K"], float(c["T"]), c["normalize"])
        if entry == "local_fwd":
            args = (self.stream, c["dt"], p(self.feat), *shape, p(self.src), p(self.flips), c["M"], *head, *tail, p(o["prob_l"]))
        elif entry == "local_bwd":
            args = (self.stream, c["dt"], p(self.feat), *shape, p(self.src), p(self.flips), c["M"], *head, *tail, p(self.gprob_l), p(o["gfeat"]),
                    p(o["gw1"]), p(o["gb1"]), gw2, gb2, p(o["ws"]), self.ws_bytes + over.get("ws_delta", 0))
        elif entry == "global_fwd":
            args = (self.stream, c["dt"], p(self.feat), *shape, p(self.src), c["M"], *head, *tail, p(o["pooled"]), p(o["prob_g"]))
        else:
            assert entry == "global_bwd"
            args = (self.stream, c["dt"], *shape, p(self.src), c["M"], *head, *tail, p(self.pooled_in), p(self.gprob_g), p(o["gfeat"]), p(o["gw1"]), p(o["gb1"]), gw2, gb2, p(o["dpool"]))
        self.cabi.call(f"miseg_head_{entry.replace('_', '_var_')}", *args)

    def changed(self):
        torch.cuda.synchronize()
        return [k for k, v in self.out.items() if not torch.equal(v, self.before[k])]


ENTRIES = ("local_fwd", "local_bwd", "global_fwd", "global_bwd")
REFUSED = [("k1", dict(K=1)), ("k65", dict(K=65)), ("hid257", dict(HID=257)), ("t0", dict(T=0.0)), ("tneg", dict(T=-1.0)), ("dtype7", dict(dt=7)),
           ("null_w2", dict(null_w2=True))]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what,over", REFUSED, ids=[w for w, _ in REFUSED])
def test_refusals_raise_and_write_nothing(entry, what, over):
    from miseg_amd import _cabi
    raw = _Raw(**{k: v for k, v in over.items() if k in _BASE})
    with pytest.raises(_cabi.MisegError):
        raw.call(entry, **over)
    assert raw.changed() == []


def test_the_smallest_valid_calls_run_and_a_short_workspace_is_refused():
    """The buffers of the refusal tests are valid: the same calls without the fault run and write every output; a workspace one byte
    short is refused."""
    from miseg_amd import _cabi
    for dt in (0, 1, 2):
        raw = _Raw(dt=dt)
        with pytest.raises(_cabi.MisegError, match="workspace too small"):
            raw.call("local_bwd", ws_delta=-1)
        assert raw.changed() == []
        assert int(_cabi.lib().miseg_head_local_var_bwd_ws_bytes(1, 2, 2, 2, 2, 1, 2)) == raw.ws_bytes
        raw.call("local_fwd")
        raw.call("local_bwd")
        raw.call("global_fwd")
        raw.call("global_bwd")
        assert sorted(raw.changed()) == sorted(raw.out)
        assert all(bool(torch.isfinite(v.float()).all()) for v in raw.out.values())
        assert bool(((raw.out["prob_l"].sum(2) - 1).abs() < 1e-6).all()) and bool(((raw.out["prob_g"].sum(2) - 1).abs() < 1e-6).all())


def test_ws_bytes_is_minus_one_for_non_positive_arguments():
    from miseg_amd import _cabi
    fn = _cabi.lib().miseg_head_local_var_bwd_ws_bytes
    good = [2, 3, 5, 4, 8, 2, 6]              # M, H, W, C, HID, S, K
    assert int(fn(*good)) == V.local_bwd_ws_bytes(*good) > 0
    assert int(fn(*(good[:4] + [0] + good[5:]))) == V.local_bwd_ws_bytes(2, 3, 5, 4, 0, 2, 6)        # HID = 0 is the single-layer head
    for i in range(7):
        for bad in (0, -1):
            if i == 4 and bad == 0:
                continue
            assert int(fn(*(good[:i] + [bad] + good[i + 1:]))) == -1, (i, bad)


# one step over the LDS limit: C + HID + K = 601 forward, 2 (C + HID + K) = 602 local backward, C + 2 HID + 2 K = 601 global backward
@pytest.mark.parametrize("entry,shape,accepted", [
    ("local_fwd", dict(C=281, HID=256, K=64), False), ("local_fwd", dict(C=280, HID=256, K=64), True),
    ("global_fwd", dict(C=281, HID=256, K=64), False), ("global_fwd", dict(C=280, HID=256, K=64), True),
    ("local_bwd", dict(C=128, HID=128, K=45), False), ("local_bwd", dict(C=128, HID=128, K=44), True),
    ("global_bwd", dict(C=217, HID=128, K=64), False), ("global_bwd", dict(C=216, HID=128, K=64), True),
    # the forward accepts shapes whose backward is then refused: pinned as it is
    ("global_fwd", dict(C=256, HID=128, K=64), True), ("global_bwd", dict(C=256, HID=128, K=64), False),
    ("local_fwd", dict(C=128, HID=128, K=45), True),
])
def test_the_lds_limit(entry, shape, accepted):
    from miseg_amd import _cabi
    raw = _Raw(**shape)
    limit = {"local_fwd": V.local_fwd_lds, "global_fwd": V.local_fwd_lds, "local_bwd": V.local_bwd_lds, "global_bwd": V.global_bwd_lds}[entry]
    assert (limit(shape["C"], shape["HID"], shape["K"]) <= V.LDS_LIMIT) == accepted
    if accepted:
        raw.call(entry)
        touched = raw.changed()
        assert touched and all(bool(torch.isfinite(raw.out[k].float()).all()) for k in touched)
    else:
        with pytest.raises(_cabi.MisegError, match="too large for LDS"):
            raw.call(entry)
        assert raw.changed() == []


# ------------------------------------------------------------------------------------------------------------ (d) global IID loss
# csrc/mi_global.hip allows K <= 64 and any N: K = 64 fills its LDS tables, N = 300 runs the n += blockDim.x stride of the Z recovery.
# Bounds of test_gpu_mi.py::test_global_mi: 1e-5 relative on the losses, 2e-4 max |grad| + 1e-9 on the gradients (joint: its rtol 1e-5,
# atol 1e-8).  Inputs: peaked simplexes (synth.probs at temperature 1/4); the second view of a sub-head is the first with its classes
# rotated by one, so that the two views disagree sample by sample and the mutual information is O(0.1 .. 1) at every N -- at N = 1 a
# pair of views that agree has a loss of ~1e-4 or exactly 0, which no fp32 evaluation holds to 1e-5 relative.  On these inputs the
# oracle itself in fp32 is <= 9.3e-7 from float64; the kernels measured <= 8.2e-7 (losses) and <= 8.3e-7 of the largest entry (gradients).
MI_CASES = [(1, 2), (64, 64), (300, 64), (300, 3)]


def _mi_inputs(n, k):
    key = f"heads_var/gmi_n{n}_k{k}"
    x = T_(synth.probs(key + "/x", (n, k), temperature=0.25))
    z = T_(synth.probs(key + "/n", (n, k), temperature=0.25))
    return torch.stack([x, x.roll(1, 1), z]), torch.stack([x.roll(1, 1), x, z.roll(1, 1)])        # three sub-heads in one launch


@pytest.mark.parametrize("n,k", MI_CASES)
def test_global_mi_at_its_limits(n, k):
    from miseg_amd import ops
    xs, ys = _mi_inputs(n, k)
    xd, yd = xs.to(DEV).requires_grad_(True), ys.to(DEV).requires_grad_(True)
    loss, loss_nl, joint = ops.global_mi(xd, yd)
    wts = torch.tensor([1.0, -2.0, 0.5])
    (loss * wts.to(DEV)).sum().backward()
    rows = {}
    for s in range(3):
        x64, y64 = xs[s].double().requires_grad_(True), ys[s].double().requires_grad_(True)
        truth, truth_nl, p64 = OI.iid_loss(x64, y64)
        gx, gy = torch.autograd.grad(truth * wts[s].double(), [x64, y64])
        rows[s] = {"loss": abs(float(loss[s]) - float(truth)) / abs(float(truth)), "loss_nl": abs(float(loss_nl[s]) - float(truth_nl)) / abs(float(truth_nl)),
                   "gx": float((xd.grad[s].cpu().double() - gx).abs().max() / gx.abs().max()), "gy": float((yd.grad[s].cpu().double() - gy).abs().max() / gy.abs().max()),
                   "value": float(truth)}
        print(f"\nglobal_mi n{n} k{k} s{s}", rows[s])
        assert rows[s]["loss"] <= 1e-5 and rows[s]["loss_nl"] <= 1e-5, rows[s]
        np.testing.assert_allclose(joint[s].detach().cpu().numpy(), p64.detach().numpy(), rtol=1e-5, atol=1e-8)
        gscale = float(max(gx.abs().max(), gy.abs().max()))
        np.testing.assert_allclose(xd.grad[s].cpu().numpy(), gx.numpy(), rtol=0, atol=2e-4 * gscale + 1e-9)
        np.testing.assert_allclose(yd.grad[s].cpu().numpy(), gy.numpy(), rtol=0, atol=2e-4 * gscale + 1e-9)
    _dump(f"gmi_n{n}_k{k}", rows)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n,k", MI_CASES)
def test_compute_joint_at_its_limits(n, k, symmetric):
    from contrastyou.losses.iic_loss import compute_joint
    xs, ys = _mi_inputs(n, k)
    x, y = xs[0].to(DEV).requires_grad_(True), ys[0].to(DEV).requires_grad_(True)
    p = compute_joint(x, y, symmetric=symmetric)
    x64, y64 = xs[0].double().requires_grad_(True), ys[0].double().requires_grad_(True)
    ref = OI.global_joint(x64, y64, symmetric=symmetric)
    np.testing.assert_allclose(p.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-8)
    cot = T_(synth.normal(f"heads_var/cj{n}_{k}/cot", (k, k)))
    (p * cot.to(DEV)).sum().backward()
    (ref * cot.double()).sum().backward()
    gscale = float(max(x64.grad.abs().max(), y64.grad.abs().max()))
    np.testing.assert_allclose(x.grad.cpu().numpy(), x64.grad.numpy(), rtol=0, atol=2e-4 * gscale + 1e-9)
    np.testing.assert_allclose(y.grad.cpu().numpy(), y64.grad.numpy(), rtol=0, atol=2e-4 * gscale + 1e-9)
