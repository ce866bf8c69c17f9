"""GPU: the kernels that turn a K x K joint into the mutual-information loss and its gradient -- csrc/mi_global.hip (six entry points)
and the local-MI loss epilogue of csrc/mi_local.hip in both its forms -- against the float64 oracle over K (1 .. 64), N (1 .. 300),
lambda (1.0, 1.5), every sub-head / window with data of its own, a weighted upstream; in properties that hold bit for bit; and in every
refusal.  Case tables, inputs, reference and bounds: tests/mi_loss_ref.py (checked by tests/test_cpu_mi_loss_ref.py); every bound is
min(10 x the fp32 oracle's own error over the family, the project's cap) and none comes from a kernel's output.

Largest measured error per family on the MI355X (mi_loss_errors.json, written by _record below) / its bound there:
  global_loss 8.4e-08 / 8.2e-07    global_nl 7.4e-08 / 8.2e-07    global_joint 7.3e-07 / 4.0e-06    global_grad 1.9e-05 / 9.7e-05
  cj_value 6.2e-07 / 3.7e-06       cj_grad 3.6e-07 / 3.1e-06      local_loss 1.6e-07 / 9.8e-07      local_grad 1.1e-06 / 4.0e-06
K = 29 / 32 end to end: loss within 5.4e-08 relative, gradients within 6.5e-07 of their scale.

One fault the suite cannot see, because it changes no bit: exchanging `rs` and `cs` in the K > 32 branch of loss_displacement.  The
symmetrised joint Pw is (q + qt) / 2 at (i, j) and (qt + q) / 2 at (j, i) -- the same bits -- so the row sums and the column sums are
added from the same numbers in the same order.
"""
import os

import pytest
import torch

import mi_loss_ref as M
import synth
import trainer_harness as th
from oracle import iic as OI

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.0
_MAXIMA = {}


def _record(errors):
    """Largest achieved error per family; with MISEG_ERROR_DUMP=<dir> (the switch of test_gpu_heads_var.py) they are written there as
    mi_loss_errors.json: the figures of the docstring above."""
    for k, v in errors.items():
        _MAXIMA[k] = max(_MAXIMA.get(k, 0.0), float(v))
    if os.environ.get("MISEG_ERROR_DUMP"):
        th.error_dump("mi_loss", "errors", {k: {"kernel": v, "bound": M.bounds()[k]} for k, v in _MAXIMA.items()}, sort_keys=True)


def _check(tag, errors):
    b = M.bounds()
    print(f"\n{tag}: " + "  ".join(f"{k} {v:.2e}/{b[k]:.2e}" for k, v in errors.items()))
    _record(errors)
    bad = {k: (v, b[k]) for k, v in errors.items() if not v <= b[k]}
    assert not bad, (tag, bad)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------ global MI
def _global_two(xs, ys, lamb):
    from miseg_amd import ops
    xd, yd = xs.to(DEV).requires_grad_(True), ys.to(DEV).requires_grad_(True)
    loss, nl, joint = ops.global_mi(xd, yd, lamb)
    (loss * torch.tensor(M.WTS, device=DEV)).sum().backward()
    return dict(loss=loss.detach().cpu(), nl=nl.cpu(), joint=joint.cpu(), gx=xd.grad.cpu(), gy=yd.grad.cpu())


def _global_pair(xs, ys, lamb):
    from miseg_amd import ops
    n = xs.shape[1]
    prob = torch.cat([xs, ys], dim=1).to(DEV).requires_grad_(True)           # [S, 2N, K]: the two views stacked along dim 1
    loss, nl, joint = ops.global_mi_pair(prob, lamb)
    (loss * torch.tensor(M.WTS, device=DEV)).sum().backward()
    return dict(loss=loss.detach().cpu(), nl=nl.cpu(), joint=joint.cpu(), gx=prob.grad[:, :n].cpu(), gy=prob.grad[:, n:].cpu())


GLOBAL_PARAMS = [(n, k, kind, lamb) for n, k, kind in M.GLOBAL_CASES for lamb in M.LAMBS]


@pytest.mark.parametrize("n,k,kind,lamb", GLOBAL_PARAMS, ids=[f"n{n}-k{k}-{kind}-l{lamb}" for n, k, kind, lamb in GLOBAL_PARAMS])
def test_global_mi_against_float64(n, k, kind, lamb):
    """All three sub-heads of global_mi and of global_mi_pair, each against its own float64 reference: loss, loss_no_lamb, joint and
    the gradients of (loss * (1, -2, 0.5)).sum(); the joint bit-symmetric ((s + t) / 2 with the operands swapped); the pair form the
    same bits as the two-tensor form."""
    xs, ys = M.global_inputs(n, k, kind)
    ref = M.global_reference(n, k, kind, lamb)["ref"]
    two, pair = _global_two(xs, ys, lamb), _global_pair(xs, ys, lamb)
    for form, got in (("two", two), ("pair", pair)):
        assert all(bool(torch.isfinite(v).all()) for v in got.values())
        _check(f"global_mi[{form}] n{n} k{k} {kind} lamb {lamb}", M.global_errors(got, ref, lamb))
        assert torch.equal(got["joint"], got["joint"].transpose(1, 2))
    for q in two:
        assert torch.equal(two[q], pair[q]), q


@pytest.mark.parametrize("n,k", M.GLOBAL_K1)
def test_global_mi_with_one_cluster_is_exactly_zero(n, k):
    xs, ys = M.global_inputs(n, k, "independent")
    for lamb in M.LAMBS:
        for got in (_global_two(xs, ys, lamb), _global_pair(xs, ys, lamb)):
            assert bool((got["joint"] == 1).all())
            assert all(float(got[q].abs().max()) == 0.0 for q in ("loss", "nl", "gx", "gy")), got


@pytest.mark.parametrize("n,k", [(7, 5), (16, 33)])
def test_global_bwd_without_upstream_is_upstream_of_ones(n, k):
    from miseg_amd import _cabi
    xs, ys = (t.to(DEV) for t in M.global_inputs(n, k, "peaked"))
    s = xs.shape[0]
    outs = []
    for up in (None, torch.ones(s, device=DEV)):
        gx, gy = torch.full_like(xs, SENTINEL), torch.full_like(ys, SENTINEL)
        _cabi.call("miseg_iic_global_bwd", _stream(), _ptr(xs), _ptr(ys), s, n, k, 1.5, _ptr(up), _ptr(gx), _ptr(gy))
        outs.append((gx.cpu(), gy.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ref = M.global_eval(xs.cpu(), ys.cpu(), 1.5, M.F64)
    for i in range(s):           # upstream of ones: the reference's gradient of (loss * WTS).sum() with the weight taken out again
        gs = float(max(ref["gx"][i].abs().max(), ref["gy"][i].abs().max())) / abs(M.WTS[i])
        for got, q in zip(outs[0], ("gx", "gy")):
            assert float((got[i].double() - ref[q][i] / M.WTS[i]).abs().max()) <= M.bounds()["global_grad"] * gs


# ------------------------------------------------------------------------------------------------------------ compute_joint
@pytest.mark.parametrize("n,k,symmetric", M.JOINT_CASES, ids=[f"n{n}-k{k}-{'sym' if s else 'asym'}" for n, k, s in M.JOINT_CASES])
def test_compute_joint_against_float64(n, k, symmetric):
    from miseg_amd import ops
    xs, ys, cot = M.joint_inputs(n, k)
    ref = M.joint_reference(n, k, symmetric)["ref"]
    xd, yd = xs.to(DEV).requires_grad_(True), ys.to(DEV).requires_grad_(True)
    joint = ops.global_joint(xd, yd, symmetric)
    (joint * cot.to(DEV)).sum().backward()
    got = dict(joint=joint.detach().cpu(), gx=xd.grad.cpu(), gy=yd.grad.cpu())
    _check(f"compute_joint n{n} k{k} symmetric {symmetric}", M.joint_errors(got, ref))
    for s in range(M.S_JOINT):
        assert torch.equal(got["joint"][s], got["joint"][s].t()) == symmetric
        if not symmetric:           # the asymmetry of the reference is there, not merely some asymmetry
            asym, asym64 = got["joint"][s] - got["joint"][s].t(), ref["joint"][s] - ref["joint"][s].t()
            assert float(asym64.abs().max()) > 1e-3 * float(ref["joint"][s].max())
            assert float((asym.double() - asym64).abs().max()) <= 2 * M.bounds()["cj_value"] * float(ref["joint"][s].max())


# ------------------------------------------------------------------------------------------------------------ local epilogue
def _local_call(form, raw, k, pad, lamda, ws_delta=0, p=None):
    """One ABI call of the single-block (``form`` = "single") or per-displacement ("ws") epilogue on raw [P,T,T,K,K] (device) ->
    (loss [P], grad_raw, workspace) on the device, outputs pre-filled with the sentinel."""
    from miseg_amd import _cabi
    p = raw.shape[0] if p is None else p
    loss, grad = torch.full((raw.shape[0],), SENTINEL, device=DEV), torch.full_like(raw, SENTINEL)
    if form == "ws":
        nb = raw.shape[0] * (2 * pad + 1) ** 2 * 4
        assert p <= 0 or _cabi.query("miseg_iic_local_loss_ws_bytes", pad, p) == p * (2 * pad + 1) ** 2 * 4
        ws = torch.full((nb // 4,), SENTINEL, device=DEV)
        try:
            _cabi.call("miseg_iic_local_loss_fwd_ws", _stream(), _ptr(raw), k, pad, p, float(lamda), _ptr(loss), _ptr(grad), _ptr(ws), nb + ws_delta)
        finally:
            torch.cuda.synchronize()
            _local_call.last = (loss, grad, ws)
        return loss, grad, ws
    try:
        _cabi.call("miseg_iic_local_loss_fwd", _stream(), _ptr(raw), k, pad, p, float(lamda), _ptr(loss), _ptr(grad))
    finally:
        torch.cuda.synchronize()
        _local_call.last = (loss, grad, None)
    return loss, grad, None


def _untouched():
    return all(t is None or bool((t == SENTINEL).all()) for t in _local_call.last)


@pytest.mark.parametrize("k,pad", M.LOCAL_WS, ids=[f"k{k}-p{pad}" for k, pad in M.LOCAL_WS])
def test_local_epilogue_against_float64(k, pad):
    """loss[P] and grad_raw of both windows against oracle.iic.local_mi_from_raw / local_mi_grad_wrt_raw in float64: the `_ws` form
    on every case, the single-block form wherever it holds K, and then the same bits of grad_raw from both (the loss differs in the
    order its T^2 terms are added only)."""
    forms = ("ws", "single") if (k, pad) in M.LOCAL_SINGLE else ("ws",)
    for kind in M.LOCAL_KINDS:
        for lamda in M.LAMBS:
            raw = M.local_inputs(k, pad, kind)
            ref = M.local_reference(k, pad, kind, lamda)["ref"]
            grads = []
            for form in forms:
                loss, grad, _ = _local_call(form, raw.to(DEV), k, pad, lamda)
                got = dict(loss=loss.cpu(), grad=grad.cpu())
                grads.append(got["grad"])
                assert bool(torch.isfinite(got["loss"]).all()) and bool(torch.isfinite(got["grad"]).all())
                if k == 1:
                    assert float(got["loss"].abs().max()) == 0.0 and float(got["grad"].abs().max()) == 0.0
                    assert float(ref["loss"].abs().max()) == 0.0 and float(ref["grad"].abs().max()) == 0.0
                else:
                    _check(f"local_loss[{form}] k{k} pad{pad} {kind} lamda {lamda}", M.local_errors(got, ref, raw, lamda))
            if len(grads) == 2:
                assert torch.equal(grads[0], grads[1]), (kind, lamda)


# ------------------------------------------------------------------------------------------------------------ refusals
GLOBAL_ENTRIES = ("joint_fwd", "joint_bwd", "fwd_pair", "bwd_pair", "fwd", "bwd")
GLOBAL_REFUSED = [("k65", dict(K=65)), ("k0", dict(K=0)), ("n0", dict(N=0)), ("s0", dict(S=0)), ("null_out", dict(null_out=True))]


class _GlobalRaw:
    """Buffers of the sizes max(shape, 1) needs (a call that should have been refused, but ran, stays in bounds); outputs filled with
    the sentinel."""

    def __init__(self, S=2, N=3, K=4):
        self.S, self.N, self.K = S, N, K
        s, n, k = max(S, 1), max(N, 1), max(K, 1)
        u = lambda *sh: torch.full(sh, 1.0 / k, device=DEV)                    # noqa: E731
        f = lambda *sh: torch.full(sh, SENTINEL, device=DEV)                   # noqa: E731
        self.x, self.y, self.prob, self.joint_in, self.gjoint, self.up = u(s, n, k), u(s, n, k), u(s, 2 * n, k), u(s, k, k), u(s, k, k), u(s)
        self.out = dict(joint=f(s, k, k), loss=f(s), nl=f(s), gx=f(s, n, k), gy=f(s, n, k), gprob=f(s, 2 * n, k))

    def call(self, entry, null_out=False):
        from miseg_amd import _cabi
        o, dims = self.out, (self.S, self.N, self.K)
        first = (lambda t: None) if null_out else _ptr                           # the entry's first output pointer
        args = {"joint_fwd": (_ptr(self.x), _ptr(self.y), *dims, 1, first(o["joint"])),
                "joint_bwd": (_ptr(self.x), _ptr(self.y), *dims, 1, _ptr(self.joint_in), _ptr(self.gjoint), first(o["gx"]), _ptr(o["gy"])),
                "fwd_pair": (_ptr(self.prob), *dims, 1.5, first(o["loss"]), _ptr(o["nl"]), _ptr(o["joint"])),
                "bwd_pair": (_ptr(self.prob), *dims, 1.5, _ptr(self.up), first(o["gprob"])),
                "fwd": (_ptr(self.x), _ptr(self.y), *dims, 1.5, first(o["loss"]), _ptr(o["nl"]), _ptr(o["joint"])),
                "bwd": (_ptr(self.x), _ptr(self.y), *dims, 1.5, _ptr(self.up), first(o["gx"]), _ptr(o["gy"]))}[entry]
        try:
            _cabi.call("miseg_iic_global_" + entry, _stream(), *args)
        finally:
            torch.cuda.synchronize()

    def changed(self):
        return sorted(k for k, v in self.out.items() if not bool((v == SENTINEL).all()))


WRITES = {"joint_fwd": ["joint"], "joint_bwd": ["gx", "gy"], "fwd_pair": ["joint", "loss", "nl"], "bwd_pair": ["gprob"],
          "fwd": ["joint", "loss", "nl"], "bwd": ["gx", "gy"]}


@pytest.mark.parametrize("entry", GLOBAL_ENTRIES)
@pytest.mark.parametrize("what,over", GLOBAL_REFUSED, ids=[w for w, _ in GLOBAL_REFUSED])
def test_global_refusals_raise_and_write_nothing(entry, what, over):
    from miseg_amd import _cabi
    raw = _GlobalRaw(**{k: v for k, v in over.items() if k in ("S", "N", "K")})
    with pytest.raises(_cabi.MisegError):
        raw.call(entry, null_out=over.get("null_out", False))
    assert raw.changed() == []


@pytest.mark.parametrize("entry", GLOBAL_ENTRIES)
def test_the_refusal_buffers_are_valid(entry):
    """The same call without the fault runs and writes exactly the entry's outputs, at K = 64 too."""
    for k in (4, 64):
        raw = _GlobalRaw(K=k)
        raw.call(entry)
        assert raw.changed() == WRITES[entry]
        assert all(bool(torch.isfinite(raw.out[q]).all()) for q in WRITES[entry])


@pytest.mark.parametrize("form", ["single", "ws"])
def test_local_loss_refusals_raise_and_write_nothing(form):
    from miseg_amd import _cabi
    for k, p in ((65, 2), (5, 0)):
        raw = torch.rand(2, 3, 3, k, k, device=DEV) + 0.01
        with pytest.raises(_cabi.MisegError, match="bad shape"):
            _local_call(form, raw, k, 1, 1.5, p=p)
        assert _untouched()
    raw = torch.rand(2, 3, 3, 5, 5, device=DEV) + 0.01
    if form == "ws":
        with pytest.raises(_cabi.MisegError, match="workspace too small"):
            _local_call(form, raw, 5, 1, 1.5, ws_delta=-4)
        assert _untouched()
    _local_call(form, raw, 5, 1, 1.5)                    # the same buffers without the fault: every output written
    assert not any(t is not None and bool((t == SENTINEL).any()) for t in _local_call.last)


def test_single_block_epilogue_holds_28_clusters_and_refuses_29():
    """The limit ops._local_loss routes by: 16 x (3 K^2 + 4 K) x 4 bytes of LDS against 156 KiB."""
    from miseg_amd import _cabi, ops
    assert ops.LOCAL_LOSS_SINGLE_BLOCK_MAX_K == M.SINGLE_MAX_K == 28
    raw = torch.rand(1, 1, 1, 28, 28, device=DEV) + 0.01
    loss, grad, _ = _local_call("single", raw, 28, 0, 1.0)
    assert bool(torch.isfinite(loss).all()) and not bool((grad == SENTINEL).any())
    raw = torch.rand(1, 1, 1, 29, 29, device=DEV) + 0.01
    with pytest.raises(_cabi.MisegError, match="K too large"):
        _local_call("single", raw, 29, 0, 1.0)
    assert _untouched()
    loss, grad, _ = _local_call("ws", raw, 29, 0, 1.0)
    assert bool(torch.isfinite(loss).all()) and not bool((grad == SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------ K = 29 .. 32 end to end
@pytest.mark.parametrize("k", [29, 32])
@pytest.mark.parametrize("pad", [0, 1])
def test_local_mi_with_29_to_32_clusters_at_small_padding(k, pad):
    """ops.local_mi_losses at K = 29 / 32 and padding 0 / 1 (padding 1 is in the shipped `paddings: [1, 3]`): the joint forward and
    the backward accept these, the single-block epilogue does not, and `_local_loss` sent every pad < 2 call to it -- "K too large" at
    the first step.  Loss and gradients against OI.iid_seg_loss in float64 at the bounds of
    test_gpu_mi.py::test_local_joint_and_loss_vs_golden; also the fp32 backward's first float64 comparison above K = 20."""
    from miseg_amd import ops
    from test_gpu_mi import LOCAL_BWD_ATOL
    n, h, w = 2, 12, 12
    key = f"mi_loss/e2e_k{k}_p{pad}"
    # peaked, correlated maps (the inputs test_gpu_mi.py applies 1e-5 relative to literally): the loss is -0.75 .. -1.1 and the oracle
    # in fp32 within 6e-8 of it; on synth.probs the loss is -0.01 and the fp32 oracle itself 5e-6 relative from float64
    xs, ys = (torch.from_numpy(a) for a in synth.peaked_pair(key, (n, k, h, w)))
    x64, y64 = xs.double().requires_grad_(True), ys.double().requires_grad_(True)
    truth = OI.iid_seg_loss(x64, y64, pad)
    gx64, gy64 = torch.autograd.grad(truth, [x64, y64])
    truth = truth.detach()
    x, y = xs.to(DEV).requires_grad_(True), ys.to(DEV).requires_grad_(True)
    loss = ops.local_mi_losses(x, y, pad, [(0, h, 0, w)])[0]
    loss.backward()
    gscale = float(gx64.abs().max())
    errs = (abs(float(loss.detach()) - float(truth)) / abs(float(truth)), float((x.grad.cpu().double() - gx64).abs().max()) / gscale,
            float((y.grad.cpu().double() - gy64).abs().max()) / gscale)
    print(f"\nlocal_mi k{k} pad{pad}: loss {errs[0]:.2e} (of |loss| = {float(truth):.3e})  gx {errs[1]:.2e}  gy {errs[2]:.2e}")
    assert errs[0] <= 1e-5, (float(loss.detach()), float(truth))
    assert errs[1] <= LOCAL_BWD_ATOL and errs[2] <= LOCAL_BWD_ATOL, errs
