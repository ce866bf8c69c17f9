"""CPU: the float64 reference of the MI-loss kernel tests (tests/mi_loss_ref.py) checked without a device -- the closed-form
d loss / d raw against autograd, 10 x the fp32-oracle error against every cap (so that no cap decides a GPU test), the distance between
`loss` and `loss_no_lamb` at lambda = 1.5 (so that a swap cannot pass), the routing of the local cases between the two epilogue forms,
and numpy restatements of the global kernels with the one-line faults the GPU tests must catch applied to them."""
import numpy as np
import pytest
import torch

import mi_loss_ref as M
from oracle import iic as OI

F64 = torch.float64
LOCAL_K2 = [(k, pad) for k, pad in M.LOCAL_WS if k >= 2]


@pytest.mark.parametrize("k,pad", LOCAL_K2, ids=[f"k{k}-p{pad}" for k, pad in LOCAL_K2])
def test_closed_form_local_gradient_equals_autograd(k, pad):
    for kind in M.LOCAL_KINDS:
        for lamda in M.LAMBS:
            raw = M.local_inputs(k, pad, kind).to(F64)
            ref = M.local_reference(k, pad, kind, lamda)["ref"]
            for p in range(M.P_LOCAL):
                r = raw[p].clone().requires_grad_(True)
                loss = OI.local_mi_from_raw(r, lamda)
                g, = torch.autograd.grad(loss, r)
                assert float(loss.detach()) == float(ref["loss"][p])
                assert float((g - ref["grad"][p]).abs().max()) <= 1e-12 * float(g.abs().max()), (kind, lamda, p)


def test_local_inputs_are_what_the_tables_say():
    for k, pad in M.LOCAL_WS:
        t = 2 * pad + 1
        rand, peak = M.local_inputs(k, pad, "rand"), M.local_inputs(k, pad, "peak")
        assert rand.shape == peak.shape == (M.P_LOCAL, t, t, k, k) and rand.dtype == peak.dtype == torch.float32
        assert float(rand.min()) >= 0.01 and not torch.equal(rand[0], rand[1]) and (k * t == 1 or not torch.equal(peak[0], peak[1]))
        assert all(float(peak[p].min()) == 0.0 and int((peak[p] == 0).sum()) == 1 for p in range(M.P_LOCAL))
        if k >= 2:
            diag = peak.diagonal(dim1=3, dim2=4)
            off = peak.clone()
            off.diagonal(dim1=3, dim2=4).zero_()
            assert 5.0 <= float(diag.min()) and float(diag.max()) <= 6.0 and float(off.max()) <= 0.02


def test_k1_reference_is_exactly_zero():
    for k, pad in M.LOCAL_WS:
        if k == 1:
            for kind in M.LOCAL_KINDS:
                ref = M.local_reference(k, pad, kind, 1.5)["ref"]
                assert float(ref["loss"].abs().max()) == 0.0 and float(ref["grad"].abs().max()) == 0.0
    for n, k in M.GLOBAL_K1:
        xs, ys = M.global_inputs(n, k, "independent")
        assert bool((xs == 1).all()) and bool((ys == 1).all())
        ref = M.global_eval(xs, ys, 1.5, F64)
        assert bool((ref["joint"] == 1).all())
        assert all(float(ref[q].abs().max()) < 1e-9 for q in ("loss", "nl", "gx", "gy"))     # log(1 + 1e-10) in float64; exactly 0 in fp32


def test_ten_times_the_fp32_oracle_error_stays_below_every_cap():
    e, b = M.e32(), M.bounds()
    print("\nfamily         E32       bound     cap")
    for k in M.FAMILIES:
        print(f"{k:14s} {e[k]:.2e}  {b[k]:.2e}  {M.CAPS[k]:.0e}")
    for k in M.FAMILIES:
        assert 0 < 10 * e[k] < M.CAPS[k], (k, e[k])
        assert b[k] == 10 * e[k]


def test_global_sub_heads_differ_and_n1_peaked_is_left_out():
    assert not any(n == 1 and kind == "peaked" for n, k, kind in M.GLOBAL_CASES)
    assert {(n, k) for n, k, _ in M.GLOBAL_CASES} | set(M.GLOBAL_K1) == set(M.GLOBAL_NK) and M.GLOBAL_K1 == [(16, 1)]
    for n, k, kind in M.GLOBAL_CASES:
        xs, ys = M.global_inputs(n, k, kind)
        assert xs.shape == ys.shape == (M.S_GLOBAL, n, k)
        for a in range(M.S_GLOBAL):
            assert not torch.equal(xs[a], ys[a])
            for b in range(a + 1, M.S_GLOBAL):
                assert not torch.equal(xs[a], xs[b]) and not torch.equal(ys[a], ys[b])
        ref = M.global_reference(n, k, kind, 1.5)["ref"]
        assert len({float(v) for v in ref["loss"]}) == M.S_GLOBAL           # a kernel that reads sub-head 0 three times cannot pass
    for n, k, sym in M.JOINT_CASES:
        ref = M.joint_reference(n, k, sym)["ref"]["joint"]
        assert not torch.equal(ref[0], ref[1])
        asym = float((ref - ref.transpose(1, 2)).abs().max() / ref.max())
        assert asym < 1e-15 if sym else asym > 1e-3, (n, k, sym, asym)


@pytest.mark.parametrize("n,k,kind", M.GLOBAL_CASES, ids=[f"n{n}-k{k}-{kind}" for n, k, kind in M.GLOBAL_CASES])
def test_loss_and_loss_no_lamb_are_far_apart_at_lambda_1_5(n, k, kind):
    ref = M.global_reference(n, k, kind, 1.5)["ref"]
    for s in range(M.S_GLOBAL):
        scale = M.entropy_scale(ref["joint"][s], 1.5, OI.GLOBAL_EPS)
        assert abs(float(ref["loss"][s]) - float(ref["nl"][s])) > 100 * M.bounds()["global_loss"] * scale
    one = M.global_reference(n, k, kind, 1.0)["ref"]
    assert torch.equal(one["loss"], one["nl"])


def test_local_routing():
    assert M.SINGLE_MAX_K == 28 and M.single_block_lds(28) <= M.LDS_BUDGET < M.single_block_lds(29)
    assert max(k for k, _ in M.LOCAL_SINGLE) == M.SINGLE_MAX_K
    assert set(M.LOCAL_SINGLE) <= set(M.LOCAL_WS) and len(set(M.LOCAL_WS)) == len(M.LOCAL_WS)
    big = [(k, pad) for k, pad in M.LOCAL_WS if k > 32]
    assert big and not set(big) & set(M.LOCAL_SINGLE) and {k for k, _ in big} == {33, 48, 64}
    assert (32, 1) in M.LOCAL_WS and {(29, 0), (29, 2), (32, 0), (32, 2)} <= set(M.LOCAL_WS)
    # the op's limit is this one (no device needed: the constant sits next to ops._local_loss)
    from miseg_amd import ops
    assert ops.LOCAL_LOSS_SINGLE_BLOCK_MAX_K == M.SINGLE_MAX_K


# ------------------------------------------------------------------------------------------------- the global kernels restated
def _np_global(xs, ys, lamb, up, fault=None, pair=False):
    """iic_global_fwd_kernel / iic_global_bwd_kernel in numpy float64, sub-head by sub-head out of flat buffers as the launches index
    them (``pair``: one buffer [S, 2N, K], stride 2 N K).  ``fault``: one of the one-line mutations the suite must catch."""
    S, N, K = xs.shape
    eps = OI.GLOBAL_EPS
    if pair:
        flat = np.concatenate([xs, ys], axis=1).reshape(-1)
        hs = N * K if fault == "pair_stride" else 2 * N * K
        xoff, yoff = 0, N * K
    else:
        flat = np.concatenate([xs.reshape(-1), ys.reshape(-1)])
        hs, xoff, yoff = N * K, 0, S * N * K
    flat = np.concatenate([flat, np.zeros(2 * S * N * K)])            # a wrong stride stays inside the buffer
    loss, nl, gx, gy = np.zeros(S), np.zeros(S), np.zeros((S, N, K)), np.zeros((S, N, K))
    for s in range(S):
        x = flat[xoff + s * hs: xoff + s * hs + N * K].reshape(N, K)
        y = flat[yoff + s * hs: yoff + s * hs + N * K].reshape(N, K)
        raw = x.T @ y
        z = ((raw + raw.T) / 2).sum()
        p = (raw + raw.T) / 2 / z
        ri, cj = p.sum(1, keepdims=True), p.sum(0, keepdims=True)
        a = -(p * (np.log(p + eps) - lamb * np.log(cj + eps) - lamb * np.log(ri + eps))).sum()
        b = -(p * (np.log(p + eps) - np.log(cj + eps) - np.log(ri + eps))).sum()
        loss[s], nl[s] = (b, a) if fault == "swap" else (a, b)
        l1 = 1.0 if fault == "drop_lamb" else lamb
        gp = -(np.log(p + eps) + p / (p + eps) - l1 * (np.log(cj + eps) + cj / (cj + eps)) - lamb * (np.log(ri + eps) + ri / (ri + eps)))
        gsym = (gp + gp.T) / 2
        gu = (up[0] if fault == "upstream0" else up[s]) * (gsym - (gsym * p).sum()) / z
        gx[s], gy[s] = y @ gu.T, x @ gu
    return dict(loss=torch.from_numpy(loss), nl=torch.from_numpy(nl), gx=torch.from_numpy(gx), gy=torch.from_numpy(gy))


RESTATED = [(7, 5, "independent"), (16, 20, "peaked"), (300, 2, "independent")]


@pytest.mark.parametrize("n,k,kind", RESTATED)
def test_numpy_restatement_of_the_global_kernels_and_its_mutations(n, k, kind):
    """The kernels' formulas, restated, meet the float64 reference to 1e-12; with each one-line fault of the issue applied (loss and
    loss_no_lamb swapped, one `lamb *` dropped from the gradient, upstream[0] for every sub-head, the pair layout strided by N K) the
    same comparison the GPU tests make fails by far more than its bound."""
    xs, ys = M.global_inputs(n, k, kind)
    ref = M.global_reference(n, k, kind, 1.5)["ref"]
    b = M.bounds()

    def errors(got):
        got = dict(got, joint=ref["joint"])
        return M.global_errors(got, ref, 1.5)

    x64, y64 = xs.double().numpy(), ys.double().numpy()
    for pair in (False, True):
        clean = errors(_np_global(x64, y64, 1.5, M.WTS, pair=pair))
        assert all(clean[q] <= 1e-12 for q in ("global_loss", "global_nl", "global_grad")), clean
    caught = {"swap": ("global_loss", "global_nl"), "drop_lamb": ("global_grad",), "upstream0": ("global_grad",),
              "pair_stride": ("global_loss", "global_grad")}
    for fault, families in caught.items():
        bad = errors(_np_global(x64, y64, 1.5, M.WTS, fault=fault, pair=fault == "pair_stride"))
        for q in families:
            assert bad[q] > 100 * b[q], (fault, q, bad[q], b[q])
    # at lambda = 1 the first two faults are invisible: the reason every case also runs at 1.5
    one = M.global_reference(n, k, kind, 1.0)["ref"]
    for fault in ("swap", "drop_lamb"):
        got = dict(_np_global(x64, y64, 1.0, M.WTS, fault=fault), joint=one["joint"])
        assert max(M.global_errors(got, one, 1.0).values()) <= 1e-12
