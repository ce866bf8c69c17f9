"""CPU: the float64 reference of the mlp / normalize cluster-head tests (tests/heads_var_ref.py) checked without a device -- against a
second float64 evaluation built from torch.nn modules, the condition every case exists for computed from its shape with the launch
arithmetic of csrc/heads_var.hip, the zero-norm gradient torch defines (g / eps), and 10 x the fp32-torch error against the cap, so that
the cap is never the number that decides a GPU test."""
import pytest
import torch

import heads_var_ref as V

F64 = torch.float64
KINDS = [(kind, name) for kind in ("local", "global") for name in V.TABLES[kind]]
KIND_IDS = [f"{k}-{n}" for k, n in KINDS]
ALL_PAIRS = [(kind, n, d) for kind in ("local", "global") for n, d in V.pairs(kind)]
ALL_IDS = [f"{k}-{n}-{V.tname(d)}" for k, n, d in ALL_PAIRS]


@pytest.mark.parametrize("kind,name", KINDS, ids=KIND_IDS)
def test_reference_equals_an_independent_module_evaluation(kind, name):
    case, x = V.TABLES[kind][name], V.inputs(kind, name)
    dtype = case["types"][-1]
    ref = V.reference(kind, name, dtype)["ref"]
    feat = V.stored_feat(kind, name, dtype).to(F64)
    wide = [None if x[k] is None else x[k].to(F64) for k in ("w1", "b1", "w2", "b2")]
    other = V.evaluate(kind, case, feat, *wide, x["cot"], fn=V.compose_modules)
    assert set(other) == set(ref) == ({"prob"} if case["fwd_only"] else {"prob", "gfeat", "gw1", "gb1"} | ({"gw2", "gb2"} if case["HID"] else set()))
    for k in ref:
        assert V.rel(other[k], ref[k]) <= 1e-12, (k, V.rel(other[k], ref[k]))
    assert bool(((ref["prob"].sum(2) - 1).abs() < 1e-12).all())
    if not case["fwd_only"]:
        unnamed = sorted(set(range(case["B"])) - set(case["src"]))
        assert float(ref["gfeat"][unnamed].abs().max() if unnamed else 0.0) == 0.0
        assert all(float(ref["gfeat"][i].abs().max()) > 0 for i in case["src"])


@pytest.mark.parametrize("kind,name", KINDS, ids=KIND_IDS)
def test_softmax_is_not_saturated(kind, name):
    ref = V.reference(kind, name, torch.float32)["ref"]
    top = ref["prob"].max(dim=2).values
    assert float((top < 0.9).double().mean()) > 0.5, float((top < 0.9).double().mean())


def test_every_case_reaches_the_branch_it_exists_for():
    L, G = V.LOCAL_CASES, V.GLOBAL_CASES
    for n in ("stride_mlp_norm", "stride_mlp", "stride_lin_norm"):
        c = L[n]
        assert V.local_chunks(c["M"], c["H"], c["W"]) == 1242 > V.MAX_BLOCKS == V.local_bwd_blocks(c["M"], c["H"], c["W"])
        assert (c["H"] * c["W"]) % V.KVT == 16
        assert sorted(set(c["flips"])) == [0, 1, 2, 3] and len(c["flips"]) > 4
        assert c["src"] != sorted(c["src"]) and len(set(range(c["B"])) - set(c["src"])) == 1
        assert c["T"] != 1
    assert [(L[n]["HID"], L[n]["normalize"]) for n in ("stride_mlp_norm", "stride_mlp", "stride_lin_norm")] == [(64, True), (64, False), (0, True)]
    c = L["upconv5"]
    assert V.local_bwd_lds(c["C"], c["HID"], c["K"]) == 103424 > 64 * 1024 and c["H"] * c["W"] < V.KVT      # 103 kB = 101 KiB
    c = L["upconv2"]
    assert c["T"] == 2 and not c["normalize"] and c["K"] == 20 and c["S"] == 5
    c = L["plain"]
    assert c["HID"] == 0 and not c["normalize"]
    c = L["lds_limit"]
    assert V.local_bwd_lds(c["C"], c["HID"], c["K"]) == V.LDS_LIMIT == 150 * 1024
    assert V.local_bwd_lds(c["C"], c["HID"], c["K"] + 1) > V.LDS_LIMIT
    c = L["lds_limit_fwd"]
    assert c["fwd_only"] and c["C"] + c["HID"] + c["K"] == 600 and V.local_fwd_lds(c["C"], c["HID"], c["K"]) == V.LDS_LIMIT
    c = G["conv5"]
    assert V.local_fwd_lds(c["C"], c["HID"], c["K"]) == int(98.5 * 1024) > 64 * 1024
    assert V.global_bwd_lds(c["C"], c["HID"], c["K"]) == 133 * 1024 and V.feat_kernel_chunks(c["H"], c["W"], c["C"]) == 2
    for n in ("mloop_mlp", "mloop_lin"):
        c = G[n]
        assert c["M"] > 128 and V.cdiv(c["M"], V.KVT) == 3 and c["M"] % V.KVT == 22 and c["H"] * c["W"] < 4
    c = G["kmax"]
    assert c["K"] == 64 and c["C"] % 64 != 0 and c["H"] * c["W"] == 1
    c = G["featcap"]
    assert V.local_fwd_lds(c["C"], c["HID"], c["K"]) > 64 * 1024 and V.global_bwd_lds(c["C"], c["HID"], c["K"]) > 64 * 1024
    assert c["H"] * c["W"] * c["C"] >= 32 * 256 * 8 and V.feat_kernel_chunks(c["H"], c["W"], c["C"]) == 32
    # both 16-bit types appear at least twice among the cases that run in one of them
    one = [t for tab in (L, G) for c in tab.values() if len(c["types"]) == 2 for t in c["types"][1:]]
    assert one.count(V.BF16) >= 2 and one.count(V.F16) >= 2
    for tab in (L, G):
        assert all(c["types"][0] == V.F32 for c in tab.values())


@pytest.mark.parametrize("kind,name", [(k, n) for k, n in KINDS if V.TABLES[k][n]["zero"]], ids=[i for i, (k, n) in zip(KIND_IDS, KINDS) if V.TABLES[k][n]["zero"]])
def test_zero_norm_cases_have_a_norm_below_eps(kind, name):
    """The raw logits' norm is below 1e-12 on at least one pixel / sample -- and, being exactly zero there, the probabilities are uniform."""
    case, x = V.TABLES[kind][name], V.inputs(kind, name)
    for dtype in case["types"]:
        z = V.compose_modules(kind, case, V.stored_feat(kind, name, dtype).to(F64), *(None if x[k] is None else x[k].to(F64) for k in ("w1", "b1", "w2", "b2")),
                              raw_logits=True)
        small = (z * z).sum(2).sqrt() < V.NORM_EPS
        assert int(small.sum()) >= 1 and not bool(small.all())
        ref = V.reference(kind, name, dtype)["ref"]["prob"]
        assert bool((ref.movedim(2, -1)[small] == 1.0 / case["K"]).all())


def test_zero_norm_gradient_is_what_torch_gives():
    """F.normalize at a zero vector: the clamp is active, so the gradient is g / eps -- the kernel's `nrm <= eps` branch."""
    z = torch.zeros(1, 4, dtype=F64, requires_grad=True)
    (torch.nn.functional.normalize(z, p=2, dim=1, eps=V.NORM_EPS) * torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=F64)).sum().backward()
    assert torch.equal(z.grad, torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=F64) / V.NORM_EPS)
    # through the softmax as the heads apply it (K = 4, T = 1): dz = p (g - <g, p>) / eps with p uniform
    z = torch.zeros(1, 4, dtype=F64, requires_grad=True)
    (torch.softmax(torch.nn.functional.normalize(z, p=2, dim=1, eps=V.NORM_EPS), 1) * torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=F64)).sum().backward()
    torch.testing.assert_close(z.grad, torch.tensor([[-3.75e11, -1.25e11, 1.25e11, 3.75e11]], dtype=F64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind,name,dtype", ALL_PAIRS, ids=ALL_IDS)
def test_ten_times_the_fp32_torch_error_stays_below_the_cap(kind, name, dtype):
    r = V.reference(kind, name, dtype)
    print(f"\n{kind} {name} {V.tname(dtype)} torch fp32 vs float64:", {k: f"{v:.2e}" for k, v in r["fp32"].items()})
    for k, v in r["fp32"].items():
        assert 0 < 10 * v < V.CAP, (k, v)
        assert r["bound"][k] == 10 * v


def test_half_ulp():
    ref = torch.tensor([1.0, 1.5, 1.999, 2.0, -3.0, 0.75, 1e-6, 0.0], dtype=F64)
    for dtype, p in ((V.BF16, 8), (V.F16, 11)):
        h = V.half_ulp(ref, dtype)
        assert h[0] == h[1] == h[2] == 2.0 ** -p and h[3] == h[4] == 2.0 ** (1 - p) and h[5] == 2.0 ** (-1 - p)
        # a correctly rounded fp32 value is within half an ulp, and some value comes arbitrarily close to it
        x = torch.linspace(0.001, 4.0, 100001, dtype=F64).to(torch.float32)
        d = (x.to(dtype).to(F64) - x.to(F64)).abs()
        assert bool((d <= V.half_ulp(x.to(F64), dtype)).all()) and float((d / V.half_ulp(x.to(F64), dtype)).max()) > 0.99
    assert V.half_ulp(ref, V.F16)[6] == 2.0 ** -25 and float(V.half_ulp(ref, V.F32).abs().max()) == 0
