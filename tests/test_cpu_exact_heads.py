"""The float64 references of tests/exact_heads.py against torch's own float64 autograd, the dispatch mirror against the case tables, and
every dyadic recipe of test_gpu_exact_heads.py inside the exact range at every shape and storage type it uses -- so a GPU case can never
fail on its own precondition.  Runs anywhere (no GPU)."""
import pytest
import torch

import exact_heads as E
import exact_ref as R

F64 = torch.float64


def _ids(pairs):
    return [f"{n}-{E.tname(d)}" for n, d in pairs]


# ------------------------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("c,s,k,m,h,w,T", [(8, 3, 6, 3, 5, 7, 0.8), (4, 2, 20, 4, 6, 4, 1.0), (12, 1, 7, 2, 3, 9, 2.0)])
def test_local_reference_equals_float64_autograd_through_the_softmax(c, s, k, m, h, w, T):
    """Continuous data: prob IS softmax((W f + b) / T); autograd of sum g prob through gather, flip, convolution and softmax against
    both forms of head_local_bwd_ref, which see prob only as an input."""
    gen = torch.Generator().manual_seed(5)
    b = m + 2
    src, flips = E.pick_src(b, m), [(i + 1) % 4 for i in range(m)]
    feat = torch.randn(b, c, h, w, dtype=F64, generator=gen).requires_grad_(True)
    wt = torch.randn(s, k, c, dtype=F64, generator=gen).requires_grad_(True)
    bias = torch.randn(s, k, dtype=F64, generator=gen).requires_grad_(True)
    g = torch.randn(s, m, k, h, w, dtype=F64, generator=gen)
    z = torch.einsum("skc,mchw->smkhw", wt, E.gather_flip(feat, src, flips)) + bias[:, None, :, None, None]
    prob = torch.softmax(z / T, dim=2)
    (prob * g).sum().backward()
    for method in ("einsum", "autograd"):
        gfeat, gw, gb = E.head_local_bwd_ref(feat.detach(), wt.detach(), src, flips, T, prob.detach(), g, method=method)
        for got, want in ((gfeat, feat.grad), (gw, wt.grad), (gb, bias.grad)):
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-13), method
        assert not bool(gfeat[0].any()) and not bool(gfeat[b - 1].any()) and bool(feat.grad[1].any())
    assert torch.allclose(E.dz_ref(prob.detach(), g, T), E.dz_ref(prob.detach(), g, T, "autograd"), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name,dtype", [("wave_16x5x20_2x6x10", torch.bfloat16), ("rw28_12x3x7_3x10x12", torch.float16),
                                        ("bf_32x3x20_2x37x45", torch.float16), ("rw64_16x6x20_2x22x36", torch.float32)], ids=str)
def test_the_two_local_reference_forms_are_equal_on_dyadic_cases(name, dtype):
    """On the GPU cases' own data every float64 operation is exact, so the two forms agree bit for bit."""
    for fs in range(len(E.flip_sets(E.LOCAL_CASES[name][4]))):
        c = E.local_case(name, dtype, "dz", fs)
        gfeat, gw, gb = E.head_local_bwd_ref(c["feat"], c["w"], c["src"], c["flips"], c["T"], c["prob"], c["gprob"], method="autograd")
        assert torch.equal(gfeat, c["gfeat"]) and torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])
        assert torch.equal(E.dz_ref(c["prob"], c["gprob"], c["T"]), E.dz_ref(c["prob"], c["gprob"], c["T"], "autograd"))


def test_flip_sets_and_sources():
    for m in (2, 3, 4, 16):
        masks = {f for fs in E.flip_sets(m) for f in fs}
        assert masks == {0, 1, 2, 3}
        src = E.pick_src(m + 2, m)
        assert len(set(src)) == m and 0 not in src and m + 1 not in src and src != sorted(src)
    x = torch.arange(2 * 3 * 4, dtype=F64).view(1, 2, 3, 4)
    assert torch.equal(E.gather_flip(x, [0], [1])[0], x[0].flip(1)) and torch.equal(E.gather_flip(x, [0], [2])[0], x[0].flip(2))
    assert torch.equal(E.gather_flip(x, [0], [3])[0], x[0].flip(1, 2)) and torch.equal(E.gather_flip(x, [0], [0])[0], x[0])


@pytest.mark.parametrize("name", sorted(E.GLOBAL_CASES))
def test_global_reference_forms_are_equal_and_match_autograd(name):
    c = E.global_case(name)
    hw = E.GLOBAL_CASES[name][1] ** 2
    gvec, gw, gb = E.head_global_bwd_ref(c["pooled"], c["w"], c["src"], hw, c["T"], c["prob"], c["gprob"], method="autograd")
    assert torch.equal(gvec, c["gvec"]) and torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])
    assert torch.equal(c["pooled"], torch.stack([c["feat"][i].sum((1, 2)) / hw for i in c["src"]]))
    # continuous data through the real softmax
    gen = torch.Generator().manual_seed(3)
    s, m, k, ch = 2, 3, 5, 6
    pooled = torch.randn(m, ch, dtype=F64, generator=gen).requires_grad_(True)
    wt = torch.randn(s, k, ch, dtype=F64, generator=gen).requires_grad_(True)
    bias = torch.randn(s, k, dtype=F64, generator=gen).requires_grad_(True)
    g = torch.randn(s, m, k, dtype=F64, generator=gen)
    prob = torch.softmax((torch.einsum("skc,mc->smk", wt, pooled) + bias[:, None, :]) / 0.8, dim=2)
    (prob * g).sum().backward()
    gvec, gw, gb = E.head_global_bwd_ref(pooled.detach(), wt.detach(), [2, 0, 1], 4, 0.8, prob.detach(), g)
    assert torch.allclose(gvec * 4, pooled.grad, rtol=1e-12) and torch.allclose(gw, wt.grad, rtol=1e-12) and torch.allclose(gb, bias.grad, rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ the dispatch mirror
def test_every_case_lands_on_the_instance_its_name_states():
    seen = set()
    for name, dtype in E.local_pairs():
        _, c, s, k, m, h, w, _ = E.LOCAL_CASES[name]
        inst = E.bwd_instance(dtype, c, s, k, h, w, m)
        assert E.FAMILY[name.split("_")[0]] in inst, (name, inst)
        assert E.bwd_loops(dtype, c, s, k, h, w, m) == (name in ("wave_16x5x20_4x128x136", "k20_16x5x20_4x112x112")), name
        assert E.bwd_lds_bytes(c, s, k) <= 150 * 1024 and c % 4 == 0 and s * k <= 256
        seen.add(inst)
    for want in ("head_local_bwd_wave_kernel<16,false>[bf16]", "head_local_bwd_wave_kernel<16,false>[f16]",
                 "head_local_bwd_fused_kernel<bf16,2,25,true,true>", "head_local_bwd_fused_kernel<f16,2,25,true,true>",
                 "head_local_bwd_fused_kernel<float,1,25,true,false>", "head_local_bwd_fused_kernel<float,2,25,true,false>",
                 "head_local_bwd_fused_kernel<float,4,25,true,false>", "head_local_bwd_fused_kernel<float,8,25,true,false>",
                 "head_local_bwd_fused_kernel<bf16,1,25,true,false>", "head_local_bwd_fused_kernel<bf16,2,25,true,false>",
                 "head_local_bwd_fused_kernel<bf16,4,25,true,false>", "head_local_bwd_fused_kernel<bf16,8,25,true,false>",
                 "head_local_bwd_fused_kernel<float,1,28,false,false>", "head_local_bwd_fused_kernel<bf16,2,28,false,false>",
                 "head_local_bwd_fused_kernel<float,1,64,false,false>", "head_local_bwd_fused_kernel<bf16,2,64,false,false>",
                 "head_local_bwd_fused_kernel<f16,1,28,false,false>", "head_local_bwd_fused_kernel<f16,1,64,false,false>"):
        assert want in seen, want
    # the refusals of test_gpu_exact_heads.py are refusals by the mirrored rules too
    assert E.bwd_lds_bytes(128, 4, 64) > 150 * 1024 and E.bwd_lds_bytes(32, 4, 64) <= 150 * 1024
    for name, dtype in E.fwd_pairs():
        _, c, s, k, m, h, w = E.FWD_CASES[name]
        inst = E.fwd_instance(dtype, c, s, k, h, w)
        key = name.split("_k")[0] if name.startswith("reg") or name.startswith("generic") else name.split("_")[0]
        if name == "k20_off_mfma_7x9":
            assert inst == f"head_local_fwd_reg_kernel<{E.tname(dtype)},20,1,false>"
        elif name == "k20_off_mfma_c32_s6":
            assert inst == f"head_local_fwd_reg_kernel<{E.tname(dtype)},20,4,true>"
        else:
            assert E.FWD_FAMILY[key] in inst, (name, inst)
    assert max(E.FWD_CASES[n][5] * E.FWD_CASES[n][6] for n in E.FWD_CASES) == 72 * 36


# ------------------------------------------------------------------------------------------------------------------ the recipes
@pytest.mark.parametrize("name,dtype", E.local_pairs(), ids=_ids(E.local_pairs()))
def test_local_backward_recipe_is_inside_the_exact_range(name, dtype):
    """For every flip assignment of the case: sums below 2^24 lsb, operands exact; 16-bit types: hi + lo reproduces dz exactly, W has no
    lo part (so no product has two), and the lo plane of dz is non-zero for at least LO_SHARE of the non-zero entries."""
    m = E.LOCAL_CASES[name][4]
    for fs in range(len(E.flip_sets(m))):
        c = E.local_precondition(name, dtype, "dz", fs)
        assert sorted(set(c["flips"])) != [] and len(c["src"]) == m and c["B"] == m + 2
        if dtype in E.HALF:
            dz = E.dz_ref(c["prob"], c["gprob"], c["T"])
            hi, lo = E.split(dz, dtype)
            assert torch.equal(hi + lo, dz)
            assert not bool(E.split(c["w"], dtype)[1].any())
            if c["den"] == E.DEN[dtype]:
                share = float((lo != 0).sum()) / float((dz != 0).sum())
                assert share >= E.LO_SHARE, share
    if dtype in E.HALF:     # at least one shape of every 16-bit kernel carries a non-zero lo plane
        assert any(E.LOCAL_CASES[n][7].get("den", E.DEN[dtype]) == E.DEN[dtype] for n in E.LOCAL_CASES if n.split("_")[:2] == name.split("_")[:2])


W_PAIRS = E.local_pairs(E.W_RECIPE_CASES)


@pytest.mark.parametrize("name,dtype", W_PAIRS, ids=_ids(W_PAIRS))
def test_weight_split_recipe_is_inside_the_exact_range(name, dtype):
    """The roles swapped: W = n / 64 with a non-zero lo part for at least W_LO_SHARE of the weights, dz inside the 16-bit type (lo = 0
    everywhere): the kernels drop the lo x lo product, and here there is none."""
    c = E.local_precondition(name, dtype, "w", 0)
    dz = E.dz_ref(c["prob"], c["gprob"], c["T"])
    hi, lo = E.split(dz, dtype)
    assert torch.equal(hi, dz) and not bool(lo.any())
    whi, wlo = E.split(c["w"], dtype)
    assert torch.equal(whi + wlo, c["w"])
    assert float((wlo != 0).double().mean()) >= E.W_LO_SHARE


GLOBAL_PAIRS = [(n, d) for n in sorted(E.GLOBAL_CASES) for d in E.ALL]


@pytest.mark.parametrize("name,dtype", GLOBAL_PAIRS, ids=_ids(GLOBAL_PAIRS))
def test_global_head_recipe_is_inside_the_exact_range(name, dtype):
    c = E.global_precondition(name, dtype)
    assert bool((c["prob"].sum(2) == 1).all())
    assert R.quantum_of(c["gvec"]) < 1.0


def test_forward_cases_build_a_simplex_reference():
    c = E.fwd_case("reg1_k10_9x10", torch.bfloat16)
    assert c["ref"].shape == (2, 3, 10, 9, 10) and torch.allclose(c["ref"].sum(2), torch.ones(2, 3, 9, 10, dtype=F64), rtol=1e-14)
    assert torch.equal(c["feat"].to(torch.bfloat16).to(F64), c["feat"]) and len(set(c["src"])) == 3 and max(c["src"]) < c["B"]
