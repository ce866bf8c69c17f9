"""The float64 references of tests/pixel_ref.py checked on the CPU: against float64 autograd of the reference expression and a
hand-written gradient, against oracle/losses.py, against the reference's own values in tests/golden/losses.npz; and every entry of
the case tables pinned to the kernel branch it names, computed from the constants the launchers use.  No GPU."""
import re

import numpy as np
import pytest
import torch

import pixel_ref as P
import synth
from oracle import losses as OL

T = torch.from_numpy
F64 = torch.float64
SMALL = [n for n in P.LOSS_CASES if not n.startswith("stride")]


@pytest.mark.parametrize("kernel", P.KERNELS)
@pytest.mark.parametrize("name", ["c2_s2", "c3_s12", "c5_s30", "c16_s12", "short_c4", "short_c16", "oneblock_c4"])
def test_reference_gradient_equals_the_hand_written_one(kernel, name):
    """float64 autograd of the expression == p (g - <g, p>) / npix written out by hand, to float64 rounding."""
    a, second = P.case_inputs(kernel, name)
    loss, grad = P.case_reference(kernel, name)
    hand = P.analytic_grad(kernel, a, second)
    assert torch.isfinite(loss) and bool(torch.isfinite(grad).all())
    assert float((grad - hand).abs().max()) <= 1e-12 * float(grad.abs().max())
    if name == "short_c4":          # and against finite differences of the expression (torch's gradcheck, float64)
        extra = () if kernel == "entropy" else (second if kernel == "kl" else second.to(F64),)
        assert torch.autograd.gradcheck(lambda z: P.EXPR[kernel](z, *extra), (a.to(F64).clone().requires_grad_(True),),
                                        eps=1e-6, atol=1e-8, rtol=1e-5)


@pytest.mark.parametrize("name", ["c4_s2", "c10_s12", "short_c16"])
def test_references_equal_the_oracle(name):
    """pixel_ref's expressions == oracle/losses.py (kl_div on class2one_hot, softmax_mse, kl_div on two softmaxes) in float64."""
    n, h, w, c, _ = P.LOSS_CASES[name]
    a, t = P.case_inputs("kl", name)
    a64 = a.to(F64)
    assert abs(float(P.kl_expr(a64, t)) - float(OL.kl_div(a64.softmax(1), OL.class2one_hot(t, c).to(F64)))) <= 1e-13
    _, b = P.case_inputs("mse", name)
    b64 = b.to(F64)
    assert abs(float(P.mse_expr(a64, b64)) - float(OL.softmax_mse(a64, b64))) <= 1e-15
    assert abs(float(P.klcons_expr(a64, b64)) - float(OL.kl_div(a64.softmax(1), b64.softmax(1)))) <= 1e-13
    p = a64.softmax(1)
    assert abs(float(P.entropy_expr(a64)) - float(-(p * (p + 1e-16).log()).sum(1).mean())) <= 1e-15


def test_references_equal_the_golden_values(golden):
    """The reference project's own numbers (tests/golden/losses.npz, fp32) at the golden shape, to the fp32 rounding of those numbers."""
    g = golden("losses")
    logits = T(synth.normal("kl/logits", (3, 4, 16, 16)))
    target = T(synth.integers("kl/target", (3, 16, 16), 4))
    np.testing.assert_array_equal(OL.class2one_hot(target, 4).numpy(), g["kl/onehot"])
    loss, grad = P.value_and_grad("kl", logits, target)
    np.testing.assert_allclose(float(loss), float(g["kl/loss"]), rtol=1e-6)
    assert float((grad - T(g["kl/glogits"]).to(F64)).abs().max()) <= 2e-6 * float(grad.abs().max())
    a, b = T(synth.normal("mse/a", (3, 4, 16, 16))), T(synth.normal("mse/b", (3, 4, 16, 16)))
    for kernel, key in (("mse", "mse"), ("klcons", "klc")):
        loss, grad = P.value_and_grad(kernel, a, b)
        np.testing.assert_allclose(float(loss), float(g[f"{key}/loss"]), rtol=1e-6)
        assert float((grad - T(g[f"{key}/ga"]).to(F64)).abs().max()) <= 2e-6 * float(grad.abs().max())


@pytest.mark.parametrize("name", list(P.FLIP_CASES))
def test_flip_reference_is_the_oracle_on_the_materialised_flip(name):
    n, h, w, c, masks = P.FLIP_CASES[name]
    a, b = P.case_inputs("mse", name)
    dec = P.masks_to_decisions(masks or [0] * n)
    loss, grad = P.case_reference("mse", name)
    a64 = a.to(F64).requires_grad_(True)
    ref = OL.softmax_mse(a64, OL.apply_flips(b, dec).to(F64))
    ref.backward()
    assert float(loss) == float(ref.detach()) and torch.equal(grad, a64.grad)
    if masks:                       # the masks' bit order: bit 0 = H (dim 2), bit 1 = W (dim 3)
        x = OL.apply_flips(b, dec)
        for i, m in enumerate(masks):
            dims = [d for d, bit in ((1, 1), (2, 2)) if m & bit]
            assert torch.equal(x[i], b[i].flip(dims) if dims else b[i])
        assert sorted(masks) == [0, 1, 2, 3]


def test_fp32_composition_stays_far_inside_the_bounds():
    """The bounds of the GPU tests are the project's 1e-5; an fp32 torch composition of the same expressions stays a factor of ~10
    inside them on these inputs at every class count and scale (1.6e-7 of the loss, 1.1e-6 of max|grad| at worst, recorded in the
    issue that introduced these tests), so the bounds are not an artefact of fp32."""
    worst_l = worst_g = 0.0
    for name in SMALL:
        for kernel in P.KERNELS:
            a, second = P.case_inputs(kernel, name)
            loss, grad = P.case_reference(kernel, name)
            l32, g32 = P.fp32_composition(kernel, a, second)
            el, bl = P.loss_error(float(l32), float(loss))
            eg, bg = P.grad_error(g32, grad)
            worst_l, worst_g = max(worst_l, el / bl), max(worst_g, eg / bg)
    print(f"\nfp32 composition: worst loss error / bound = {worst_l:.3f}, worst gradient error / bound = {worst_g:.3f}")
    assert worst_l <= 0.25 and worst_g <= 0.25


def test_every_loss_case_reaches_the_branch_it_names():
    for name, (n, h, w, c, scale) in P.LOSS_CASES.items():
        assert c in P.CLASS_COUNTS and P.loss_branch(n, h, w) == P.LOSS_CASE_BRANCH[name], name
    sweep = {(c, s) for name, (n, h, w, c, s) in P.LOSS_CASES.items() if (n, h, w) == (3, 19, 23)}
    assert sweep == {(c, s) for c in P.CLASS_COUNTS for s in P.SCALES}
    assert 3 * 19 * 23 == 5 * P.LOSS_THREADS + 31 and P.loss_blocks(3 * 19 * 23) == 6
    assert 1 * 5 * 7 < P.LOSS_THREADS and P.loss_blocks(35) == 1
    assert 16 * 16 == P.LOSS_THREADS and P.loss_blocks(256) == 1
    npix = 2 * 512 * 513
    assert npix == 525312 > P.LOSS_MAX_BLOCKS * P.LOSS_THREADS == 524288 and P.loss_blocks(npix) == P.LOSS_MAX_BLOCKS
    assert {P.LOSS_CASES[n][3] for n in P.LOSS_CASES if P.LOSS_CASE_BRANCH[n] == "grid_stride"} == {2, 4}
    assert {P.LOSS_CASES[n][3] for n in P.LOSS_CASES if P.LOSS_CASE_BRANCH[n] == "short_single_block"} == {4, 16}
    assert not set(P.REFUSED_CLASS_COUNTS) & set(P.CLASS_COUNTS)
    for name, (n, h, w, c, masks) in P.FLIP_CASES.items():
        assert h % 2 == 1 and w % 2 == 1 and n == 4 and c in P.CLASS_COUNTS


def test_the_tables_mirror_the_launchers_constants():
    """The constants above are those of the sources: a change of a block size or a dispatch list has to move the tables with it."""
    import os
    from miseg_amd import _cabi
    csrc = os.path.join(_cabi.PKG_ROOT, "csrc")
    losses, tape = open(os.path.join(csrc, "losses.hip")).read(), open(os.path.join(csrc, "tape.hip")).read()
    shared = open(os.path.join(csrc, "pixel_loss.h")).read()          # the pixel grid and the class-count dispatch of every pixel-loss unit
    assert int(re.search(r"constexpr int kLT = (\d+);", losses).group(1)) == P.LOSS_THREADS and "static_assert(kLT == kPixelThreads" in losses
    assert int(re.search(r"constexpr int kPixelThreads = (\d+);", shared).group(1)) == P.LOSS_THREADS
    assert int(re.search(r"pixel_blocks\(int64_t npix\) \{ return \(int\)std::min<int64_t>\(cdiv\(npix, kPixelThreads\), (\d+)\)", shared).group(1)) == P.LOSS_MAX_BLOCKS
    assert "miseg_loss_ws_bytes(int64_t N, int64_t H, int64_t W) { return (int64_t)pixel_blocks(N * H * W) * 4; }" in losses
    assert "#define MISEG_DISPATCH_C" not in losses and losses.count("const int nb = pixel_blocks(npix);") == 1
    dispatch = shared[shared.index("#define MISEG_DISPATCH_C"):shared.index("default: return fail")]
    assert tuple(int(v) for v in re.findall(r"case (\d+):", dispatch)) == P.CLASS_COUNTS
    assert f"cdiv(H * W, {P.DICE_THREADS}), {P.DICE_MAX_BLOCKS})" in losses
    assert losses.count(f"cdiv(total, {P.CAT_THREADS}), {P.CAT_MAX_BLOCKS})") == 3          # cat_flip, cat_flip_pad, cat_flipped
    assert f"std::min<int64_t>((n16 + 255) / {P.COPY_THREADS}, {P.COPY_MAX_BLOCKS})" in tape
    from miseg_amd import ops
    assert tuple(ops._LOSS_CLASS_COUNTS) == P.CLASS_COUNTS


def test_dice_cat_and_mover_cases_reach_their_branches():
    for name, (n, h, w, c) in P.DICE_CASES.items():
        assert c in P.CLASS_COUNTS
    n, h, w, c = P.DICE_CASES["dice_inner_loop"]
    assert h * w == 16770 > P.DICE_MAX_BLOCKS * P.DICE_THREADS
    assert 19 * 23 > P.DICE_THREADS and (19 * 23) % P.DICE_THREADS                      # more than one block, a partial last one
    na, nb, c, h, w = P.CAT_CASES["cat_grid_stride"]
    assert (na + 2 * nb) * c * h * w > P.CAT_MAX_BLOCKS * P.CAT_THREADS >= (na + nb) * c * h * w     # cat_flip loops there, cat_flipped not yet:
    na, nb, c, h, w = P.CAT_FLIPPED_GRID_STRIDE
    assert (na + nb) * c * h * w > P.CAT_MAX_BLOCKS * P.CAT_THREADS                                  # ... it has a case of its own
    for key in ("cat_2_3_1_5x7", "cat_1_4_2_19x23"):
        na, nb, c, h, w = P.CAT_CASES[key]
        assert h % 2 and w % 2 and nb >= 3
    assert P.CAT_CABI_CASE[0] == 0
    assert P.BYTE_COUNTS[-2] // 16 == P.COPY_MAX_BLOCKS * P.COPY_THREADS and P.BYTE_COUNTS[-2] % 16 == 5       # the full grid, no loop yet
    assert P.BYTE_COUNTS[-1] // 16 > P.COPY_MAX_BLOCKS * P.COPY_THREADS and P.BYTE_COUNTS[-1] % 16 == 5        # the grid-stride loop
    assert {b % 16 for b in P.BYTE_COUNTS} >= {0, 1, 15, 3, 5} and min(P.BYTE_COUNTS) < 16
    assert P.ASSEMBLE_BIG % 4 == 0 and P.ASSEMBLE_BIG // 4 > P.COPY_MAX_BLOCKS * P.COPY_THREADS


def test_argmax_reference_takes_the_first_maximum_and_counts_like_the_oracle():
    z = P.tie_logits("dice/ties", 3, 5, 19, 23)
    first = P.first_argmax(z)
    assert torch.equal(z.max(1)[1], first)                    # torch's CPU argmax == numpy's first maximum on ties, -0.0 == 0.0 included
    tied = (z == z.max(1, keepdim=True)[0]).sum(1) > 1
    assert float(tied.float().mean()) > 0.5                   # ties are the rule
    assert torch.equal(P.first_argmax(torch.tensor([-0.0, 0.0]).view(1, 2, 1, 1)), torch.zeros(1, 1, 1, dtype=torch.int64))
    t = P.labels("dice/t", 3, 19, 23, 5)
    oi, ou = OL.dice_counts(first, t, 5)
    bi, bu = P.dice_bincount(first, t, 5)
    assert torch.equal(oi, bi) and torch.equal(ou, bu)
    t2 = t.clone()
    t2[0, 0, 0], t2[1, 9, 11], t2[2, 18, 22] = -1, 5, 255    # out of range: the prediction still counts, the label nowhere
    bi2, bu2 = P.dice_bincount(first, t2, 5)
    assert int(bu.sum() - bu2.sum()) == 3 and bool((bi2 <= bi).all()) and bool((bu2 <= bu).all())


@pytest.mark.parametrize("bad", [-1, 4, 255])
def test_class2one_hot_refuses_what_the_kernel_flags(bad):
    """The reference raises AssertionError in class2one_hot for a label outside [0, C) -- this project's own port and the oracle's
    restatement do the same --, so ops.softmax_kl's AssertionError for the same labels is the reference's behaviour."""
    from deepclustering2.utils import class2one_hot
    t = P.labels("bad/t", 3, 19, 23, 4)
    class2one_hot(t, 4), OL.class2one_hot(t, 4)
    for pos in ((0, 0, 0), (1, 9, 11), (2, 18, 22)):
        t2 = t.clone()
        t2[pos] = bad
        with pytest.raises(AssertionError):
            class2one_hot(t2, 4)
        with pytest.raises(AssertionError):
            OL.class2one_hot(t2, 4)
    # the float64 reference the GPU test uses: such a pixel adds nothing, the divisor stays npix, its gradient row is zero
    a = P.logits("bad/a", 3, 4, 19, 23, 2)
    t2 = t.clone()
    t2[1, 9, 11] = bad
    loss, grad = P.value_and_grad("kl", a, t2)
    full, _ = P.value_and_grad("kl", a, t)
    p = a.to(F64).softmax(1)
    dropped = -torch.log(p[1, t[1, 9, 11], 9, 11] + 1e-16) / (3 * 19 * 23)
    assert abs(float(full - loss) - float(dropped)) <= 1e-15 and float(grad[1, :, 9, 11].abs().max()) == 0.0


def test_payloads_carry_the_bit_patterns_and_round_differently():
    x = P.bit_payload("payload", (2, 3, 5, 7))
    xi = P.bits(x)
    for pat in P.SPECIAL_BITS[:5]:
        want = pat - (1 << 32) if pat >= (1 << 31) else pat
        assert bool((xi == want).any()) or pat not in (P.SPECIAL_BITS[0], P.SPECIAL_BITS[4])
    assert bool(torch.isnan(x).any()) and torch.equal(P.bits(P.bit_payload("payload", (2, 3, 5, 7), torch.int32)), xi)
    img = P.rounding_image("round", 3, 19, 23)
    trunc = (P.bits(img) >> 16).to(torch.int16)
    rne = P.bits(img.to(torch.bfloat16))
    fin = torch.isfinite(img)
    assert int((trunc != rne)[fin].sum()) > 0                                            # truncation would be seen
    half = img.to(torch.float16)
    assert bool(torch.isinf(half[fin]).any())                                            # finite fp32 above 65504 -> inf
    sub = (half.float().abs() > 0) & (half.float().abs() < 2.0 ** -14)
    assert bool(sub.any()) and bool(torch.isnan(half).any())                             # half denormals, NaN
    for pat in P.ROUNDING_BITS:
        want = pat - (1 << 32) if pat >= (1 << 31) else pat
        assert bool((P.bits(img) == want).any()), hex(pat)
