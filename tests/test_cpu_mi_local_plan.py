"""CPU (no GPU): the case table of tests/mi_local_ref.py against the library's own dispatch.  miseg_iic_local_joint_plan and
miseg_iic_local_bwd_plan report what plan_joint / plan_bwd (csrc/mi_local.h) decide -- the functions miseg_iic_local_joint_fwd and
miseg_iic_local_bwd launch by -- so a kernel variant that exists for some (K, pad) but has no row in VARIANT_CASES fails here, as does
a row that no longer reaches the variant its name states.  Also: the walking shapes do make a block walk, the real-valued inputs can
see an exchange of the displacement axes or of the class axes, and the integer cases stay exact."""
import pytest
import torch

import mi_local_ref as M
from oracle import iic as OI

ALL_CASES = M.VARIANT_CASES + M.BF16_CASES


def _enumerate():
    """Every distinct forward (cap, sb, RB, WB) and backward (kind, width, gInLds, plain_rmw) over K = 1 .. 64, pad = 0 .. 7 at the
    small map, both selectable arithmetics of this table (fp32, plain bf16), with one (K, pad) that reaches it."""
    fwd, bwd = {}, {}
    for k in M.K_ENUM:
        for pad in M.PAD_ENUM:
            jp = M.joint_plan(2, k, 11, 70, pad, 1)
            if jp is not None:
                fwd.setdefault(M.fwd_key(jp), (k, pad))
            for prec in M.PRECISIONS:
                for masked in (False, True):
                    bp = M.bwd_plan(2, k, 11, 70, pad, 1, masked, prec)
                    if bp is not None:
                        bwd.setdefault(M.bwd_key(bp), (k, pad, prec))
    return fwd, bwd


def _table():
    fwd = {M.fwd_key(M.joint_plan(*M.small_shape(k, pad), pad, 1)) for _, k, pad in M.VARIANT_CASES}
    bwd = {M.bwd_key(M.bwd_plan(*M.small_shape(k, pad), pad, 1)) for _, k, pad in M.BWD_CASES}
    bwd |= {M.bwd_key(M.bwd_plan(*M.small_shape(k, pad), pad, 1, False, "bf16")) for _, k, pad in M.BF16_CASES}
    return fwd, bwd


# The rows by name: the GPU file's recorded errors (mi_local_variants.json) are keyed by them, and a row that shares its forward with one
# row and its backward with another would otherwise leave unnoticed.
ROW_NAMES = """f9_sb2_8x64__direct2_lds f9_sb2_8x64_ragged__direct4_glb f9_sb2_4x64__direct4_glb f9_sb2_4x64__direct2_lds
f9_sb2_8x64__direct1_lds f9_sb3_4x64__direct4_glb f9_sb3_4x32__direct4_glb f9_sb4_4x32__direct2_glb f9_sb1_8x64__bwd2x9_atomic f4_sb1_4x64
f9_sb1_4x64 f9_sb2_4x32 f9_sb4_4x32_k64 f9_sb5_4x32 f9_sb6_4x32 f9_sb6_4x16 f9_sb7_4x16 ctl_f9_sb1_8x64__bwd2x9_rmw
ctl_f4_sb1_8x64__bwd2x4_atomic ctl_f4_sb1_8x64__bwd2x4_rmw ctl_f9_sb1_8x64__direct4_lds""".split()


def test_every_variant_the_dispatch_can_select_has_a_row():
    assert sorted(c[0] for c in M.VARIANT_CASES) == sorted(ROW_NAMES)          # no row deleted, none added without its name here
    fwd_all, bwd_all = _enumerate()
    fwd_tab, bwd_tab = _table()
    print(f"\nforward variants {len(fwd_all)}, backward variants {len(bwd_all)}")
    missing_f = {k: v for k, v in fwd_all.items() if k not in fwd_tab}
    missing_b = {k: v for k, v in bwd_all.items() if k not in bwd_tab}
    left_out = (len(missing_f) + len(missing_b)) / float(len(fwd_all) + len(bwd_all))
    assert not missing_f, f"forward (cap, sb, RB, WB) without a row, first reached at (K, pad): {missing_f}"
    assert not missing_b, f"backward (kind, width, gInLds, plain_rmw) without a row, first reached at: {missing_b}"
    assert left_out == 0.0
    # what the table is there for: every family named in csrc/mi_local.hip is in the enumerated set at all
    assert {k[0] for k in fwd_all} == {4, 9} and {k[1] for k in fwd_all} == set(range(1, 8))
    assert {k[2:] for k in fwd_all} == {(8, 64), (4, 64), (4, 32), (4, 16)}
    assert {(M.BWD2, 4, 1, 0), (M.BWD2, 4, 1, 1), (M.BWD2, 9, 1, 0), (M.BWD2, 9, 1, 1)} <= set(bwd_all)
    assert {(M.DIRECT, w, g, 0) for w, g in ((4, 1), (2, 1), (1, 1), (4, 0), (2, 0))} <= set(bwd_all)
    assert (M.ROWS, 1, 0, 0) in bwd_all


def test_no_row_is_redundant_but_the_controls():
    """Every non-control row is the only one that brings some (forward key, backward key) pair: deleting it shrinks what the GPU file
    runs.  (Rows may share a forward or a backward variant -- the pair is what a row is.)"""
    pairs = {}
    for name, k, pad in M.VARIANT_CASES:
        shp = M.small_shape(k, pad)
        key = (M.fwd_key(M.joint_plan(*shp, pad, 1)), M.bwd_key(M.bwd_plan(*shp, pad, 1)) if k <= 32 else None, M.joint_plan(*shp, pad, 1).tps)
        pairs.setdefault(key, []).append(name)
    dup = {k: v for k, v in pairs.items() if len(v) > 1}
    assert not dup, dup


def _describe(name):
    """The variant a row's name states -> (forward key or None, backward key or None)."""
    parts = name.replace("ctl_", "").split("__")
    f = parts[0].split("_")
    rb, wb = (int(v) for v in f[2].split("x"))
    fkey = (int(f[0][1:]), int(f[1][2:]), rb, wb)
    bkey = None
    if len(parts) > 1:
        b = parts[1].split("_")
        if b[0].startswith("direct"):
            bkey = (M.DIRECT, int(b[0][6:]), int(b[1] == "lds"), 0)
        else:
            bkey = (M.BWD2, int(b[0][5:]), 1, int(b[1] == "rmw"))
    return fkey, bkey


@pytest.mark.parametrize("name,k,pad", M.VARIANT_CASES, ids=[c[0] for c in M.VARIANT_CASES])
def test_row_reaches_the_variant_it_is_named_for(name, k, pad):
    fkey, bkey = _describe(name)
    for which in ("small", "walking") if k <= 32 else ("small",):
        n, _, h, w = M.shape_of(k, pad, which)
        for kind in ("whole", "crops"):
            p = len(M.windows(h, w, kind))
            jp = M.joint_plan(n, k, h, w, pad, p)
            assert M.fwd_key(jp) == fkey, (which, kind, jp)
            if "ragged" in name:
                assert (-(-(2 * pad + 1) * k // 16)) % jp.tps != 0      # the last sub-block holds fewer tiles (mtu / ntu < tps)
            bp = M.bwd_plan(n, k, h, w, pad, p, kind == "crops") if k <= 32 else None
            assert M.bwd_key(bp) == bkey, (which, kind, bp)
    if k > 32:
        assert M.bwd_plan(2, k, 11, 70, pad, 1) is None


def test_refusals_and_the_16_bit_selection():
    assert M.joint_plan(2, 20, 11, 70, 3, 0) is None and M.joint_plan(0, 20, 11, 70, 3, 1) is None
    assert M.bwd_plan(2, 33, 11, 70, 0, 1) is None and M.bwd_plan(2, 20, 11, 70, -1, 1) is None
    for _, k, pad in M.BF16_CASES:
        assert M.bwd_plan(2, k, 11, 70, pad, 1, False, "bf16") == M.BwdPlan(M.ROWS, 1, 0, 0, 64)
        assert M.bwd_plan(2, k, 11, 70, pad, 1, True, "bf16").kind == M.BWD2        # a mask sends every arithmetic to the fp32 kernels
    assert M.bwd_plan(2, 21, 11, 70, 3, 1, False, "bf16").kind == M.DIRECT
    from miseg_amd import _cabi
    with pytest.raises(_cabi.MisegError):
        _cabi.query("miseg_iic_local_bwd_plan", 2, 33, 11, 70, 0, 1, 0, 0)
    assert _cabi.query("miseg_iic_local_joint_plan", 2, 20, 11, 70, 3, 1) == 9 | 1 << 8 | 9 << 16 | 8 << 24 | 64 << 32 | 256 << 40
    assert _cabi.query("miseg_iic_local_bwd_plan", 2, 12, 11, 70, 3, 1, 0, 0) == 2 | 9 << 4 | 1 << 8 | 0 << 9 | 58 << 16


@pytest.mark.parametrize("name,k,pad", M.BWD_CASES, ids=[c[0] for c in M.BWD_CASES])
def test_walking_shapes_make_a_block_take_a_second_item_and_key(name, k, pad):
    n, _, h, w = M.walking_shape(k, pad)
    wins = M.windows(h, w, "whole")
    jp, bp = M.joint_plan(n, k, h, w, pad, 1), M.bwd_plan(n, k, h, w, pad, 1)
    assert M.fwd_items(n, h, w, wins, jp) > jp.G, (n, jp)
    assert M.bwd_items(n, wins, bp) > 256, (n, bp)        # 256 blocks walk (direction, window, item): one takes both directions
    crops = M.windows(h, w, "crops")
    bpc = M.bwd_plan(n, k, h, w, pad, 2, True)
    assert M.bwd_items(n, crops, bpc) > 256, (n, bpc)     # ... and, with two windows, more than one window


def _real_cases():
    out = []
    for _, k, pad in ALL_CASES:
        out.append((M.small_shape(k, pad), pad))
    for _, k, pad in M.BWD_CASES + M.BF16_CASES:
        out.append((M.walking_shape(k, pad), pad))
    return sorted(set(out))


@pytest.mark.parametrize("shape,pad", _real_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"p{v}")
def test_real_inputs_can_see_swapped_axes(shape, pad):
    """An exchange of the two displacement axes, or of the two class axes, must move the oracle's joint by more than 1e-2 of its largest
    entry -- 1000 x the bound the kernels are held to -- or the float64 tests could not tell such a kernel from a right one."""
    x, y, _ = M.real_inputs(shape)
    raw = OI.local_joint_raw(x.double(), y.double(), pad)
    top = float(raw.abs().max())
    d_class = float((raw - raw.transpose(2, 3)).abs().max()) / top
    print(f"\n{shape} pad {pad}: class axes {d_class:.2e}", end="")
    assert d_class > 1e-2
    if pad > 0:
        d_disp = float((raw - raw.transpose(0, 1)).abs().max()) / top
        print(f"  displacement axes {d_disp:.2e}")
        assert d_disp > 1e-2


@pytest.mark.parametrize("name,k,pad", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_integer_cases_are_exact_in_fp32_and_bf16(name, k, pad):
    for which in ("small", "walking") if k <= 32 else ("small",):
        shape = M.shape_of(k, pad, which)
        fwd_max, bwd_max = M.int_sum_bounds(shape, pad)
        assert fwd_max < 2 ** 24 and bwd_max < 2 ** 23          # 2^23: the scale 0.5 leaves halves
        d = M.int_inputs(shape, pad, 2)
        for key, lo, hi in (("x", 0, 3), ("y", 0, 3), ("G", -3, 3), ("mask", 0, 1), ("prefill_x", -4, 4), ("prefill_y", -4, 4)):
            t = d[key]
            assert torch.equal(t, t.round()) and float(t.min()) >= lo and float(t.max()) <= hi
            assert float(t.min()) == lo and float(t.max()) == hi                      # the whole range is used
            assert torch.equal(M.to_bf16(t), t)                                       # exact as a bf16 operand
    # and the float64 oracle on them is an integer below the bound
    shape = M.small_shape(k, pad)
    d = M.int_inputs(shape, pad, 2)
    wins = M.windows(shape[2], shape[3], "crops")
    raw = M.ref_joint(d["x"], d["y"], pad, wins, d["mask"])
    assert torch.equal(raw, raw.round()) and float(raw.abs().max()) <= M.int_sum_bounds(shape, pad)[0]
    assert torch.equal(raw.to(torch.float32).double(), raw)
