"""Replay equals eager, for every entry point that records itself on the launch tape (csrc/tape.h).

One case per taped entry point and storage type / precision / dispatch branch: the call runs eagerly while a tape records it,
its outputs are poisoned and its in-place state restored, the tape is replayed, and every output must have the eager bits
(tests/tape_harness.py).  A ``MISEG_TAPE`` line with two same-typed arguments swapped, an entry point that reads a host array
during the call, a wrapper that needs an ATen fill: each leaves the eager call right and only this comparison wrong.  Hence
non-square maps, N >= 2, Cin != Cout, and a distinct buffer with distinct content behind every pointer argument.

A case names the arguments of ONE C-ABI call by parameter name; the parsed signature (tests/test_cpu_tape_table.py) puts them in
order and says which pointers are read (``const``: inputs) and which are written (outputs, poisoned before the replay).  ``inout``
lists written pointers that carry state or that the call writes only in part; ``ws``-like scratch is neither compared nor kept.
Shapes are the smallest of the kernel's own reference tables (exact_ref.py, exact_heads.py, heads_var_ref.py, pixel_ref.py, ...),
one of H, W moved where the table is square.

Order-dependent (float atomics; compared at the bound of the kernel's float64 test instead of bit for bit):
  miseg_iic_local_bwd at K = 4 -- local_bwd2_kernel adds with atomicAdd when K divides 4, 8 or 12 (the `!plain_rmw` branch).
"""
import ctypes
import struct
import zlib
from typing import Callable, Dict, List

import pytest
import torch

import test_cpu_tape_table as TABLE
from test_gpu_mi import LOCAL_BWD_ATOL          # of max|g|, rtol = 0: the bound of the local-MI gradients against float64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
TWO = (F32, BF16)
ALL = (F32, BF16, F16)
HALF = (BF16, F16)

EXCLUDED: Dict[str, str] = {}
CASES: Dict[str, Callable] = {}
VARIANTS: Dict[str, tuple] = {}
RECORDED: set = set()
ORDER_DEPENDENT: List[str] = []
_G = torch.Generator()


def _abi():
    from miseg_amd import _cabi
    return _cabi


def _H():
    import tape_harness
    return tape_harness


def DT(dtype) -> int:
    return {F32: 0, BF16: 1, F16: 2}[dtype]


def q(name, *args) -> int:
    return _abi().query(name, *args)


def st() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- operands: distinct content everywhere, from one seeded generator per case
def rn(*shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=_G) * scale).to(dtype).to(DEV)


def ru(*shape, lo=0.5, hi=1.5):
    return (torch.rand(*shape, generator=_G) * (hi - lo) + lo).to(DEV)


def ri(lo, hi, *shape, dtype=I64):
    return torch.randint(lo, hi, shape, generator=_G).to(dtype).to(DEV)


def ints(vals, dtype=I32):
    return torch.tensor(vals, dtype=dtype).to(DEV)


def simplex(*shape, dim):
    return torch.softmax(torch.randn(*shape, generator=_G) * 2.0, dim).contiguous().to(DEV)


def ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=U8, device=DEV)


def zeros(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def out(*shape, dtype=F32):
    return torch.empty(*shape, dtype=dtype, device=DEV)


def shuffled(t):
    """Same shape, strides and value range, other content: what a rebinding replays with."""
    flat = t.detach().cpu().flatten()
    return flat[torch.randperm(flat.numel(), generator=_G)].view(t.shape).to(t.device)


SCRATCH = ("ws", "dz_ws", "dpool_ws")


def abi_case(name, args: dict, inout=(), scratch=SCRATCH, rebind=None, order_dependent=False, reason="", close=None, loose=()):
    """A Case for one call of entry point ``name`` with the arguments ``args`` (by parameter name; the stream is filled in)."""
    H = _H()
    ep = TABLE.EPS[name]
    assert ep.params[0] == "stream" and set(args) == set(ep.params[1:]), (name, sorted(set(args) ^ set(ep.params[1:])))
    inputs, state, outputs, keep = {}, {}, {}, []
    for p, ty in zip(ep.params[1:], ep.types[1:]):
        v = args[p]
        if "*" not in ty:
            assert not isinstance(v, torch.Tensor), (name, p)
            continue
        if v is None:
            continue
        assert isinstance(v, torch.Tensor), (name, p)
        if p in scratch:
            keep.append(v)
        elif p in inout:
            state[p] = v
        elif "const" in ty:
            inputs[p] = v
        else:
            outputs[p] = v
    every = list(inputs.values()) + list(state.values()) + list(outputs.values()) + keep
    assert len({t.data_ptr() for t in every}) == len(every), f"{name}: two pointer arguments share a buffer"
    assert not set(inout) - set(state), (name, set(inout) - set(state))

    def call(T):
        vals = [st()]
        for p in ep.params[1:]:
            v = T.get(p, args[p])
            vals.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
        _abi().call(name, *vals)

    alt = shuffled(inputs[rebind]) if rebind else None
    case = H.Case(call=call, inputs=inputs, inout=state, outputs=outputs, rebind=rebind, alt=alt, order_dependent=order_dependent,
                  reason=reason, close=close, loose=loose, expect=(name,))
    case.keep_alive = keep
    return case


def case(name, variants=(None,)):
    def deco(fn):
        CASES[name] = fn
        VARIANTS[name] = tuple(variants)
        return fn
    return deco


# =================================================================================================================== tape.hip, api.hip
@case("miseg_fill_zero")
def _(v):
    return abi_case("miseg_fill_zero", dict(dst=out(1000, dtype=U8), nbytes=1000))


@case("miseg_copy")
def _(v):
    return abi_case("miseg_copy", dict(dst=out(1000, dtype=U8), src=ri(0, 255, 1000, dtype=U8), nbytes=1000), rebind="src")


@case("miseg_gather_rows")
def _(v):
    return abi_case("miseg_gather_rows", dict(src=rn(2, 5, 4), dst=out(2, 3, 4), outer=2, n_src=5, n_idx=3, idx=ints([4, 0, 2]), chunk=4), rebind="src")


@case("miseg_assemble_rows")
def _(v):
    return abi_case("miseg_assemble_rows", dict(out=out(24), src0=rn(8), scale0=ru(1), numel0=8, src1=rn(4), scale1=None, numel1=4,
                                                src2=None, scale2=ru(1), numel2=12), rebind="src1")


def _staging(v):
    """miseg_upload, miseg_download and miseg_event_record as the step uses them: pinned block up, results down, an event after them."""
    H, lib = _H(), _abi().lib()
    n = 4096
    src = torch.randint(0, 255, (n,), dtype=U8, generator=_G).pin_memory()
    back = torch.zeros(n, dtype=U8).pin_memory()
    dev = out(n, dtype=U8)
    ev = lib.miseg_event_create()
    assert ev

    def call(T):
        _abi().call("miseg_upload", st(), T["dev"].data_ptr(), T["src"].data_ptr(), n)
        _abi().call("miseg_download", st(), T["back"].data_ptr(), T["dev"].data_ptr(), n)
        _abi().call("miseg_event_record", st(), ev)

    c = H.Case(call=call, inputs={"src": src}, outputs={"dev": dev, "back": back}, rebind="src", alt=shuffled(src).pin_memory(),
               expect=("miseg_upload", "miseg_download", "miseg_event_record"))
    c.after = lambda: (torch.cuda.synchronize(), lib.miseg_event_destroy(ev))
    return c


for _n in ("miseg_upload", "miseg_download", "miseg_event_record"):
    case(_n)(_staging)


@case("miseg_stream_wait_stream")
def _(v):
    """A copy on a side stream, the wait, and a copy of its result on the caller's stream."""
    H = _H()
    a, b, c = rn(256), out(256), out(256)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call(T):
        _abi().call("miseg_copy", side.cuda_stream, T["b"].data_ptr(), T["a"].data_ptr(), 1024)
        _abi().call("miseg_stream_wait_stream", st(), side.cuda_stream)
        _abi().call("miseg_copy", st(), T["c"].data_ptr(), T["b"].data_ptr(), 1024)

    cs = H.Case(call=call, inputs={"a": a}, outputs={"b": b, "c": c}, rebind="a", alt=shuffled(a), expect=("miseg_stream_wait_stream", "miseg_copy"))
    cs.keep_alive = [side]
    return cs


# =================================================================================================================== losses.hip, dice.hip
LOSS = (3, 19, 23)              # pixel_ref.LOSS_CASES: N, H, W


def _loss_common(c):
    n, h, w = LOSS
    return dict(N=n, H=h, W=w, C=c, upstream=ru(1), loss=out(1), ws=ws(q("miseg_loss_ws_bytes", n, h, w)), ws_bytes=max(q("miseg_loss_ws_bytes", n, h, w), 16))


@case("miseg_softmax_kl")
def _(v):
    n, h, w = LOSS
    return abi_case("miseg_softmax_kl", dict(logits=rn(n, h, w, 4, scale=3.0), labels=ri(0, 4, n, h, w), glogits=out(n, h, w, 4), bad_label=zeros(1, dtype=I32),
                                             **_loss_common(4)), inout=("bad_label",), rebind="labels")


@case("miseg_softmax_mse")
def _(v):
    n, h, w = LOSS
    return abi_case("miseg_softmax_mse", dict(a=rn(n, h, w, 5, scale=3.0), b=rn(n, h, w, 5, scale=3.0), flips=ints([1, 2, 3]), ga=out(n, h, w, 5), **_loss_common(5)),
                    rebind="b")


@case("miseg_softmax_klcons")
def _(v):
    n, h, w = LOSS
    return abi_case("miseg_softmax_klcons", dict(a=rn(n, h, w, 3, scale=3.0), b=rn(n, h, w, 3, scale=3.0), flips=ints([2, 0, 1]), ga=out(n, h, w, 3), **_loss_common(3)),
                    rebind="a")


@case("miseg_softmax_entropy")
def _(v):
    n, h, w = LOSS
    return abi_case("miseg_softmax_entropy", dict(logits=rn(n, h, w, 6, scale=3.0), glogits=out(n, h, w, 6), **_loss_common(6)), rebind="logits")


@case("miseg_softmax_dice")
def _(v):
    n, c, h, w = 2, 16, 5, 7            # dice_ref.SHAPES
    nb = q("miseg_softmax_dice_ws_bytes", n, h, w, c)
    return abi_case("miseg_softmax_dice", dict(logits=rn(n, h, w, c, scale=3.0), labels=ri(0, c, n, h, w), N=n, H=h, W=w, C=c, pow=2, eps=1e-8, class_weight=ru(c),
                                               kl_weight=0.25, dice_weight=0.75, upstream=ru(1), loss=out(1), glogits=out(n, h, w, c),
                                               bad_label=zeros(1, dtype=I32), ws=ws(nb), ws_bytes=max(nb, 16)), inout=("bad_label",), rebind="logits")


@case("miseg_cat_flip")
def _(v):
    na, nb, c, h, w = 2, 3, 1, 5, 7     # pixel_ref.CAT_CASES
    return abi_case("miseg_cat_flip", dict(a=rn(na, c, h, w), Na=na, b=rn(nb, c, h, w), Nb=nb, C=c, H=h, W=w, flips=ints([1, 2, 3]), out=out(na + 2 * nb, c, h, w)),
                    rebind="b")


@case("miseg_cat_flipped")
def _(v):
    na, nb, c, h, w = 1, 4, 2, 19, 23
    return abi_case("miseg_cat_flipped", dict(a=rn(na, c, h, w), Na=na, b=rn(nb, c, h, w), Nb=nb, C=c, H=h, W=w, flips=ints([1, 2, 3, 0]), out=out(na + nb, c, h, w)),
                    rebind="a")


@case("miseg_cat_flip_pad", HALF)
def _(v):
    na, nb, h, w = 2, 3, 5, 7
    return abi_case("miseg_cat_flip_pad", dict(a=rn(na, 1, h, w), Na=na, b=rn(nb, 1, h, w), Nb=nb, H=h, W=w, flips=ints([3, 1, 2]), out=out(na + 2 * nb, 1, h, w),
                                               dt_pad=DT(v), pad8=out(na + 2 * nb, h, w, 8, dtype=v)), rebind="b")


@case("miseg_argmax_dice")
def _(v):
    n, h, w, c = 3, 19, 23, 4
    return abi_case("miseg_argmax_dice", dict(logits=rn(n, h, w, c), labels=ri(0, c, n, h, w), N=n, H=h, W=w, C=c, pred=out(n, h, w, dtype=I64),
                                              inter=out(n, c, dtype=I64), uni=out(n, c, dtype=I64)), rebind="labels")


@case("miseg_simplex_violations")
def _(v):
    x = simplex(3, 5, 7, dim=1)
    x[1, :, 2] += 0.25                  # one position off the simplex
    return abi_case("miseg_simplex_violations", dict(x=x, outer=3, C=5, inner=7, tol=1e-3, count=ints([11])), inout=("count",), rebind="x")


@case("miseg_report_scalars")
def _(v):
    r, c = 2, 4
    flat = rn(c + 6)
    flat[c + 2] = float("nan")
    desc = ints([[0, 1, 0], [1, c, 6], [2, 1, 0]])
    return abi_case("miseg_report_scalars", dict(flat=flat, iflat=ints([0, 5, 0]), coeff=rn(r, c), R=r, C=c, desc=desc, ncheck=3, out=out(r + 3)), rebind="flat")


@case("miseg_flip")
def _(v):
    """Through the ctypes stride arrays of the C ABI (the wrapper's host tensors are the same thing): channels_last in, contiguous out."""
    H = _H()
    shape = (2, 3, 5, 7)
    x = rn(*shape).contiguous(memory_format=torch.channels_last)
    o = out(*shape)
    flips = ints([1, 2])
    ost = (ctypes.c_int64 * 4)(*o.stride())
    box = {}

    def call(T):
        t = T["x"]
        box["is"] = (ctypes.c_int64 * 4)(*t.stride())
        _abi().call("miseg_flip", st(), t.data_ptr(), T["o"].data_ptr(), *shape, box["is"], ost, 4, T["flips"].data_ptr())
        for i in range(4):
            box["is"][i] = 0            # the caller's array does not outlive the call

    return H.Case(call=call, inputs={"x": x, "flips": flips}, outputs={"o": o}, rebind="x",
                  alt=rn(*shape).contiguous(memory_format=torch.channels_last), expect=("miseg_flip",))


# =================================================================================================================== optim.hip, ema.hip
def _optim(name, hyper_n, extra=None, guard=True):
    n = 1000
    args = dict(param=rn(n), grad=rn(n), exp_avg=rn(n, scale=0.1), exp_avg_sq=ru(n, lo=0.01, hi=0.1), numel=n, beta1=0.9, beta2=0.999,
                hyper=ints(([1e-3, 1e-4, 1e-8, 1e-5, 0.5, 0.1] if hyper_n == 6 else [1e-3, 1.0, 1e-8, 1e-5, 0.5])[:hyper_n], dtype=F32))
    if guard:
        args.update(grad_scale=2.0, guard=zeros(3), nguard=3)
    args.update(extra or {})
    st_ = tuple(k for k in ("param", "exp_avg", "exp_avg_sq", "max_exp_avg_sq") if args.get(k) is not None and k in TABLE.EPS[name].params)
    return abi_case(name, args, inout=st_, rebind="grad")


@case("miseg_adam_step")
def _(v):
    return _optim("miseg_adam_step", 4, guard=False)


@case("miseg_adam_step_scaled")
def _(v):
    return _optim("miseg_adam_step_scaled", 4, dict(grad_scale=4.0), guard=False)


@case("miseg_adam_step_guarded")
def _(v):
    return _optim("miseg_adam_step_guarded", 5, dict(grad_scale=-1.0))


@case("miseg_radam_step")
def _(v):
    return _optim("miseg_radam_step", 5)


@case("miseg_adabound_step", (0, 1))
def _(v):
    return _optim("miseg_adabound_step", 6, dict(max_exp_avg_sq=ru(1000, lo=0.01, hi=0.2), decoupled=v))


@case("miseg_count_nonfinite")
def _(v):
    g = rn(1000)
    g[17], g[500] = float("nan"), float("inf")
    return abi_case("miseg_count_nonfinite", dict(grad=g, numel=1000, count=out(1)), rebind="grad")


@case("miseg_ema_update")
def _(v):
    return abi_case("miseg_ema_update", dict(teacher=rn(1000), student=rn(1000), numel=1000, coef=ints([0.99, 0.01, 0.999], dtype=F32), guard=zeros(2), nguard=2),
                    inout=("teacher",), rebind="student")


# =================================================================================================================== vat.hip
@case("miseg_l2_perturb")
def _(v):
    n, m = 3, 19 * 23
    nb = q("miseg_l2_perturb_ws_bytes", n, m)
    return abi_case("miseg_l2_perturb", dict(g=rn(n, m), x=rn(n, m), scale=ru(n), N=n, M=m, out=out(n, m), r=out(n, m), d=out(n, m), flag=zeros(1, dtype=I32),
                                             ws=ws(nb), ws_bytes=max(nb, 16)), inout=("flag",), rebind="x")


@case("miseg_normal_fill")
def _(v):
    return abi_case("miseg_normal_fill", dict(seed=20261020, offset=7, out=out(1001), numel=1001))


@case("miseg_philox_fill")
def _(v):
    return abi_case("miseg_philox_fill", dict(seed=20261020, offset=5, out=out(1003, dtype=I32), numel=1003))


# =================================================================================================================== affine, components, surface, augment
@case("miseg_affine_warp_fwd", ((0, 0), (0, 1), (1, 0), (1, 1)))
def _(v):
    cl, mode = v
    h, w, c, n = 9, 7, 5, 2             # affine_ref.SHAPES
    theta = ints([[[0.9, 0.2, 0.05], [-0.1, 1.1, -0.03]], [[1.0, -0.3, 0.1], [0.25, 0.8, 0.0]]], dtype=F32)
    shape = (n, h, w, c) if cl else (n, c, h, w)
    return abi_case("miseg_affine_warp_fwd", dict(x=rn(*shape), theta=theta, N=n, C=c, H=h, W=w, channels_last=cl, mode=mode, y=out(*shape)), rebind="x")


@case("miseg_affine_warp_bwd", ((0, 0), (0, 1), (1, 0), (1, 1)))
def _(v):
    cl, mode = v
    h, w, c, n = 9, 7, 5, 2
    theta = ints([[[0.9, 0.2, 0.05], [-0.1, 1.1, -0.03]], [[1.0, -0.3, 0.1], [0.25, 0.8, 0.0]]], dtype=F32)
    shape = (n, h, w, c) if cl else (n, c, h, w)
    return abi_case("miseg_affine_warp_bwd", dict(gy=rn(*shape), theta=theta, N=n, C=c, H=h, W=w, channels_last=cl, mode=mode, reach=8, gx=out(*shape)), rebind="gy")


def _blobs(n, h, w, classes=4):
    """Class-coded masks with a few rectangles per class."""
    m = torch.zeros(n, h, w, dtype=I64)
    for i in range(n):
        for c in range(1, classes):
            for _ in range(2):
                y0, x0 = int(torch.randint(0, h - 4, (1,), generator=_G)), int(torch.randint(0, w - 4, (1,), generator=_G))
                m[i, y0:y0 + int(torch.randint(2, 8, (1,), generator=_G)), x0:x0 + int(torch.randint(2, 8, (1,), generator=_G))] = c
    return m.to(DEV)


@case("miseg_largest_component", ((2, 1), (3, 2)))
def _(v):
    rank, conn = v
    n, h, w, c = 3, 24, 40, 4           # component_ref.GPU_SHAPES
    nb = q("miseg_largest_component_ws_bytes", n, h, w, 2, rank)
    u = n if rank == 2 else 1
    return abi_case("miseg_largest_component", dict(pred=_blobs(n, h, w), N=n, H=h, W=w, classes=ints([3, 1]), n_classes=2, rank=rank, connectivity=conn, fill=0,
                                                    out=out(n, h, w, dtype=I64), labels=out(n, h, w, dtype=I32), stats=out(u, 2, 3, dtype=I64), target=_blobs(n, h, w),
                                                    C=c, inter=out(n, c, dtype=I64), uni=out(n, c, dtype=I64), ws=ws(nb), ws_bytes=max(nb, 16)), rebind="pred")


@case("miseg_surface_stats")
def _(v):
    n, h, w = 3, 24, 40                 # surface_ref.SHAPES
    nb = q("miseg_surface_stats_ws_bytes", n, h, w, 2)
    return abi_case("miseg_surface_stats", dict(pred=_blobs(n, h, w), target=_blobs(n, h, w), N=n, H=h, W=w, classes=ints([2, 1]), n_classes=2, q=0.95,
                                                stats=out(n, 2, 2, 4, dtype=I64), sum_dist=out(n, 2, 2, dtype=torch.float64), ws=ws(nb), ws_bytes=max(nb, 16)),
                    rebind="target")


@case("miseg_augment_slices")
def _(v):
    """Two jobs on a 3-slice atlas: a crop and a horizontal flip (job layout: include/miseg_hip.h, MISEG_AUG_*)."""
    ns, sh, sw, oh, ow = 3, 12, 20, 8, 16
    jobs = torch.zeros(2, 48, dtype=I32)
    jobs[0, 0], jobs[0, 3] = 2, 1
    jobs[0, 12:21] = torch.tensor([1, 2, 3, 0, 0, 0, 0, sw, sh])            # crop top 2, left 3
    jobs[1, 0], jobs[1, 3] = 1, 2
    jobs[1, 12:21] = torch.tensor([1, 1, 1, 0, 0, 0, 0, sw, sh])
    jobs[1, 21:30] = torch.tensor([3, 0, 0, 0, 0, 0, 0, ow, oh])            # then a horizontal flip of the cropped image
    return abi_case("miseg_augment_slices", dict(atlas_img=ri(0, 256, ns, sh, sw, dtype=U8), atlas_gt=ri(0, 4, ns, sh, sw, dtype=U8), n_slices=ns, slice_h=sh, slice_w=sw,
                                                 jobs_dev=jobs.to(DEV), njobs=2, out_h=oh, out_w=ow, img_out=out(2, oh, ow), gt_out=out(2, oh, ow, dtype=I64)),
                    rebind="atlas_img")


# =================================================================================================================== supcon, contrast, contrast_decoder
@case("miseg_supcon")
def _(v):
    b, views, d = 3, 2, 8
    n = b * views
    nb = q("miseg_supcon_ws_bytes", n, d)
    return abi_case("miseg_supcon", dict(e=rn(n, d), N=n, D=d, V=views, labels=ints([1, 0, 1]), temperature=0.07, base_temperature=0.1, upstream=ru(1), loss=out(1),
                                         ge=out(n, d), ws=ws(nb), ws_bytes=max(nb, 16)), rebind="e")


@case("miseg_avgpool_fwd", ALL)
def _(v):
    n, h, w, c = 2, 5, 7, 24
    return abi_case("miseg_avgpool_fwd", dict(dt=DT(v), feat=rn(n, h, w, c, dtype=v), N=n, H=h, W=w, C=c, pooled=out(n, c)), rebind="feat")


@case("miseg_avgpool_bwd", TWO)
def _(v):
    n, h, w, c = 2, 5, 7, 24
    return abi_case("miseg_avgpool_bwd", dict(dt=DT(v), g=rn(n, c), N=n, H=h, W=w, C=c, gfeat=out(n, h, w, c, dtype=v)), rebind="g")


@case("miseg_bias_lrelu_fwd", ALL)
def _(v):
    n, h, w, c = 2, 5, 7, 24
    return abi_case("miseg_bias_lrelu_fwd", dict(dt=DT(v), raw=rn(n, h, w, c, dtype=v), N=n, H=h, W=w, C=c, bias=rn(c), slope=0.01, y=out(n, h, w, c, dtype=v)), rebind="raw")


@case("miseg_bias_lrelu_bwd", TWO)
def _(v):
    n, h, w, c = 2, 5, 7, 24
    nb = q("miseg_bias_lrelu_bwd_ws_bytes", DT(v), n, h, w, c)
    return abi_case("miseg_bias_lrelu_bwd", dict(dt=DT(v), y=rn(n, h, w, c, dtype=v), gy=rn(n, h, w, c, dtype=v), N=n, H=h, W=w, C=c, slope=0.01,
                                                 gx=out(n, h, w, c, dtype=v), gbias=out(c), ws=ws(nb), ws_bytes=max(nb, 16)), rebind="gy")


AMAX = dict(N=6, H=11, W=14, C=8, OH=4, OW=5, PH=2, PW=1, V=3)


@case("miseg_bias_amaxpool_fwd", TWO)
def _(v):
    a = AMAX
    bh, bw = a["OH"] // a["PH"], a["OW"] // a["PW"]
    return abi_case("miseg_bias_amaxpool_fwd", dict(dt=DT(v), raw=rn(a["N"], a["H"], a["W"], a["C"], dtype=v), bias=rn(a["C"]),
                                                    e=out(a["N"] * a["PH"] * a["PW"], a["C"] * bh * bw), idx=out(a["N"], a["OH"], a["OW"], a["C"], dtype=I32), **a), rebind="raw")


@case("miseg_bias_amaxpool_bwd", TWO)
def _(v):
    a = AMAX
    bh, bw = a["OH"] // a["PH"], a["OW"] // a["PW"]
    idx = (ri(0, a["H"] * a["W"], a["N"], a["OH"], a["OW"], a["C"], dtype=I32))
    return abi_case("miseg_bias_amaxpool_bwd", dict(dt=DT(v), ge=rn(a["N"] * a["PH"] * a["PW"], a["C"] * bh * bw), idx=idx,
                                                    graw=out(a["N"], a["H"], a["W"], a["C"], dtype=v), gbias=out(a["C"]), **a), rebind="ge")


# =================================================================================================================== mi_global.hip
GS, GN, GK = 3, 6, 5


@case("miseg_iic_global_fwd")
def _(v):
    return abi_case("miseg_iic_global_fwd", dict(x=simplex(GS, GN, GK, dim=2), y=simplex(GS, GN, GK, dim=2), S=GS, N=GN, K=GK, lamb=1.5, loss=out(GS), loss_no_lamb=out(GS),
                                                 joint=out(GS, GK, GK)), rebind="x")


@case("miseg_iic_global_bwd")
def _(v):
    return abi_case("miseg_iic_global_bwd", dict(x=simplex(GS, GN, GK, dim=2), y=simplex(GS, GN, GK, dim=2), S=GS, N=GN, K=GK, lamb=1.5, upstream=ru(GS),
                                                 gx=out(GS, GN, GK), gy=out(GS, GN, GK)), rebind="y")


@case("miseg_iic_global_fwd_pair")
def _(v):
    return abi_case("miseg_iic_global_fwd_pair", dict(prob=simplex(GS, 2 * GN, GK, dim=2), S=GS, N=GN, K=GK, lamb=1.5, loss=out(GS), loss_no_lamb=out(GS),
                                                      joint=out(GS, GK, GK)), rebind="prob")


@case("miseg_iic_global_bwd_pair")
def _(v):
    return abi_case("miseg_iic_global_bwd_pair", dict(prob=simplex(GS, 2 * GN, GK, dim=2), S=GS, N=GN, K=GK, lamb=1.5, upstream=ru(GS), gprob=out(GS, 2 * GN, GK)), rebind="prob")


@case("miseg_iic_global_joint_fwd", (0, 1))
def _(v):
    return abi_case("miseg_iic_global_joint_fwd", dict(x=simplex(GS, GN, GK, dim=2), y=simplex(GS, GN, GK, dim=2), S=GS, N=GN, K=GK, symmetric=v, joint=out(GS, GK, GK)), rebind="x")


@case("miseg_iic_global_joint_bwd", (0, 1))
def _(v):
    return abi_case("miseg_iic_global_joint_bwd", dict(x=simplex(GS, GN, GK, dim=2), y=simplex(GS, GN, GK, dim=2), S=GS, N=GN, K=GK, symmetric=v, joint=ru(GS, GK, GK),
                                                       gjoint=rn(GS, GK, GK), gx=out(GS, GN, GK), gy=out(GS, GN, GK)), rebind="y")


# =================================================================================================================== mi_local.hip, mi_out.hip
# (K, H, W, pad): fp32 at the smallest admissible shape (test_gpu_mi.LOCAL_CASES[0]); K = 20, pad = 3 at _PLANE_CASES[0] for the 16-bit paths
MI_SMALL = (5, 12, 10, 2)
MI_K20 = (20, 24, 40, 3)
PREC = {"fp32": 0, "bf16x3": 1, "f16f8": 3}


def _mi(k, h, w, pad, n, p_windows):
    t = 2 * pad + 1
    win = ints(p_windows).view(len(p_windows), 4)
    return t, win, len(p_windows)


def _close_atol(k, want, got):
    tol = LOCAL_BWD_ATOL * float(want.abs().max())
    err = float((want - got).abs().max())
    assert err <= tol, f"{k}: |replay - eager| = {err:.3e} > {tol:.3e}"


@case("miseg_iic_local_joint_fwd", (("fp32", MI_SMALL, True), ("fp32", MI_K20, False), ("bf16x3", MI_K20, False), ("f16f8", MI_K20, False)))
def _(v):
    prec, (k, h, w, pad), masked = v
    n = 2
    t, win, P = _mi(k, h, w, pad, n, [(0, h, 0, w)])
    nb = q("miseg_iic_local_joint_ws_bytes", n, k, h, w, pad, P)
    return abi_case("miseg_iic_local_joint_fwd", dict(x=simplex(n, k, h, w, dim=1), y=simplex(n, k, h, w, dim=1), mask=ru(n, 1, h, w, lo=0.0, hi=1.0) if masked else None,
                                                      N=n, K=k, H=h, W=w, pad=pad, win=win, P=P, raw=out(P, t, t, k, k), ws=ws(nb), ws_bytes=max(nb, 16),
                                                      precision=PREC[prec]), rebind="x")


@case("miseg_iic_local_loss_fwd")
def _(v):
    k, pad, P = 5, 1, 2
    return abi_case("miseg_iic_local_loss_fwd", dict(raw=ru(P, 3, 3, k, k, lo=0.1, hi=2.0), K=k, pad=pad, P=P, lamda=1.5, loss=out(P), grad_raw=out(P, 3, 3, k, k)), rebind="raw")


@case("miseg_iic_local_loss_fwd_ws")
def _(v):
    k, pad, P = 5, 2, 2
    nb = q("miseg_iic_local_loss_ws_bytes", pad, P)
    return abi_case("miseg_iic_local_loss_fwd_ws", dict(raw=ru(P, 5, 5, k, k, lo=0.1, hi=2.0), K=k, pad=pad, P=P, lamda=1.5, loss=out(P), grad_raw=out(P, 5, 5, k, k),
                                                        ws=ws(nb), ws_bytes=max(nb, 16)), rebind="raw")


@case("miseg_iic_local_bwd", (("fp32", MI_SMALL, "store"), ("fp32", MI_SMALL, "masked_acc"), ("fp32", (4, 12, 10, 2), "atomic"), ("fp32", MI_K20, "store"),
                              ("fp32", (24, 12, 10, 1), "store"), ("fp32", (5, 12, 10, 4), "acc"), ("bf16x3", MI_K20, "store"), ("f16f8", MI_K20, "acc")))
def _(v):
    """fp32: local_bwd2_kernel<4> (K = 5, 4) and <9> (K = 20, pad = 3), and the direct form behind them -- local_bwd_kernel, after two
    hipMemsetAsync when it stores -- for more than 20 channels (K = 24) and for a source tile of more than 10 rows (pad = 4); it adds
    without atomics, one writer per element.  16-bit: the row kernels."""
    prec, (k, h, w, pad), form = v
    n = 2
    whole = form in ("store", "atomic")
    t, win, P = _mi(k, h, w, pad, n, [(0, h, 0, w)] if whole else [(0, h // 2, 0, w), (h // 2, h, 2, w)])
    nb = q("miseg_iic_local_bwd_ws_bytes", k, pad, P)
    gx, gy = (out(n, k, h, w), out(n, k, h, w)) if whole else (rn(n, k, h, w), rn(n, k, h, w))
    args = dict(x=simplex(n, k, h, w, dim=1), y=simplex(n, k, h, w, dim=1), mask=ru(n, 1, h, w, lo=0.0, hi=1.0) if form == "masked_acc" else None, N=n, K=k, H=h, W=w,
                pad=pad, win=win, P=P, grad_raw=rn(P, t, t, k, k), scale=ru(P), gx=gx, gy=gy, accumulate=0 if whole else 1, precision=PREC[prec], ws=ws(nb),
                ws_bytes=max(nb, 16))
    if form == "atomic":
        ORDER_DEPENDENT.append("miseg_iic_local_bwd[K=4]")
        return abi_case("miseg_iic_local_bwd", args, rebind="x", order_dependent=True, close=_close_atol, loose=("gx", "gy"),
                        reason="local_bwd2_kernel adds its col2im rows with atomicAdd when K divides 4, 8 or 12 (!plain_rmw)")
    return abi_case("miseg_iic_local_bwd", args, inout=() if whole else ("gx", "gy"), rebind="x")


def _heads(k, h, w, pad, ub=2):
    s = 4 if pad == 3 else 3            # S, UB, pad and P pairwise distinct
    t, win, P = _mi(k, h, w, pad, ub, [(0, h, 0, w)])
    return s, ub, t, win, P, simplex(s, 2 * ub, k, h, w, dim=2)


@case("miseg_iic_local_joint_fwd_heads", (("fp32", MI_SMALL), ("bf16x3", MI_K20), ("f16f8", MI_K20)))
def _(v):
    prec, (k, h, w, pad) = v
    s, ub, t, win, P, probs = _heads(k, h, w, pad)
    nb = max(q("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, P * s), q("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, P))
    return abi_case("miseg_iic_local_joint_fwd_heads", dict(probs=probs, S=s, UB=ub, K=k, H=h, W=w, pad=pad, win=win, P=P, raw=out(s, P, t, t, k, k), ws=ws(nb),
                                                            ws_bytes=max(nb, 16), precision=PREC[prec]), rebind="probs")


@case("miseg_iic_local_bwd_heads", (("fp32", MI_SMALL, 0), ("fp32", MI_SMALL, 1), ("bf16x3", MI_K20, 0), ("f16f8", MI_K20, 0), ("f16f8", MI_K20, 1)))
def _(v):
    prec, (k, h, w, pad), acc = v
    s, ub, t, win, P, probs = _heads(k, h, w, pad)
    nb = q("miseg_iic_local_bwd_ws_bytes", k, pad, P * s)
    gprob = rn(s, 2 * ub, k, h, w) if acc else out(s, 2 * ub, k, h, w)
    return abi_case("miseg_iic_local_bwd_heads", dict(probs=probs, S=s, UB=ub, K=k, H=h, W=w, pad=pad, win=win, P=P, grad_raw=rn(s, P, t, t, k, k), scale=ru(s, P),
                                                      gprob=gprob, accumulate=acc, precision=PREC[prec], ws=ws(nb), ws_bytes=max(nb, 16)),
                    inout=("gprob",) if acc else (), rebind="probs")


def _planes(fill):
    k, h, w, pad = MI_K20
    s, ub, t, win, P, probs = _heads(k, h, w, pad)
    pb = q("miseg_iic_local_planes_bytes", s, ub, k, h, w, pad)
    assert pb > 0
    return k, h, w, pad, s, ub, t, win, P, probs, pb, torch.full((pb,), fill, dtype=U8, device=DEV)


@case("miseg_iic_local_make_planes")
def _(v):
    k, h, w, pad, s, ub, t, win, P, probs, pb, planes = _planes(0x7F)
    return abi_case("miseg_iic_local_make_planes", dict(probs=probs, S=s, UB=ub, K=k, H=h, W=w, pad=pad, planes=planes, planes_bytes=pb), inout=("planes",), rebind="probs")


@case("miseg_iic_local_joint_fwd_heads_planes")
def _(v):
    k, h, w, pad, s, ub, t, win, P, probs, pb, planes = _planes(0x7F)
    nb = q("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, P * s)
    return abi_case("miseg_iic_local_joint_fwd_heads_planes", dict(probs=probs, S=s, UB=ub, K=k, H=h, W=w, pad=pad, win=win, P=P, raw=out(s, P, t, t, k, k), ws=ws(nb),
                                                                   ws_bytes=max(nb, 16), planes=planes, planes_bytes=pb), inout=("planes",), rebind="probs")


@case("miseg_iic_local_bwd_heads_planes")
def _(v):
    k, h, w, pad, s, ub, t, win, P, probs, pb, planes = _planes(0x00)
    _abi().call("miseg_iic_local_make_planes", st(), probs.data_ptr(), s, ub, k, h, w, pad, planes.data_ptr(), pb)
    nb = q("miseg_iic_local_bwd_ws_bytes", k, pad, P * s)
    return abi_case("miseg_iic_local_bwd_heads_planes", dict(planes=planes, planes_bytes=pb, S=s, UB=ub, K=k, H=h, W=w, pad=pad, win=win, P=P, grad_raw=rn(s, P, t, t, k, k),
                                                             scale=ru(s, P), gprob=out(s, 2 * ub, k, h, w), accumulate=0, ws=ws(nb), ws_bytes=max(nb, 16)), rebind="grad_raw")


OUT_MI = dict(N=2, C=4, H=12, W=10, pad=1)


@case("miseg_iic_out_joint_fwd")
def _(v):
    o = OUT_MI
    wins = [(0, 8, 0, 10), (4, 12, 2, 9), (1, 7, 3, 8)]
    nb = q("miseg_iic_out_joint_ws_bytes", o["N"], o["C"], o["H"], o["W"], o["pad"], len(wins))
    return abi_case("miseg_iic_out_joint_fwd", dict(a=rn(o["N"], o["H"], o["W"], o["C"]), b=rn(o["N"], o["H"], o["W"], o["C"]), flips=ints([2, 1]), win=ints(wins), P=len(wins),
                                                    raw=out(len(wins), 3, 3, o["C"], o["C"]), ws=ws(nb), ws_bytes=max(nb, 16), **o), rebind="a")


@case("miseg_iic_out_bwd", (0, 1))
def _(v):
    o = OUT_MI
    wins = [(0, 8, 0, 10), (4, 12, 2, 9), (1, 7, 3, 8)]
    ga = rn(o["N"], o["H"], o["W"], o["C"]) if v else out(o["N"], o["H"], o["W"], o["C"])
    return abi_case("miseg_iic_out_bwd", dict(a=rn(o["N"], o["H"], o["W"], o["C"]), b=rn(o["N"], o["H"], o["W"], o["C"]), flips=ints([2, 1]), win=ints(wins), P=len(wins),
                                              grad_raw=rn(len(wins), 3, 3, o["C"], o["C"]), scale=ru(len(wins)), ga=ga, gb=out(o["N"], o["H"], o["W"], o["C"]), accumulate=v,
                                              **o), inout=("ga",) if v else (), rebind="b")


# =================================================================================================================== cluster heads
# exact_heads.LOCAL_CASES "k20_24x2x20_3x22x36" (every storage type) and "wave_16x5x20_2x6x10" (the shipped top tap, 16-bit);
# exact_heads.FWD_CASES "reg4_guard_k7" for the forward
LH = dict(C=24, S=2, K=20, M=3, H=22, W=36, B=4)
LH_FWD = dict(C=8, S=2, K=7, M=3, H=24, W=44, B=4)
LH_TOP = dict(C=16, S=5, K=20, M=2, H=6, W=10, B=3)


def _lh(v, d, rows=False):
    b, m, h, w, c, s, k = d["B"], d["M"], d["H"], d["W"], d["C"], d["S"], d["K"]
    src = ints([3, 1, 2][:m]) if b == 4 else ints([2, 1][:m])
    return dict(dt=DT(v), feat=rn(b, h, w, c, dtype=v), B=b, H=h, W=w, C=c, src=src, flips=ints([1, 2, 3][:m]), M=m, S=s, K=k, T=0.5)


@case("miseg_head_local_fwd", ALL)
def _(v):
    d = LH_FWD
    a = _lh(v, d)
    return abi_case("miseg_head_local_fwd", dict(w=rn(d["S"], d["K"], d["C"], scale=0.3), b=rn(d["S"], d["K"], scale=0.1), prob=out(d["S"], d["M"], d["K"], d["H"], d["W"]),
                                                 simplex_tol=1e-3, simplex_violations=ints([5]), **a), inout=("simplex_violations",), rebind="feat")


def _lh_bwd(name, v, d, **more):
    a = _lh(v, d)
    b, m, h, w, c, s, k = d["B"], d["M"], d["H"], d["W"], d["C"], d["S"], d["K"]
    nb = q("miseg_head_local_bwd_ws_bytes", m, h, w, c, s, k)
    a.update(w=rn(s, k, c, scale=0.3), gprob=rn(s, m, k, h, w, scale=0.1), gw=out(s, k, c), gb=out(s, k), ws=ws(nb), ws_bytes=max(nb, 16))
    if "prob" in TABLE.EPS[name].params:
        a["prob"] = simplex(s, m, k, h, w, dim=2)
    a.update(more)
    return a


@case("miseg_head_local_bwd", ALL)
def _(v):
    d = LH
    a = _lh_bwd("miseg_head_local_bwd", v, d, gfeat=zeros(d["B"], d["H"], d["W"], d["C"], dtype=v))
    return abi_case("miseg_head_local_bwd", a, inout=("gfeat",), rebind="feat")


@case("miseg_head_local_bwd_rows", TWO)
def _(v):
    d = LH
    a = _lh_bwd("miseg_head_local_bwd_rows", v, d, gfeat_rows=zeros(3, d["H"], d["W"], d["C"], dtype=v), row0=1)
    return abi_case("miseg_head_local_bwd_rows", a, inout=("gfeat_rows",), rebind="feat")


@case("miseg_head_local_bwd_recompute", HALF)
def _(v):
    d = LH_TOP
    assert q("miseg_head_local_bwd_recompute_supported", DT(v), d["C"], d["S"], d["K"])
    a = _lh_bwd("miseg_head_local_bwd_recompute", v, d, gfeat_rows=zeros(2, d["H"], d["W"], d["C"], dtype=v), row0=1, bias=rn(d["S"], d["K"], scale=0.1))
    return abi_case("miseg_head_local_bwd_recompute", a, inout=("gfeat_rows",), rebind="feat")


@case("miseg_head_local_bwd_acc", ALL)
def _(v):
    d = LH if v == F32 else LH_TOP      # fp32: the general kernel; 16-bit: the shipped top tap's wave kernel
    assert q("miseg_head_local_bwd_acc_supported", DT(v), d["C"], d["S"], d["K"])
    a = _lh_bwd("miseg_head_local_bwd_acc", v, d, gfeat_inout=rn(d["B"], d["H"], d["W"], d["C"], dtype=v))
    return abi_case("miseg_head_local_bwd_acc", a, inout=("gfeat_inout",), rebind="feat")


# exact_heads.GLOBAL_CASES "c48_8x8_s5k20_m3", W halved (H * W stays a power of two)
GH = dict(C=48, H=8, W=4, S=5, K=20, M=3, B=4)


def _gh(v, d):
    return dict(dt=DT(v), B=d["B"], H=d["H"], W=d["W"], C=d["C"], src=ints([3, 0, 2]), M=d["M"], S=d["S"], K=d["K"], T=0.5)


@case("miseg_head_global_fwd", ALL)
def _(v):
    d = GH
    return abi_case("miseg_head_global_fwd", dict(feat=rn(d["B"], d["H"], d["W"], d["C"], dtype=v), w=rn(d["S"], d["K"], d["C"], scale=0.3), b=rn(d["S"], d["K"], scale=0.1),
                                                  pooled=out(d["M"], d["C"]), prob=out(d["S"], d["M"], d["K"]), **_gh(v, d)), rebind="feat")


def _gh_bwd(v, d):
    s, m, k, c = d["S"], d["M"], d["K"], d["C"]
    return dict(w=rn(s, k, c, scale=0.3), pooled=rn(m, c), prob=simplex(s, m, k, dim=2), gprob=rn(s, m, k, scale=0.1), gw=out(s, k, c), gb=out(s, k), dz_ws=out(s * m * k),
                **_gh(v, d))


@case("miseg_head_global_bwd", TWO)
def _(v):
    d = GH
    return abi_case("miseg_head_global_bwd", dict(gfeat=zeros(d["B"], d["H"], d["W"], d["C"], dtype=v), **_gh_bwd(v, d)), inout=("gfeat",), rebind="pooled")


@case("miseg_head_global_bwd_rows", TWO)
def _(v):
    d = GH
    a = _gh_bwd(v, d)
    a["src"] = ints([3, 1, 2])
    return abi_case("miseg_head_global_bwd_rows", dict(gfeat_rows=zeros(3, d["H"], d["W"], d["C"], dtype=v), row0=1, **a), inout=("gfeat_rows",), rebind="pooled")


# heads_var_ref.LOCAL_CASES "zero_norm_mlp" / "plain" shapes, GLOBAL_CASES "zero_norm_mlp" / "zero_norm_lin"
def _var_w(s, c, hid, k):
    if hid:
        return dict(w1=rn(s, hid, c, scale=0.3), b1=rn(s, hid, scale=0.1), HID=hid, w2=rn(s, k, hid, scale=0.3), b2=rn(s, k, scale=0.1))
    return dict(w1=rn(s, k, c, scale=0.3), b1=rn(s, k, scale=0.1), HID=0, w2=None, b2=None)


def _var_g(s, c, hid, k):
    if hid:
        return dict(gw1=out(s, hid, c), gb1=out(s, hid), gw2=out(s, k, hid), gb2=out(s, k))
    return dict(gw1=out(s, k, c), gb1=out(s, k), gw2=None, gb2=None)


VAR = tuple((t, hid, nrm) for t in TWO for hid, nrm in ((64, 1), (0, 0)))
LV = dict(B=4, M=3, C=8, K=6, S=2, H=5, W=7)


def _lv(v):
    dtype, hid, nrm = v
    d = LV
    hid_ = hid
    return dtype, d, hid_, dict(dt=DT(dtype), feat=rn(d["B"], d["H"], d["W"], d["C"], dtype=dtype), B=d["B"], H=d["H"], W=d["W"], C=d["C"], src=ints([3, 0, 2]), flips=ints([3, 1, 2]),
                                M=d["M"], S=d["S"], K=d["K"], T=0.5, normalize=nrm, **_var_w(d["S"], d["C"], hid_, d["K"]))


@case("miseg_head_local_var_fwd", VAR + ((F16, 64, 1),))
def _(v):
    dtype, d, hid, a = _lv(v)
    return abi_case("miseg_head_local_var_fwd", dict(prob=out(d["S"], d["M"], d["K"], d["H"], d["W"]), **a), rebind="feat")


@case("miseg_head_local_var_bwd", VAR)
def _(v):
    dtype, d, hid, a = _lv(v)
    nb = q("miseg_head_local_var_bwd_ws_bytes", d["M"], d["H"], d["W"], d["C"], hid, d["S"], d["K"])
    return abi_case("miseg_head_local_var_bwd", dict(gprob=rn(d["S"], d["M"], d["K"], d["H"], d["W"], scale=0.1), gfeat=zeros(d["B"], d["H"], d["W"], d["C"], dtype=dtype),
                                                     ws=ws(nb), ws_bytes=max(nb, 16), **_var_g(d["S"], d["C"], hid, d["K"]), **a), inout=("gfeat",), rebind="feat")


GVAR = tuple((t, hid, nrm) for t in TWO for hid, nrm in ((128, 1), (0, 0)))
GV = dict(B=5, M=4, C=8, K=6, S=2, H=2, W=3)


def _gv(v):
    dtype, hid, nrm = v
    d = GV
    return dtype, d, hid, dict(dt=DT(dtype), B=d["B"], H=d["H"], W=d["W"], C=d["C"], src=ints([4, 0, 3, 1]), M=d["M"], S=d["S"], K=d["K"], T=0.5, normalize=nrm,
                               **_var_w(d["S"], d["C"], hid, d["K"]))


@case("miseg_head_global_var_fwd", GVAR)
def _(v):
    dtype, d, hid, a = _gv(v)
    return abi_case("miseg_head_global_var_fwd", dict(feat=rn(d["B"], d["H"], d["W"], d["C"], dtype=dtype), pooled=out(d["M"], d["C"]), prob=out(d["S"], d["M"], d["K"]), **a),
                    rebind="feat")


@case("miseg_head_global_var_bwd", GVAR)
def _(v):
    dtype, d, hid, a = _gv(v)
    return abi_case("miseg_head_global_var_bwd", dict(pooled=rn(d["M"], d["C"]), gprob=rn(d["S"], d["M"], d["K"], scale=0.1), gfeat=zeros(d["B"], d["H"], d["W"], d["C"], dtype=dtype),
                                                      dpool_ws=out(d["S"] * d["M"] * d["C"]), **_var_g(d["S"], d["C"], hid, d["K"]), **a), inout=("gfeat",), rebind="pooled")


# =================================================================================================================== U-Net layers
CONV = (3, 20, 36)              # exact_ref "tiled_ragged_*" / "few_tiles_*": N, H, W


def pack(wt, dtype, kind=0, cb=0, cs=0, cin=None):
    from miseg_amd import packcache
    p = packcache._pack_now(wt, dtype, kind, cb, cs if kind else wt.shape[1], cin=cin)
    torch.cuda.synchronize()
    return p


@case("miseg_pack_conv3x3_weights", tuple((t, k) for t in TWO for k in (0, 1)))
def _(v):
    dtype, kind = v
    cout, cin, cb, cc = 32, 24, 8, 16
    numel = (cc * cout if kind else cout * cin) * 9
    return abi_case("miseg_pack_conv3x3_weights", dict(dt=DT(dtype), w=rn(cout, cin, 3, 3), Cout=cout, Cin=cin, kind=kind, ci_begin=cb if kind else 0,
                                                       ci_count=cc if kind else cin, packed=out(numel, dtype=dtype)), rebind="w")


@case("miseg_pack_conv3x3_weights_multi", TWO)
def _(v):
    """Two jobs (a forward pack and a dgrad slice) from one device job table: the table's pointers are recorded by the table's address only."""
    H = _H()
    w0, w1 = rn(32, 16, 3, 3), rn(16, 24, 3, 3)
    p0, p1 = out(32 * 16 * 9, dtype=v), out(8 * 16 * 9, dtype=v)
    first1 = (p0.numel() + 255) // 256
    total = first1 + (p1.numel() + 255) // 256
    blob = struct.pack("<QQiiiiii", w0.data_ptr(), p0.data_ptr(), 32, 16, 0, 0, 16, 0) + struct.pack("<QQiiiiii", w1.data_ptr(), p1.data_ptr(), 16, 24, 1, 8, 8, first1)
    table = torch.frombuffer(bytearray(blob), dtype=U8).clone().to(DEV)

    def call(T):
        _abi().call("miseg_pack_conv3x3_weights_multi", st(), DT(v), T["table"].data_ptr(), 2, total)

    return H.Case(call=call, inputs={"table": table, "w0": w0, "w1": w1}, outputs={"p0": p0, "p1": p1}, expect=("miseg_pack_conv3x3_weights_multi",))


def _conv_in(v, c0=16, c1=0, ups0=0, cout=32):
    n, h, w = CONV
    x0 = rn(n, h >> ups0, w >> ups0, c0, dtype=v)
    x1 = rn(n, h, w, c1, dtype=v) if c1 else None
    return dict(dt=DT(v), in0=x0, C0=c0, ups0=ups0, in1=x1, C1=c1, ups1=0, N=n, H=h, W=w, packed_w=pack(rn(cout, c0 + c1, 3, 3, scale=0.2), v), Cout=cout)


@case("miseg_conv3x3_fwd", tuple((t, f) for t in ALL for f in ("plain", "cat_up")))
def _(v):
    dtype, form = v
    n, h, w = CONV
    a = _conv_in(dtype, 16, 8, 1, 32) if form == "cat_up" else _conv_in(dtype, 8, 0, 0, 32)
    parts = q("miseg_conv3x3_fwd_parts", DT(dtype), a["C0"] + a["C1"], n, h, w, 32)
    return abi_case("miseg_conv3x3_fwd", dict(out=out(n, h, w, 32, dtype=dtype), stats=out(parts, 2, 32), **a), rebind="in0")


@case("miseg_conv3x3_fwd_acc", TWO)
def _(v):
    n, h, w = CONV
    a = _conv_in(v, 8, 0, 0, 32)
    assert q("miseg_conv3x3_fwd_acc_supported", DT(v), 8, n, h, w, 32)
    return abi_case("miseg_conv3x3_fwd_acc", dict(out=out(n, h, w, 32, dtype=v), acc=zeros(2 * 32 + 1, dtype=I64), **a), inout=("acc",), rebind="in0")


@case("miseg_conv3x3_bn_fwd", TWO)
def _(v):
    n, h, w = CONV
    a = _conv_in(v, 8, 0, 0, 32)
    assert q("miseg_conv3x3_bn_fwd_fusable", DT(v), 8, n, h, w, 32)
    parts = q("miseg_conv3x3_stats_parts", DT(v), 8, n, h, w)
    return abi_case("miseg_conv3x3_bn_fwd", dict(out=out(n, h, w, 32, dtype=v), stats=out(parts, 2, 32), gamma=ru(32), beta=rn(32), eps=1e-5, momentum=0.1, rmean=rn(32),
                                                 rvar=ru(32), nbt=ints([7], dtype=I64), saved=out(4, 32), sync_counter=zeros(1, dtype=I32), **a),
                    inout=("rmean", "rvar", "nbt", "sync_counter"), rebind="in0")


@case("miseg_conv3x3_fwd_sumpool", HALF)
def _(v):
    n, h, w, k, cs = 3, 20, 36, 64, 64          # exact_ref.SUMPOOL_CASES "tiled_64_64"
    assert q("miseg_conv3x3_fwd_sumpool_supported", DT(v), k, n, h, w, cs)
    return abi_case("miseg_conv3x3_fwd_sumpool", {"dt": DT(v), "in": rn(n, h, w, k, dtype=v), "Cin": k, "N": n, "H": h, "W": w,
                                                  "packed_w": pack(rn(k, cs, 3, 3, scale=0.2), v, 1, 0, cs), "Cout": cs, "out_pooled": out(n, h // 2, w // 2, cs, dtype=v)},
                    rebind="in")


@case("miseg_conv3x3_fwd_sumpool_acc", HALF)
def _(v):
    n, h, w, k, cs = 4, 256, 256, 16, 32        # exact_ref.SUMPOOL_CASES "stream_16_32": the acc form has streaming shapes only
    assert q("miseg_conv3x3_fwd_sumpool_acc_supported", DT(v), k, n, h, w)
    return abi_case("miseg_conv3x3_fwd_sumpool_acc", {"dt": DT(v), "in": rn(n, h, w, k, dtype=v), "Cin": k, "N": n, "H": h, "W": w,
                                                      "packed_w": pack(rn(k, cs, 3, 3, scale=0.2), v, 1, 0, cs), "Cout": cs,
                                                      "inout_pooled": rn(n, h // 2, w // 2, cs, dtype=v)}, inout=("inout_pooled",), rebind="in")


@case("miseg_conv3x3_dgrad_dual", TWO)
def _(v):
    n, h, w = CONV
    k, c0, c1 = 32, 16, 4                       # exact_ref.DUAL_CASES "tiled_ragged_32_16p4" channels
    return abi_case("miseg_conv3x3_dgrad_dual", dict(dt=DT(v), graw=rn(n, h, w, k, dtype=v), K=k, N=n, H=h, W=w, packed_w=pack(rn(k, c0 + c1, 3, 3, scale=0.2), v, 1, 0, c0 + c1),
                                                     C0=c0, out0=out(n, h, w, c0, dtype=v), C1=c1, out1=out(n, h, w, c1, dtype=v)), rebind="graw")


def _coef(k):
    c = rn(6, k, scale=0.1)
    c[0], c[3] = ru(k), ru(k)
    return c


@case("miseg_conv3x3_dgrad_bn", tuple((t, f) for t in TWO for f in ("loader", "red")))
def _(v):
    dtype, form = v
    n, h, w = CONV
    k, cs = 32, 16                              # exact_ref.DGRAD_BN_CASES "eval_tiled_ragged"
    assert q("miseg_conv3x3_dgrad_bn_supported", DT(dtype), k, n, h, w, cs, 0)
    a = dict(dt=DT(dtype), raw_or_graw=rn(n, h, w, k, dtype=dtype), gy=rn(n, h, w, k, dtype=dtype), bwd_coef=_coef(k), K=k, N=n, H=h, W=w,
             packed_w=pack(rn(k, cs, 3, 3, scale=0.2), dtype, 1, 0, cs), Cs=cs, out=out(n, h, w, cs, dtype=dtype), pool_out=0, red_raw=None, red_saved=None, red_parts=None)
    if form == "red":
        rows = q("miseg_conv3x3_dgrad_red_parts", DT(dtype), k, n, h, w, cs)
        assert rows > 0
        a.update(red_raw=rn(n, h, w, cs, dtype=dtype), red_saved=rn(4, cs), red_parts=out(rows, 2, cs))
    return abi_case("miseg_conv3x3_dgrad_bn", a, rebind="gy")


@case("miseg_conv3x3_wgrad", tuple((t, f) for t in ALL for f in ("plain", "cat_up")))
def _(v):
    dtype, form = v
    n, h, w = CONV
    c0, ups0, c1, cout = (32, 1, 16, 32) if form == "cat_up" else (16, 0, 0, 32)
    nb = q("miseg_conv3x3_wgrad_ws_bytes", n, h, w, c0 + c1, cout)
    return abi_case("miseg_conv3x3_wgrad", dict(dt=DT(dtype), in0=rn(n, h >> ups0, w >> ups0, c0, dtype=dtype), C0=c0, ups0=ups0, in1=rn(n, h, w, c1, dtype=dtype) if c1 else None,
                                                C1=c1, ups1=0, N=n, H=h, W=w, gout=rn(n, h, w, cout, dtype=dtype), Cout=cout, gw=out(cout, c0 + c1, 3, 3), ws=ws(nb),
                                                ws_bytes=max(nb, 16)), rebind="in0")


@case("miseg_conv3x3_wgrad_bn", TWO)
def _(v):
    n, h, w = CONV
    c0, cout = 16, 32
    nb = q("miseg_conv3x3_wgrad_ws_bytes", n, h, w, c0, cout)
    return abi_case("miseg_conv3x3_wgrad_bn", dict(dt=DT(v), in0=rn(n, h, w, c0, dtype=v), C0=c0, ups0=0, in1=None, C1=0, ups1=0, N=n, H=h, W=w, raw=rn(n, h, w, cout, dtype=v),
                                                   gy=rn(n, h, w, cout, dtype=v), bwd_coef=_coef(cout), Cout=cout, gw=out(cout, c0, 3, 3), ws=ws(nb), ws_bytes=max(nb, 16)),
                    rebind="in0")


@case("miseg_conv3x3_wgrad_slice")
def _(v):
    cout, cpad, cin = 16, 8, 3                  # exact_ref.SLICE_CASE
    return abi_case("miseg_conv3x3_wgrad_slice", dict(gw_padded=rn(cout, cpad, 3, 3), Cout=cout, Cin_pad=cpad, Cin=cin, gw=out(cout, cin, 3, 3)), rebind="gw_padded")


STEM = (3, 50, 46, 16)          # exact_ref.STEM_CASES "ragged_16"


@case("miseg_conv3x3_stem_fwd", tuple((t, f) for t in HALF for f in (0, 1)))
def _(v):
    dtype, x_f32 = v
    n, h, w, cout = STEM
    cp = 1 if x_f32 else 8
    assert q("miseg_conv3x3_stem_supported", DT(dtype), 1, cp, cout)
    x = rn(n, h, w, 1) if x_f32 else rn(n, h, w, 8, dtype=dtype)
    return abi_case("miseg_conv3x3_stem_fwd", dict(dt=DT(dtype), x=x, x_f32=x_f32, CP=cp, N=n, H=h, W=w, w=rn(cout, 1, 3, 3, scale=0.3), Cin_weight=1, Cout=cout,
                                                   out=out(n, h, w, cout, dtype=dtype), acc_or_null=zeros(2 * cout + 1, dtype=I64)), inout=("acc_or_null",), rebind="x")


@case("miseg_conv3x3_stem_wgrad", tuple((t, f) for t in HALF for f in (0, 1)))
def _(v):
    dtype, x_f32 = v
    n, h, w, cout = STEM
    cp = 1 if x_f32 else 8
    nb = q("miseg_conv3x3_stem_wgrad_ws_bytes", cout)
    x = rn(n, h, w, 1) if x_f32 else rn(n, h, w, 8, dtype=dtype)
    return abi_case("miseg_conv3x3_stem_wgrad", dict(dt=DT(dtype), x=x, x_f32=x_f32, CP=cp, N=n, H=h, W=w, graw=rn(n, h, w, cout, dtype=dtype), Cout=cout, gw=out(cout, 1, 3, 3),
                                                     ws=ws(nb), ws_bytes=max(nb, 16)), rebind="x")


@case("miseg_conv3x3_stem_dgrad", TWO)
def _(v):
    n, h, w, cout = STEM
    assert q("miseg_conv3x3_stem_dgrad_supported", DT(v), cout, w)
    nb = q("miseg_conv3x3_stem_dgrad_ws_bytes", cout)
    return abi_case("miseg_conv3x3_stem_dgrad", dict(dt=DT(v), graw=rn(n, h, w, cout, dtype=v), N=n, H=h, W=w, Cout=cout, w=rn(cout, 1, 3, 3, scale=0.3), gimage=out(n, 1, h, w),
                                                     ws=ws(nb), ws_bytes=max(nb, 16)), rebind="graw")


C1 = (3, 37, 53)                # exact_ref.C1X1_SHAPES "ragged"


@case("miseg_conv1x1_fwd", ALL)
def _(v):
    n, h, w = C1
    return abi_case("miseg_conv1x1_fwd", {"dt": DT(v), "in": rn(n, h, w, 16, dtype=v), "N": n, "H": h, "W": w, "Cin": 16, "w": rn(4, 16, scale=0.3), "bias": rn(4), "Cout": 4,
                                          "out": out(n, h, w, 4)}, rebind="in")


@case("miseg_conv1x1_bwd", TWO)
def _(v):
    n, h, w = C1
    nb = q("miseg_conv1x1_bwd_ws_bytes", n, h, w, 16, 4)
    return abi_case("miseg_conv1x1_bwd", {"dt": DT(v), "in": rn(n, h, w, 16, dtype=v), "gout": rn(n, h, w, 4), "N": n, "H": h, "W": w, "Cin": 16, "w": rn(4, 16, scale=0.3),
                                          "Cout": 4, "gin": out(n, h, w, 16, dtype=v), "gw": out(4, 16), "gbias": out(4), "ws": ws(nb), "ws_bytes": max(nb, 16)}, rebind="gout")


# ---- BatchNorm
BN = (2, 8, 12, 24)             # exact_ref.BN_FWD_CASES: N, H, W, C


def _saved(c):
    s = rn(4, c, scale=0.3)
    s[1], s[2] = ru(c), ru(c)
    return s


@case("miseg_bn_finalize")
def _(v):
    parts, c = 5, 24
    p = rn(parts, 2, c)
    p[:, 1] = p[:, 0] ** 2 + ru(parts, c) * 40
    return abi_case("miseg_bn_finalize", dict(parts=p, nparts=parts, C=c, count=200, gamma=ru(c), beta=rn(c), eps=1e-5, momentum=0.1, rmean=rn(c), rvar=ru(c),
                                              nbt=ints([3], dtype=I64), saved=out(4, c)), inout=("rmean", "rvar", "nbt"), rebind="parts")


@case("miseg_bn_eval_coeffs")
def _(v):
    c = 24
    return abi_case("miseg_bn_eval_coeffs", dict(C=c, gamma=ru(c), beta=rn(c), eps=1e-5, rmean=rn(c), rvar=ru(c), saved=rn(4, c)), inout=("saved",), rebind="rvar")


@case("miseg_bn_relu_fwd", ALL)
def _(v):
    n, h, w, c = BN
    return abi_case("miseg_bn_relu_fwd", dict(dt=DT(v), raw=rn(n, h, w, c, dtype=v), N=n, H=h, W=w, C=c, saved=_saved(c), y=out(n, h, w, c, dtype=v),
                                              pooled=out(n, h // 2, w // 2, c, dtype=v)), rebind="raw")


@case("miseg_bn_relu_fwd_acc", TWO)
def _(v):
    n, h, w, c = BN
    raw = rn(n, h, w, c, dtype=v)
    x = raw.float().view(-1, c)
    acc = torch.cat(((x.sum(0) * 2 ** 20).round().to(I64), ((x * x).sum(0) * 2 ** 20).round().to(I64), zeros(1, dtype=I64)))
    return abi_case("miseg_bn_relu_fwd_acc", dict(dt=DT(v), raw=raw, N=n, H=h, W=w, C=c, acc=acc, gamma=ru(c), beta=rn(c), eps=1e-5, momentum=0.1, rmean=rn(c), rvar=ru(c),
                                                  nbt=ints([3], dtype=I64), saved=out(4, c), y=out(n, h, w, c, dtype=v), pooled=out(n, h // 2, w // 2, c, dtype=v)),
                    inout=("rmean", "rvar", "nbt"), rebind="raw")


def _bn_bwd(v, c=None):
    n, h, w = BN[:3]
    c = c or 32                                 # the backward kernels need C / vector to divide 256
    nb = q("miseg_bn_bwd_ws_bytes", n, h, w, c)
    return dict(dt=DT(v), raw=rn(n, h, w, c, dtype=v), gy=rn(n, h, w, c, dtype=v), N=n, H=h, W=w, C=c, gamma=ru(c), saved=_saved(c), training=1,
                ggamma=out(c), gbeta=out(c), ws=ws(nb), ws_bytes=max(nb, 16)), (n, h, w, c)


@case("miseg_bn_relu_bwd", ALL)
def _(v):
    a, (n, h, w, c) = _bn_bwd(v)
    return abi_case("miseg_bn_relu_bwd", dict(y=rn(n, h, w, c, dtype=v), gpool=rn(n, h // 2, w // 2, c, dtype=v), graw=out(n, h, w, c, dtype=v), **a), rebind="gy")


@case("miseg_bn_relu_bwd_sync", TWO)
def _(v):
    a, (n, h, w, c) = _bn_bwd(v)
    return abi_case("miseg_bn_relu_bwd_sync", dict(y=rn(n, h, w, c, dtype=v), gpool=rn(n, h // 2, w // 2, c, dtype=v), graw=out(n, h, w, c, dtype=v),
                                                   sync_counter=zeros(1, dtype=I32), **a), inout=("sync_counter",), rebind="gy")


@case("miseg_bn_relu_bwd_dual", TWO)
def _(v):
    a, (n, h, w, c) = _bn_bwd(v)
    return abi_case("miseg_bn_relu_bwd_dual", dict(gpool=rn(n, h // 2, w // 2, c, dtype=v), gy2=rn(1, h, w, c, dtype=v), n2_begin=1, n2_end=2, graw=out(n, h, w, c, dtype=v), **a),
                    rebind="gy")


@case("miseg_bn_relu_bwd_dual_acc", TWO)
def _(v):
    a, (n, h, w, c) = _bn_bwd(v)
    assert q("miseg_bn_relu_bwd_acc_supported", DT(v), n, h, w, c)
    return abi_case("miseg_bn_relu_bwd_dual_acc", dict(gpool=rn(n, h // 2, w // 2, c, dtype=v), gy2=rn(1, h, w, c, dtype=v), n2_begin=1, n2_end=2, graw=out(n, h, w, c, dtype=v),
                                                       acc=zeros(4 * c + 2, dtype=I64), **a), inout=("acc",), rebind="gy")


@case("miseg_bn_relu_bwd_ext", TWO)
def _(v):
    a, (n, h, w, c) = _bn_bwd(v)
    return abi_case("miseg_bn_relu_bwd_ext", dict(graw=out(n, h, w, c, dtype=v), ext_parts=rn(6, 2, c), ext_nparts=6, **a), rebind="gy")


@case("miseg_bn_relu_bwd_stats", tuple((t, e) for t in TWO for e in (0, 1)))
def _(v):
    dtype, ext = v
    a, (n, h, w, c) = _bn_bwd(dtype)
    return abi_case("miseg_bn_relu_bwd_stats", dict(bwd_coef=out(6, c), ext_parts=rn(6, 2, c) if ext else None, ext_nparts=6 if ext else 0, **a), rebind="gy" if not ext else "ext_parts")


@case("miseg_sumpool2x2", tuple((t, a) for t in TWO for a in (0, 1)))
def _(v):
    dtype, acc = v
    n, h, w, c = 2, 6, 10, 16                   # exact_ref.SUMPOOL2X2_SHAPES
    o = rn(n, h // 2, w // 2, c, dtype=dtype) if acc else out(n, h // 2, w // 2, c, dtype=dtype)
    return abi_case("miseg_sumpool2x2", {"dt": DT(dtype), "in": rn(n, h, w, c, dtype=dtype), "N": n, "H": h, "W": w, "C": c, "out": o, "accumulate": acc},
                    inout=("out",) if acc else (), rebind="in")


@case("miseg_axpy", ALL)
def _(v):
    return abi_case("miseg_axpy", dict(dt=DT(v), src=rn(1000, dtype=v), dst=rn(1000, dtype=v), numel=1000), inout=("dst",), rebind="src")


@case("miseg_cast_pad", tuple((t, c) for t in TWO for c in (1, 3)))
def _(v):
    dtype, cin = v
    npix, cp = 3 * 50 * 46, 4 if dtype == F32 else 8
    return abi_case("miseg_cast_pad", {"in": rn(npix, cin), "npix": npix, "Cin": cin, "dt_out": DT(dtype), "out": out(npix, cp, dtype=dtype), "CP": cp}, rebind="in")


# =================================================================================================================== the tests
def _id(v):
    if v is None:
        return "call"
    return "-".join(str(x).replace("torch.", "") for x in (v if isinstance(v, tuple) else (v,))).replace(" ", "")


def _distinct_builders():
    seen, rows = set(), []
    for name in sorted(CASES):
        if CASES[name] in seen:
            continue
        seen.add(CASES[name])
        rows += [pytest.param(name, v, id=f"{name}[{_id(v)}]") for v in VARIANTS[name]]
    return rows


@pytest.mark.parametrize("name,variant", _distinct_builders())
def test_replay_equals_eager(name, variant):
    H = _H()
    _G.manual_seed(zlib.crc32(f"{name}/{_id(variant)}".encode()))
    c = CASES[name](variant)
    torch.cuda.synchronize()
    try:
        RECORDED.update(H.assert_replay_equals_eager(c))
    finally:
        torch.cuda.synchronize()
        if getattr(c, "after", None):
            c.after()


def test_zz_every_taped_entry_point_was_replayed():
    """Last in the module: the names on the tapes recorded above against the taped entry points parsed from csrc/*.hip."""
    taped = set(TABLE.taped_entry_points())
    want = taped - set(EXCLUDED)
    print(f"\ntaped entry points: {len(taped)}; replayed here: {len(RECORDED & taped)}; excluded: {len(EXCLUDED)}; order-dependent cases: {sorted(set(ORDER_DEPENDENT))}")
    assert len(EXCLUDED) <= 5 and not set(EXCLUDED) - taped
    assert not want - RECORDED, f"taped, never on a tape of this module: {sorted(want - RECORDED)}"
    assert not RECORDED - taped, f"on a tape, not parsed as taped: {sorted(RECORDED - taped)}"
    assert len(RECORDED & taped) + len(EXCLUDED) == len(taped)
