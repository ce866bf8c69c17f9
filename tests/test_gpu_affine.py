"""``ops.affine_warp`` (csrc/affine.hip) and ``AffineTensorTransform`` on GPU tensors against torch on the CPU in float64
(tests/affine_ref.py: ``F.affine_grid`` + ``F.grid_sample`` and its autograd).  Shapes, matrices and bounds are affine_ref's; every
test prints the figures it asserts on (run with -s).

Bounds.  Forward: 16 * 2^-23 * max(H, W) * max|x|.  Backward: the same with max|g|, times 4 * max(1, cov), cov the largest entry of
the float64 backward of an all-ones gradient.  Nearest: exact away from rounding ties (float64 source coordinate further than 1e-3
from k + 0.5; at most 2 % of the pixels may be left out); the nearest gradient is integer-valued so that fp32 sums are exact.
Adjoint identity: 1e-5 relative to the larger of the two inner products, summed in float64 on the host.
"""
import functools

import numpy as np
import pytest
import torch

import affine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SHAPES]
shapes = pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
orders = pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])


def _ops():
    from miseg_amd import ops
    return ops


def _on_device(t, channels_last):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t.contiguous()


def _nearest_gradient(shape):
    """Integer-valued, and zero where the output pixel sits near a rounding tie."""
    h, w, c = shape
    theta = R.theta_for("nearest")
    gen = torch.Generator().manual_seed(77 + h + w)
    g = torch.randint(-8, 9, (theta.shape[0], c, h, w), generator=gen).float()
    return g * R.away_from_ties(theta, h, w)[:, None].float()


def _run(shape, mode, channels_last):
    """One forward and one backward through autograd: (y, gx) on the device."""
    x, g = R.inputs(shape, mode)
    if mode == "nearest":
        g = _nearest_gradient(shape)
    x = _on_device(x, channels_last).requires_grad_(True)
    y = _ops().affine_warp(x, R.theta_for(mode), mode=mode)
    (gx,) = torch.autograd.grad(y, x, _on_device(g, channels_last))
    return y.detach(), gx


@functools.lru_cache(maxsize=None)
def result(shape, mode, channels_last):
    y, gx = _run(shape, mode, channels_last)
    torch.cuda.synchronize()
    return y, gx


def _check_format(t, channels_last):
    assert t.is_contiguous(memory_format=torch.channels_last) if channels_last else t.is_contiguous()


@shapes
@orders
def test_bilinear_forward(shape, channels_last):
    h, w, c = shape
    x, _ = R.inputs(shape, "bilinear")
    y64 = R.reference(shape, "bilinear")[0]
    y, _ = result(shape, "bilinear", channels_last)
    _check_format(y, channels_last)
    err, bound = float((y.cpu().double() - y64).abs().max()), R.forward_bound(h, w, x.abs().max())
    print(f"\naffine fwd {shape} nhwc={channels_last}: max|y - y64| = {err:.3e}  bound {bound:.3e}")
    assert err <= bound


@shapes
@orders
def test_bilinear_backward(shape, channels_last):
    h, w, c = shape
    _, g = R.inputs(shape, "bilinear")
    _, gx64, cov = R.reference(shape, "bilinear")
    _, gx = result(shape, "bilinear", channels_last)
    _check_format(gx, channels_last)
    err, bound = float((gx.cpu().double() - gx64).abs().max()), R.backward_bound(h, w, g.abs().max(), cov)
    print(f"\naffine bwd {shape} nhwc={channels_last}: max|gx - gx64| = {err:.3e}  bound {bound:.3e}  cov {cov:.2f}")
    assert err <= bound


@shapes
@orders
def test_adjoint_identity(shape, channels_last):
    x, g = R.inputs(shape, "bilinear")
    y, gx = result(shape, "bilinear", channels_last)
    lhs = float((y.cpu().double() * g.double()).sum())
    rhs = float((x.double() * gx.cpu().double()).sum())
    rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"\naffine adjoint {shape} nhwc={channels_last}: <Wx, g> = {lhs:.9e}  <x, W'g> = {rhs:.9e}  relative {rel:.2e}")
    assert rel <= 1e-5


@shapes
@orders
def test_two_calls_give_the_same_bits(shape, channels_last):
    for mode in ("bilinear", "nearest"):
        y0, gx0 = result(shape, mode, channels_last)
        y1, gx1 = _run(shape, mode, channels_last)
        assert torch.equal(y0, y1) and torch.equal(gx0, gx1), mode


@shapes
def test_channels_last_equals_contiguous_bit_for_bit(shape):
    for mode in ("bilinear", "nearest"):
        (y0, gx0), (y1, gx1) = result(shape, mode, False), result(shape, mode, True)
        assert y1.shape == y0.shape and torch.equal(y1.contiguous(), y0) and torch.equal(gx1.contiguous(), gx0), mode


@shapes
def test_flip_matrices_agree_with_ops_flip(shape):
    h, w, c = shape
    x, _ = R.inputs(shape, "bilinear")
    rows = [R.NAMES.index(n) for n in R.FLIP_MASKS]
    flips = torch.tensor(list(R.FLIP_MASKS.values()), dtype=torch.int32, device=DEV)
    want = _ops().flip(x[rows].to(DEV).contiguous(), flips)
    y, _ = result(shape, "bilinear", False)
    err, bound = float((y[rows] - want).abs().max()), R.forward_bound(h, w, x.abs().max())
    print(f"\naffine vs flip {shape}: max difference {err:.3e}  bound {bound:.3e}")
    assert err <= bound


@shapes
@orders
def test_nearest_forward_and_backward_are_exact_away_from_ties(shape, channels_last):
    h, w, c = shape
    theta = R.theta_for("nearest")
    x, _ = R.inputs(shape, "nearest")
    keep = R.away_from_ties(theta, h, w)
    left_out = 1.0 - float(keep.double().mean())
    print(f"\naffine nearest {shape} nhwc={channels_last}: {100 * left_out:.2f} % of the pixels within 1e-3 of a tie")
    assert left_out <= 0.02
    y, gx = result(shape, "nearest", channels_last)
    y64 = R.reference(shape, "nearest")[0]
    keep_c = keep[:, None].expand_as(y64)
    assert torch.equal(y.cpu().double()[keep_c], y64[keep_c])
    g = _nearest_gradient(shape)
    assert torch.equal(gx.cpu().double(), R.warp64_bwd(g, theta, "nearest"))
    assert float(gx.abs().max()) > 0


def test_device_theta_inverse_and_explicit_reach():
    ops = _ops()
    shape = (16, 16, 3)
    x, _ = R.inputs(shape, "bilinear")
    theta = R.thetas()
    xd = x.to(DEV)
    y, _ = result(shape, "bilinear", False)
    assert torch.equal(ops.affine_warp(xd, theta.to(DEV)), y)                            # a device theta: the same bits
    xg = xd.clone().requires_grad_(True)
    ops.affine_warp(xg, theta.to(DEV)).sum().backward()                                  # ... its backward searches 8 pixels
    xh = xd.clone().requires_grad_(True)
    ops.affine_warp(xh, theta, reach=ops.affine_reach(theta, 16, 16)).sum().backward()
    assert torch.equal(xg.grad, xh.grad)                                                 # pixels beyond the needed reach add nothing
    inv = ops.affine_inverse(theta)
    assert torch.equal(ops.affine_warp(xd, theta, inverse=True), ops.affine_warp(xd, inv))
    assert torch.equal(ops.affine_warp(xd, theta.to(DEV), inverse=True), ops.affine_warp(xd, inv))
    assert not ops.affine_warp(xd, theta).requires_grad


# ---- the class

class _Spy:
    def __init__(self, monkeypatch):
        self.calls = 0
        ops = _ops()
        real = ops.affine_warp

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)

        monkeypatch.setattr(ops, "affine_warp", spy)


@pytest.fixture()
def numpy_state():
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_class_on_gpu_tensors_equals_its_cpu_result(monkeypatch, numpy_state, mode):
    from contrastyou.augment import AffineTensorTransform
    spy = _Spy(monkeypatch)
    tf = AffineTensorTransform(mode=mode)
    x = torch.randn(6, 3, 33, 40, generator=torch.Generator().manual_seed(5))
    np.random.seed(8)
    y_cpu, theta_cpu = tf(x)
    assert spy.calls == 0
    np.random.seed(8)
    y_gpu, theta_gpu = tf(x.to(DEV))
    assert spy.calls == 1 and y_gpu.is_cuda and y_gpu.shape == x.shape and torch.equal(theta_gpu, theta_cpu)
    diff = (y_gpu.cpu() - y_cpu).abs()
    if mode == "bilinear":
        bound = R.forward_bound(33, 40, x.abs().max())
        print(f"\naffine class gpu vs cpu: max difference {float(diff.max()):.3e}  bound {bound:.3e}")
        assert float(diff.max()) <= bound
    else:
        keep = R.away_from_ties(theta_cpu, 33, 40)[:, None].expand_as(diff)
        assert float(keep.double().mean()) >= 0.98 and float(diff[keep].max()) == 0.0
    # 2-D and 3-D inputs, and a channels_last batch, keep shape and memory format
    for shape in ((33, 40), (3, 33, 40)):
        out, m = tf(x[0, 0].to(DEV) if len(shape) == 2 else x[0].to(DEV))
        assert out.shape == shape and m.shape == (1, 2, 3)
    out, _ = tf(x.to(DEV).contiguous(memory_format=torch.channels_last), AffineMatrix=theta_cpu)
    assert out.is_contiguous(memory_format=torch.channels_last) and torch.equal(out.contiguous(), y_gpu)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_class_on_gpu_tensors_agrees_with_the_golden_outputs(golden, monkeypatch, numpy_state, seed):
    from contrastyou.augment import AffineTensorTransform
    spy = _Spy(monkeypatch)
    g = golden("affine")
    x = torch.from_numpy(g[f"seed{seed}/x"])
    tf = AffineTensorTransform()
    np.random.seed(seed)
    y, theta = tf(x.to(DEV))
    assert np.array_equal(theta.numpy(), g[f"seed{seed}/theta_ind"])
    bound = R.forward_bound(9, 7, x.abs().max())
    err = float(np.abs(y.cpu().numpy() - g[f"seed{seed}/y"]).max())
    back, theta_inv = tf(y, AffineMatrix=theta, inverse=True)
    assert np.array_equal(theta_inv.numpy(), g[f"seed{seed}/theta_inv"])
    err_back = float(np.abs(back.cpu().numpy() - g[f"seed{seed}/back"]).max())
    print(f"\naffine class vs golden seed {seed}: forward {err:.3e} (bound {bound:.3e})  round trip {err_back:.3e} (bound {2 * bound:.3e})")
    # the second warp interpolates an input that is `bound` off the golden one (weights sum to at most 1) and adds its own `bound`
    assert spy.calls == 2 and err <= bound and err_back <= 2 * bound


def test_class_gradients_flow_to_the_input(monkeypatch, numpy_state):
    from contrastyou.augment import AffineTensorTransform
    spy = _Spy(monkeypatch)
    tf = AffineTensorTransform()
    x = torch.randn(4, 2, 24, 24, generator=torch.Generator().manual_seed(6))
    w = torch.randn(4, 2, 24, 24, generator=torch.Generator().manual_seed(7))
    xd = x.to(DEV).requires_grad_(True)
    np.random.seed(9)
    y, theta = tf(xd)
    assert y.requires_grad and spy.calls == 1
    (y * w.to(DEV)).sum().backward()
    gx64 = R.warp64_bwd(w, theta, "bilinear")
    cov = float(R.warp64_bwd(torch.ones_like(w), theta, "bilinear").max())
    err, bound = float((xd.grad.cpu().double() - gx64).abs().max()), R.backward_bound(24, 24, w.abs().max(), cov)
    print(f"\naffine class gradient: max error {err:.3e}  bound {bound:.3e}")
    assert err <= bound and float(xd.grad.abs().max()) > 0


def test_class_inverse_returns_the_interior_of_a_smooth_image(numpy_state):
    """f = sin(a u + 0.3) cos(b v - 0.2) on 64 x 64.  Bilinear interpolation of a function with second derivatives f_uu, f_vv is off by
    at most (|f_uu| + |f_vv|) / 8 per unit cell.  Warp 1 samples f at T p: error e1 <= M / 8 with M >= |f_uu| + 2 |f_uv| + |f_vv| (a
    bound on the Hessian's norm).  Warp 2 interpolates y1 = f o T + d, |d| <= e1: the d part stays below e1 (weights sum to 1), and f o T
    has second derivatives a_k' H a_k along the axes, a_k the columns of T's 2 x 2 part A in pixels (a square image: theta's own), so
    e2 <= ||A||_F^2 M / 8.  In all (1 + ||A||_F^2) M / 8, plus two forward roundings.  Interior: |q - centre| <= 23 pixels, whose
    pre-images, their taps and those taps' source points stay inside the image for scales in [0.9, 1.1] and shear <= 0.5 degrees
    (23 * 1.12 + 1.5 = 27.3, times 1.12 = 30.5 < 31.5)."""
    from contrastyou.augment import AffineTensorTransform
    n, hw, a, b = 4, 64, 0.15, 0.11
    v, u = torch.meshgrid(torch.arange(hw, dtype=torch.float64), torch.arange(hw, dtype=torch.float64), indexing="ij")
    f = (torch.sin(a * u + 0.3) * torch.cos(b * v - 0.2)).float()
    img = f[None, None].repeat(n, 1, 1, 1).to(DEV)
    tf = AffineTensorTransform()
    np.random.seed(10)
    y, theta = tf(img)
    back, _ = tf(y, AffineMatrix=theta, inverse=True)
    m = a * a + 2 * a * b + b * b
    frob2 = float((theta[:, :, :2].double() ** 2).sum((1, 2)).max())
    tol = (1 + frob2) * m / 8 + 2 * R.forward_bound(hw, hw, 1.0)
    interior = ((u - 31.5) ** 2 + (v - 31.5) ** 2) <= 23.0 ** 2
    err = float((back.cpu()[:, 0] - f)[:, interior].abs().max())
    moved = float((y.cpu()[:, 0] - f)[:, interior].abs().max())
    print(f"\naffine class round trip: interior error {err:.3e}  tolerance {tol:.3e}  (the warped image itself differs by {moved:.2f})")
    assert err <= tol and moved > 10 * tol


def test_class_takes_the_torch_path_for_what_the_kernels_do_not_cover(monkeypatch):
    from contrastyou.augment import AffineTensorTransform
    spy = _Spy(monkeypatch)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    tiny = torch.tensor([[0.1, 0, 0], [0, 0.1, 0]]).repeat(2, 1, 1)                     # the backward would need 11 pixels
    xd = x.to(DEV).requires_grad_(True)
    y, _ = AffineTensorTransform()(xd, AffineMatrix=tiny)
    assert spy.calls == 0
    y.sum().backward()
    gx64 = R.warp64_bwd(torch.ones_like(x), tiny, "bilinear")
    assert (xd.grad.cpu().double() - gx64).abs().max() <= 1e-4 * float(gx64.max())
    y2, _ = AffineTensorTransform()(x.to(DEV), AffineMatrix=tiny)                       # no gradient wanted: the kernel
    assert spy.calls == 1 and (y2 - y.detach()).abs().max() <= R.forward_bound(32, 32, x.abs().max())
    for other in (x.to(DEV).half(), x.to(DEV).double()):
        out, _ = AffineTensorTransform()(other, AffineMatrix=R.thetas()[-2:].to(other.dtype))      # torch wants one dtype, as in the reference
        assert out.dtype == other.dtype and out.shape == x.shape
    out, _ = AffineTensorTransform(mode="bicubic")(x.to(DEV), AffineMatrix=R.thetas()[-2:])
    assert spy.calls == 1 and out.shape == x.shape


def test_refusals():
    ops = _ops()
    theta = torch.eye(2, 3)[None]
    x = torch.zeros(1, 1, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="2048"):
        ops.affine_warp(torch.zeros(1, 1, 4096, 2, device=DEV), theta)
    with pytest.raises(ValueError, match="GPU"):
        ops.affine_warp(torch.zeros(1, 1, 8, 8), theta)
    with pytest.raises(ValueError, match="theta"):
        ops.affine_warp(x, theta.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reach"):
        ops.affine_warp(x, theta, reach=9)
    with pytest.raises(ValueError, match="reach"):
        ops.affine_warp(x, theta, reach=0)
    with pytest.raises(ValueError):
        ops.affine_warp(x, theta, mode="bicubic")
    with pytest.raises(ValueError):
        ops.affine_warp(x.half(), theta)
    with pytest.raises(ValueError):
        ops.affine_warp(x, torch.eye(2, 3).repeat(2, 1, 1))                             # two matrices for one sample
    with pytest.raises(ValueError):
        ops.affine_warp(torch.zeros(1, 2, 8, 16, device=DEV)[:, :, :, ::2], theta)      # neither contiguous nor channels_last
    xg = torch.zeros(1, 1, 64, 64, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="search"):
        ops.affine_warp(xg, theta * 0.1)                                                # needs 11 pixels, and a gradient is wanted
    with pytest.raises(ValueError, match="search"):
        ops.affine_warp(xg, theta * 0.5, reach=1)                                       # an explicit reach below what the matrices need
    assert ops.affine_warp(xg.detach(), theta * 0.1).shape == xg.shape                  # forward only: any matrix
    huge = torch.tensor([[[3e38, -3e38, 3e38], [float("inf"), float("nan"), 1.0]]])
    assert float(ops.affine_warp(torch.ones(1, 1, 8, 8, device=DEV), huge).abs().max()) == 0.0     # reads nothing, nothing out of bounds
