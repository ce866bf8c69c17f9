"""``contrastyou.augment.AffineTensorTransform`` on the host: the reference's draws and results (tests/golden/affine.npz, made by
tests/golden/make_golden_affine.py from the reference's class), the shapes it keeps, the dispatch, the declaration of the three new
entry points, and ``ops.affine_reach`` -- the host half of the backward kernel -- against a float64 restatement of the kernel's
search (tests/affine_ref.py)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import affine_ref as R
from contrastyou.augment import AffineTensorTransform, inverse_transform_matrix

SEEDS = (0, 1, 2)


@pytest.fixture()
def numpy_state():
    state = np.random.get_state()
    yield
    np.random.set_state(state)


@pytest.mark.parametrize("seed", SEEDS)
def test_draws_and_outputs_are_the_references(golden, numpy_state, seed):
    g = golden("affine")
    x = torch.from_numpy(g[f"seed{seed}/x"])
    tf = AffineTensorTransform()
    np.random.seed(seed)
    y, theta = tf(x)
    assert theta.dtype == torch.float32 and np.array_equal(theta.numpy(), g[f"seed{seed}/theta_ind"])          # bit for bit
    assert np.array_equal(y.numpy(), g[f"seed{seed}/y"])
    after_independent = np.random.rand()
    np.random.seed(seed)
    _, theta_dep = tf(x, independent=False)
    assert np.array_equal(theta_dep.numpy(), g[f"seed{seed}/theta_dep"])
    assert (theta_dep == theta_dep[0]).all() and not torch.equal(theta_dep[0], theta[0])
    # the matrix drawn before the `independent` branch is dropped: independent=True consumes 3 * (B + 1) numbers, False 3
    np.random.seed(seed)
    np.random.rand(3 * (x.shape[0] + 1))
    assert np.random.rand() == after_independent
    np.random.seed(seed)
    tf.get_random_affinematrix()
    assert np.array_equal(torch.stack([tf.get_random_affinematrix() for _ in range(3)]).numpy(), g[f"seed{seed}/theta_ind"])


@pytest.mark.parametrize("seed", SEEDS)
def test_inverse_replay_is_the_references(golden, seed):
    g = golden("affine")
    theta, y = torch.from_numpy(g[f"seed{seed}/theta_ind"]), torch.from_numpy(g[f"seed{seed}/y"])
    inv = inverse_transform_matrix(theta)
    assert inv.shape == (3, 2, 3) and np.array_equal(inv.numpy(), g[f"seed{seed}/theta_inv"])
    back, theta_back = AffineTensorTransform()(y, AffineMatrix=theta, inverse=True)
    assert np.array_equal(theta_back.numpy(), g[f"seed{seed}/theta_inv"])
    assert np.array_equal(back.numpy(), g[f"seed{seed}/back"])
    # ... and it inverts: [[A | t], [0 0 1]] times its inverse
    full = lambda m: torch.cat([m.double(), torch.tensor([[[0.0, 0.0, 1.0]]]).double().expand(len(m), 1, 3)], 1)
    assert (full(theta) @ full(inv) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6


def test_constructor_defaults_are_the_references():
    tf = AffineTensorTransform()
    assert (tf.min_rot, tf.max_rot, tf.min_shear, tf.max_shear, tf.min_scale, tf.max_scale, tf.mode) == (0, 180, 0.0, 0.5, 0.9, 1.1, "bilinear")


def test_two_and_three_dimensional_inputs_keep_their_shape(numpy_state):
    tf = AffineTensorTransform()
    np.random.seed(3)
    for shape in ((9, 7), (5, 9, 7), (2, 5, 9, 7)):
        x = torch.randn(*shape)
        y, theta = tf(x)
        assert y.shape == x.shape and theta.shape == (shape[0] if len(shape) == 4 else 1, 2, 3)
    # a [C, H, W] input is ONE sample of C channels, a [H, W] input one sample of one channel
    x = torch.randn(5, 9, 7)
    y3, theta = tf(x)
    y4, _ = tf(x[None], AffineMatrix=theta)
    assert torch.equal(y3, y4[0])
    with pytest.raises(AssertionError):
        tf(torch.randn(2, 5, 9, 7), AffineMatrix=theta)                 # one matrix for two samples


def test_cpu_tensors_do_not_take_the_gpu_dispatch(monkeypatch, numpy_state):
    from miseg_amd import ops

    def refuse(*a, **k):
        raise AssertionError("ops.affine_warp called for a CPU tensor")

    monkeypatch.setattr(ops, "affine_warp", refuse)
    x = torch.randn(2, 3, 9, 7, requires_grad=True)
    np.random.seed(4)
    for mode in ("bilinear", "nearest"):
        y, theta = AffineTensorTransform(mode=mode)(x)
        assert torch.allclose(y.double(), R.warp64(x.detach(), theta, mode), atol=R.forward_bound(9, 7, x.detach().abs().max()))
    y.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape


def test_ops_affine_warp_refuses_on_the_host():
    from miseg_amd import ops
    theta = torch.eye(2, 3).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="GPU"):
        ops.affine_warp(torch.randn(2, 3, 9, 7), theta)


def test_affine_symbols_are_declared_and_exported():
    from miseg_amd import _cabi
    names = set(_cabi.declared_symbols())
    new = {"miseg_affine_warp_fwd": 10, "miseg_affine_warp_bwd": 11, "miseg_affine_warp_supported": 5}
    assert set(new) <= names
    for name, nargs in new.items():
        assert len(_cabi.PROTOTYPES[name][1]) == nargs, name
    assert _cabi.PROTOTYPES["miseg_affine_warp_supported"][0] is ctypes.c_int64
    assert _cabi.PROTOTYPES["miseg_affine_warp_bwd"][1][9] is ctypes.c_int64                                  # reach
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(new) <= exported
    assert {n for n in exported if n.startswith("miseg_")} == names                                           # exactly the declared ones


def test_library_version_and_capability_query():
    from miseg_amd import _cabi
    lib = _cabi.lib()
    assert lib.miseg_version() >= 412
    q = lib.miseg_affine_warp_supported
    assert q(4, 256, 256, 1, 0) == 1 and q(1, 1, 1, 0, 1) == 1 and q(3, 2048, 2048, 0, 0) == 1
    assert q(4, 4096, 8, 0, 0) == -1 and q(4, 8, 2049, 1, 0) == -1 and q(0, 8, 8, 0, 0) == -1
    assert q(4, 8, 8, 2, 0) == -1 and q(4, 8, 8, 0, 2) == -1 and q(512, 2048, 2048, 0, 0) == -1               # 2^31 elements
    # refused on the host, before any launch (no device here)
    with pytest.raises(_cabi.MisegError, match="null pointer"):
        _cabi.call("miseg_affine_warp_fwd", None, None, None, 1, 1, 8, 8, 0, 0, None)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for bad in (dict(H=4096), dict(N=0), dict(mode=2), dict(channels_last=3), dict(reach=0), dict(reach=9)):
        a = dict(N=1, C=1, H=4, W=4, channels_last=0, mode=0, reach=3)
        a.update(bad)
        with pytest.raises(_cabi.MisegError):
            _cabi.call("miseg_affine_warp_bwd", None, p, p, a["N"], a["C"], a["H"], a["W"], a["channels_last"], a["mode"], a["reach"], p)
        if "reach" not in bad:
            with pytest.raises(_cabi.MisegError):
                _cabi.call("miseg_affine_warp_fwd", None, p, p, a["N"], a["C"], a["H"], a["W"], a["channels_last"], a["mode"], p)


# ---- ops.affine_reach: what the host promises the backward kernel

@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reach_covers_every_test_matrix_and_the_search_is_the_adjoint(shape):
    from miseg_amd import ops
    h, w, c = shape
    theta = R.thetas()
    _, g = R.inputs(shape, "bilinear")
    g = g[:, :2]
    want = R.warp64_bwd(g, theta, "bilinear")
    reaches = [ops.affine_reach(theta[i:i + 1], h, w) for i in range(R.N)]
    assert all(1 <= r <= ops.AFFINE_MAX_REACH for r in reaches), dict(zip(R.NAMES, reaches))
    assert ops.affine_reach(theta, h, w) == max(reaches)
    for i, r in enumerate(reaches):
        got = R.searched_adjoint64(g[i:i + 1], theta[i:i + 1], r)
        assert (got - want[i:i + 1]).abs().max() <= 1e-12 * max(1.0, float(want.abs().max())), (R.NAMES[i], r)
    rows = list(R.NEAREST_ROWS)
    got = R.searched_adjoint64(g[rows], theta[rows], max(reaches[i] for i in rows), "nearest")
    assert torch.equal(got, R.warp64_bwd(g[rows], theta[rows], "nearest"))


def test_the_restated_search_loses_weight_when_the_reach_is_too_small():
    """The check above can fail: scale 0.25 spreads the readers of one input pixel over 4 output pixels per axis."""
    from miseg_amd import ops
    theta = torch.tensor([[[0.25, 0, 0], [0, 0.25, 0]]])
    g = torch.ones(1, 1, 33, 33)
    want = R.warp64_bwd(g, theta, "bilinear")
    need = ops.affine_reach(theta, 33, 33)
    assert need == 5
    assert (R.searched_adjoint64(g, theta, need) - want).abs().max() < 1e-12
    assert (R.searched_adjoint64(g, theta, 2) - want).abs().max() > 1.0


def test_reach_of_the_default_ranges_and_of_matrices_the_kernel_cannot_cover(numpy_state):
    from miseg_amd import ops
    np.random.seed(11)
    tf = AffineTensorTransform()
    drawn = torch.stack([tf.get_random_affinematrix() for _ in range(500)])
    assert ops.affine_reach(drawn, 256, 256) <= 3                       # row sums <= 1.6 on square images
    assert ops.affine_reach(drawn, 33, 130) <= 6                        # <= 4.7 at 33 x 130
    eye = torch.eye(2, 3)[None]
    assert ops.affine_reach(eye, 64, 64) == 2
    assert ops.affine_reach(eye * 0.1, 64, 64) == 11                    # beyond the kernel's 8: the caller must refuse
    singular = torch.tensor([[[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]]])
    assert ops.affine_reach(singular, 64, 64) == 63 and ops.affine_reach(singular, 5, 7) == 6      # the whole image
    assert ops.affine_reach(torch.tensor([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0]]]), 5, 1) == 4        # a turned one-pixel-wide image
    assert ops.affine_reach(eye * 3e4, 2048, 2048) == 2                 # huge but well conditioned: nearly every pixel reads outside
    coarse = torch.tensor([[[1e4, 1e4, 0.0], [1e4, 10001.0, 0.0]]])    # row sums of |A^-1| = 2, but fp32 source points are ~40 px coarse
    assert ops.affine_reach(coarse, 2048, 2048) == 2047
    assert ops.affine_reach(torch.full((1, 2, 3), float("nan")), 64, 64) == 63


def test_affine_inverse_in_float64():
    from miseg_amd import ops
    theta = R.thetas()
    inv = ops.affine_inverse(theta)
    assert inv.dtype == torch.float32 and inv.shape == theta.shape
    assert (inv - inverse_transform_matrix(theta)).abs().max() < 1e-5
    with pytest.raises(ValueError, match="invertible"):
        ops.affine_inverse(torch.zeros(1, 2, 3))
