"""Shared by the affine-warp tests: the shapes and matrices, the float64 yardstick (torch on the CPU: ``F.affine_grid`` +
``F.grid_sample`` and its autograd -- never the code under test), the bounds the tests assert, and a float64 restatement of the
backward kernel's SEARCH (pre-image, clamp, box of half-width ``reach``) that the CPU tests use to check ``ops.affine_reach``.

Every reference is computed once per (shape, mode) and cached; callers must not write into what they get.
"""
import functools

import numpy as np
import torch
from torch.nn import functional as F

SHAPES = ((9, 7, 5), (16, 16, 3), (5, 1, 2), (1, 6, 2), (64, 48, 20), (33, 130, 4))          # (H, W, C)
DRAW_SEED = 20261019
EPS = 2.0 ** -23

_c, _s = float(np.cos(0.6)), float(np.sin(0.6))
FIXED = (
    ("identity", [[1, 0, 0], [0, 1, 0]]),
    ("flip_w", [[-1, 0, 0], [0, 1, 0]]),
    ("flip_h", [[1, 0, 0], [0, -1, 0]]),
    ("rot90", [[0, -1, 0], [1, 0, 0]]),
    ("rot180", [[-1, 0, 0], [0, -1, 0]]),
    ("shift1.5", [[1, 0, 1.5], [0, 1, -0.25]]),            # most of the image leaves: only x in [-1, -0.5] still reads inside
    ("scale0.5", [[0.5, 0, 0], [0, 0.5, 0]]),
    ("scale2_offset", [[2, 0, 0.3], [0, 2, -0.2]]),
    ("generic_shear", [[1.2 * _c, -0.8 * _s + 0.3, 0.11], [0.9 * _s, 0.7 * _c - 0.1, -0.07]]),
)
# ops.flip's masks (bit0 = H, bit1 = W) of the fixed matrices that are flips
FLIP_MASKS = {"identity": 0, "flip_w": 2, "flip_h": 1, "rot180": 3}
N_DRAWN = 4


@functools.lru_cache(maxsize=None)
def drawn():
    """Four matrices from ``AffineTensorTransform()`` (default ranges) under a fixed numpy seed; numpy's global state is put back."""
    from contrastyou.augment import AffineTensorTransform
    state = np.random.get_state()
    try:
        np.random.seed(DRAW_SEED)
        tf = AffineTensorTransform()
        return torch.stack([tf.get_random_affinematrix() for _ in range(N_DRAWN)])
    finally:
        np.random.set_state(state)


@functools.lru_cache(maxsize=None)
def thetas():
    """[13, 2, 3] fp32: the nine fixed matrices, then the four drawn ones."""
    fixed = torch.tensor([m for _, m in FIXED], dtype=torch.float32)
    return torch.cat([fixed, drawn()], 0)


NAMES = tuple(n for n, _ in FIXED) + tuple(f"drawn{i}" for i in range(N_DRAWN))
N = len(NAMES)
# nearest: the lattice matrices put every source point on a rounding tie or a lattice point by construction; the generic and drawn do not
NEAREST_ROWS = tuple(i for i, n in enumerate(NAMES) if n == "generic_shear" or n.startswith("drawn"))


def theta_for(mode):
    return thetas() if mode == "bilinear" else thetas()[list(NEAREST_ROWS)]


@functools.lru_cache(maxsize=None)
def inputs(shape, mode):
    """(x, g) fp32 [n, C, H, W], standard normal, seeded by the shape."""
    h, w, c = shape
    n = theta_for(mode).shape[0]
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + c + (0 if mode == "bilinear" else 7))
    return torch.randn(n, c, h, w, generator=gen), torch.randn(n, c, h, w, generator=gen)


def warp64(x, theta, mode):
    grid = F.affine_grid(theta.double(), list(x.shape), align_corners=True)
    return F.grid_sample(x.double(), grid, mode=mode, padding_mode="zeros", align_corners=True)


def warp64_bwd(g, theta, mode):
    x = torch.zeros(g.shape, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(warp64(x, theta, mode), x, g.double())
    return gx


@functools.lru_cache(maxsize=None)
def reference(shape, mode):
    """(y64, gx64, cov): the float64 forward of inputs()[0], the float64 backward of inputs()[1], and the largest entry of the
    float64 backward of an all-ones gradient (the weights that land on one input pixel)."""
    x, g = inputs(shape, mode)
    theta = theta_for(mode)
    return warp64(x, theta, mode), warp64_bwd(g, theta, mode), float(warp64_bwd(torch.ones_like(g), theta, mode).max())


def forward_bound(h, w, amax):
    """16 * 2^-23 * max(H, W) * max|x|: coordinates of magnitude up to max(H, W) pass through about a dozen fp32 roundings, and the
    interpolant's slope is at most 2 max|x| per pixel and axis."""
    return 16 * EPS * max(h, w) * float(amax)


def backward_bound(h, w, gmax, cov):
    return forward_bound(h, w, gmax) * 4 * max(1.0, cov)


def source_points64(theta, h, w):
    """float64 (sx, sy) [n, H, W]: where each output pixel reads, in pixels."""
    grid = F.affine_grid(theta.double(), [theta.shape[0], 1, h, w], align_corners=True)
    return (grid[..., 0] + 1) / 2 * (w - 1), (grid[..., 1] + 1) / 2 * (h - 1)


def away_from_ties(theta, h, w, margin=1e-3):
    """bool [n, H, W]: neither source coordinate lies within ``margin`` of k + 0.5."""
    sx, sy = source_points64(theta, h, w)
    dist = lambda s: (s - torch.floor(s) - 0.5).abs()
    return (dist(sx) > margin) & (dist(sy) > margin)


def searched_adjoint64(g, theta, reach, mode="bilinear"):
    """The backward kernel's algorithm in float64 numpy (csrc/affine.hip): every input pixel q rounds its pre-image A^-1 (q - b) to a
    pixel, clamps it into the image and sums w(p, q) g[p] over the output pixels p of the (2 reach + 1)^2 box around it.  With a
    sufficient ``reach`` this IS the adjoint; with too small a one it loses weight."""
    g = g.double().numpy()
    n, c, h, w = g.shape
    sx, sy = (s.numpy() for s in source_points64(theta, h, w))
    t = theta.double().numpy()
    out = np.zeros_like(g)
    qy, qx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for b in range(n):
        both = h > 1 and w > 1
        a00 = t[b, 0, 0] if w > 1 else 1.0
        a11 = t[b, 1, 1] if h > 1 else 1.0
        a01 = t[b, 0, 1] * (w - 1) / (h - 1) if both else 0.0
        a10 = t[b, 1, 0] * (h - 1) / (w - 1) if both else 0.0
        b0, b1 = sx[b, 0, 0], sy[b, 0, 0]
        det = a00 * a11 - a01 * a10
        with np.errstate(all="ignore"):
            u, v = qx - b0, qy - b1
            cj = np.rint(np.fmin(np.fmax((a11 * u - a01 * v) / det, 0.0), w - 1)).astype(np.int64)
            ci = np.rint(np.fmin(np.fmax((a00 * v - a10 * u) / det, 0.0), h - 1)).astype(np.int64)
        if mode == "bilinear":
            x0, y0 = np.floor(sx[b]), np.floor(sy[b])
            fx, fy = sx[b] - x0, sy[b] - y0
        else:
            x0, y0 = np.rint(sx[b]), np.rint(sy[b])
            fx, fy = np.zeros_like(x0), np.zeros_like(y0)
        for di in range(-reach, reach + 1):
            for dj in range(-reach, reach + 1):
                pi, pj = ci + di, cj + dj
                ok = (pi >= 0) & (pi < h) & (pj >= 0) & (pj < w)
                pi, pj = np.clip(pi, 0, h - 1), np.clip(pj, 0, w - 1)
                dx, dy = qx - x0[pi, pj], qy - y0[pi, pj]
                nt = 1 if mode == "bilinear" else 0
                hit = ok & (dx >= 0) & (dx <= nt) & (dy >= 0) & (dy <= nt)
                wgt = np.where(dx == 1, fx[pi, pj], 1 - fx[pi, pj]) * np.where(dy == 1, fy[pi, pj], 1 - fy[pi, pj])
                out[b] += np.where(hit, wgt, 0.0)[None] * g[b][:, pi, pj]
    return torch.from_numpy(out)
