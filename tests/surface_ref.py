"""Host references for ``miseg_surface_stats`` (include/miseg_hip.h) and the masks the surface tests share.  A helper, not a test.

``stats_ref`` goes through ``scipy.ndimage.distance_transform_edt(..., return_indices=True)`` and takes the squared distance as
an integer from the returned indices; ``stats_brute`` finds the border by comparing neighbours and the distances by comparing every
border pixel with every border pixel -- no erosion, no distance transform -- so the two share nothing but the definition."""
import math
from functools import lru_cache

import numpy as np


# ------------------------------------------------------------------------------------------ squared distances, two ways
def _border_scipy(m):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    return m ^ binary_erosion(m, structure=generate_binary_structure(2, 1), iterations=1)      # MedPy 0.4.0 __surface_distances


def _border_neighbours(m):
    p = np.pad(m, 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def _sq_edt(src, dst):
    """Squared distances (int64, ascending) from the border pixels of ``src`` to the nearest border pixel of ``dst``."""
    from scipy.ndimage import distance_transform_edt
    bs, bd = _border_scipy(src), _border_scipy(dst)
    idx = distance_transform_edt(~bd, return_distances=False, return_indices=True)
    yy, xx = np.nonzero(bs)
    sq = (idx[0][yy, xx].astype(np.int64) - yy) ** 2 + (idx[1][yy, xx].astype(np.int64) - xx) ** 2
    return np.sort(sq)


def _sq_brute(src, dst):
    ps, pd = np.argwhere(_border_neighbours(src)).astype(np.int64), np.argwhere(_border_neighbours(dst)).astype(np.int64)
    out = np.empty(len(ps), np.int64)
    for i0 in range(0, len(ps), 512):                       # chunks keep the n x n table small
        d = ps[i0:i0 + 512, None, :] - pd[None, :, :]
        out[i0:i0 + 512] = (d * d).sum(-1).min(1)
    return np.sort(out)


def _distances(pred, target, classes, sq_fn):
    """{(b, k, direction): ascending int64 squared distances}, or None where either mask of (b, k) is empty."""
    pred, target = np.asarray(pred), np.asarray(target)
    out = {}
    for b in range(pred.shape[0]):
        for k, c in enumerate(classes):
            p, t = pred[b] == c, target[b] == c
            if not p.any() or not t.any():
                out[b, k, 0] = out[b, k, 1] = None
            else:
                out[b, k, 0], out[b, k, 1] = sq_fn(p, t), sq_fn(t, p)
    return out


def distances_ref(pred, target, classes):
    return _distances(pred, target, classes, _sq_edt)


def distances_brute(pred, target, classes):
    return _distances(pred, target, classes, _sq_brute)


def stats_from(dist, n_samples, n_classes, q):
    """The kernel's two outputs from a ``distances_*`` table: stats int64 [N, K, 2, 4] = (n, max_sq, qlo_sq, qhi_sq) with the ranks
    floor(v), ceil(v) of v = (n - 1) * q, and sum_dist float64 [N, K, 2] = the correctly rounded sum of the square roots."""
    stats = np.zeros((n_samples, n_classes, 2, 4), np.int64)
    sums = np.zeros((n_samples, n_classes, 2), np.float64)
    for (b, k, d), sq in dist.items():
        if sq is None:
            continue
        n = len(sq)
        v = (n - 1) * float(q)
        stats[b, k, d] = (n, sq[-1], sq[int(math.floor(v))], sq[int(math.ceil(v))])
        sums[b, k, d] = math.fsum(np.sqrt(sq.astype(np.float64)))
    return stats, sums


def stats_ref(pred, target, classes, q):
    return stats_from(distances_ref(pred, target, classes), len(pred), len(classes), q)


def stats_brute(pred, target, classes, q):
    return stats_from(distances_brute(pred, target, classes), len(pred), len(classes), q)


# ------------------------------------------------------------------------------------------ the mask zoo (labels 0..3, N = 3)
def _blobs(rng, h, w):
    """Three rectangles, one per class 1..3, in separate thirds of the width: every class is present."""
    m = np.zeros((h, w), np.int64)
    for c in (1, 2, 3):
        x0, x1 = (c - 1) * w // 3, c * w // 3
        ya, xa = int(rng.integers(0, max(h // 2, 1))), int(rng.integers(x0, max((x0 + x1) // 2, x0 + 1)))
        m[ya:ya + max(int(rng.integers(1, h // 2 + 1)), 1), xa:max(xa + 1, min(x1, xa + int(rng.integers(1, w // 3 + 1))))] = c
    return m


@lru_cache(maxsize=None)
def zoo(h, w):
    """[(name, pred, target)], int64 [3, h, w] each, read-only.  ``FULL`` below names the entries in which classes 1..3 are present
    in every slice of both masks (what a meter needs to record a batch)."""
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    # one pixel per class, each in a corner (the corners rotate with the sample)
    corners = [(0, 0), (0, w - 1), (h - 1, w - 1), (h - 1, 0)]
    p, t = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    for b in range(3):
        for c in (1, 2, 3):
            p[(b,) + corners[(c + b) % 4]] = c
            t[(b,) + corners[(c + b + 2) % 4]] = c
    out.append(("corners", p, t))
    # an object touching all four image edges (a cross), against a thicker, shifted one; classes 2, 3 as small blocks
    p, t = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    for b in range(3):
        p[b, h // 2 - 1:h // 2 + 1, :] = 1
        p[b, :, w // 2 - 1:w // 2 + 1] = 1
        t[b, h // 2 - 1 + b:h // 2 + 2 + b, :] = 1
        t[b, :, w // 2 - 2:w // 2 + 1 + b] = 1
        p[b, 0:2, 0:2], t[b, 0:1, 0:3] = 2, 2
        p[b, h - 2:h, 0:1], t[b, h - 1:h, 0:2] = 3, 3
    out.append(("cross", p, t))
    # a mask that fills the image: its border is the frame (classes 2, 3 absent from pred: zero rows)
    p, t = np.ones((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    for b in range(3):
        t[b, h // 4:h // 4 + h // 2 + b, w // 4:w // 4 + w // 2] = 1
        t[b, 0, 0] = 2
    out.append(("full", p, t))
    # pred == target: every distance is zero
    p = np.stack([_blobs(rng, h, w) for _ in range(3)])
    out.append(("same", p, p.copy()))
    # two objects in opposite corners: the largest distances the shape allows
    p, t = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    for b in range(3):
        p[b, 0:1 + b, 0:2], t[b, h - 2:h, w - 1 - b:w] = 1, 1
        p[b, 0:2, w - 2:w], t[b, h - 1:h, 0:1 + b] = 2, 2
        p[b, h - 1:h, w - 2 - b:w], t[b, 0:1, 0:1] = 3, 3
    out.append(("opposite", p, t))
    # a checkerboard of classes 1 and 2: every pixel is a border pixel; against its negative, 2x2 cells, and itself
    board = np.where((yy + xx) % 2 == 0, 1, 2).astype(np.int64)
    coarse = np.where((yy // 2 + xx // 2) % 2 == 0, 1, 2).astype(np.int64)
    out.append(("checkerboard", np.stack([board, board, board]), np.stack([3 - board, coarse, board])))
    # concentric rings of classes 0..3, the target's centre shifted
    p, t = np.zeros((3, h, w), np.int64), np.zeros((3, h, w), np.int64)
    step = max(min(h, w) / 9.0, 1.0)
    for b in range(3):
        p[b] = (np.sqrt((yy - h / 2) ** 2 + (xx - w / 2) ** 2) / step).astype(np.int64) % 4
        t[b] = (np.sqrt((yy - h / 2 - 1 - b) ** 2 + (xx - w / 2 + 2) ** 2) / step).astype(np.int64) % 4
    out.append(("rings", p, t))
    # class 2 missing from pred in slice 0, class 3 missing from target in slice 2: zero rows that must not disturb their neighbours
    p, t = np.stack([_blobs(rng, h, w) for _ in range(3)]), np.stack([_blobs(rng, h, w) for _ in range(3)])
    p[0][p[0] == 2] = 0
    t[2][t[2] == 3] = 0
    out.append(("missing", p, t))
    for _, a, b2 in out:
        a.setflags(write=False)
        b2.setflags(write=False)
    return out


FULL = ("corners", "cross", "opposite", "rings")
SHAPES = ((8, 8), (24, 40), (37, 53), (64, 64))


@lru_cache(maxsize=None)
def zoo_distances(h, w, classes):
    """{name: distances_ref table} of ``zoo(h, w)`` for a tuple of classes: computed once, shared by every test that needs it."""
    return {name: distances_ref(p, t, classes) for name, p, t in zoo(h, w)}


def discs(n, size, seed):
    """``n`` slices with three random discs (classes 1..3) per mask, fixed seed."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    p, t = np.zeros((n, size, size), np.int64), np.zeros((n, size, size), np.int64)
    for m in (p, t):
        for b in range(n):
            for c in (1, 2, 3):
                cy, cx, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(size / 16, size / 4)
                m[b][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = c
    return p, t
