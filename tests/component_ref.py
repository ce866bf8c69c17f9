"""Host references for ``miseg_largest_component`` (include/miseg_hip.h) and the masks the component tests share.  A helper, not a
test.

``keep_ref`` is the definition: ``scipy.ndimage.label`` per (unit, class), ``np.bincount`` for the sizes, ``np.argmax`` for the kept
component (scipy numbers components in raster order of their first pixel, so the first of equals wins).  ``keep_brute`` is a plain
flood fill with an explicit stack over a padded flat copy of the unit -- no scipy, no labelling pass -- so the two share nothing but
the definition.  Both return ``(out int64 [N, H, W], labels int32 [N, H, W], stats int64 [U, K, 3])``."""
from functools import lru_cache

import numpy as np


def keep_ref(pred, classes, rank=2, connectivity=1, fill=0):
    from scipy.ndimage import generate_binary_structure, label
    pred = np.asarray(pred)
    structure = generate_binary_structure(rank, 1 if connectivity == 1 else rank)
    out, labels = pred.copy(), np.full(pred.shape, -1, np.int32)
    units = [slice(None)] if rank == 3 else list(range(len(pred)))
    stats = np.zeros((len(units), len(classes), 3), np.int64)
    for u, sel in enumerate(units):
        for k, c in enumerate(classes):
            lab, count = label(pred[sel] == c, structure=structure)
            if count == 0:
                continue
            sizes = np.bincount(lab.ravel())
            keep = int(np.argmax(sizes[1:])) + 1
            stats[u, k] = (count, sizes[keep], sizes[1:].sum())
            out[sel][(lab > 0) & (lab != keep)] = fill
            flat = lab.ravel()
            first = np.full(count + 1, flat.size, np.int64)
            np.minimum.at(first, flat, np.arange(flat.size))  # the smallest pixel index of every label
            labels[sel][lab > 0] = first[lab[lab > 0]]
    return out, labels, stats


def keep_brute(pred, classes, rank=2, connectivity=1, fill=0):
    pred = np.asarray(pred)
    n, h, w = pred.shape
    out, labels = pred.copy(), np.full(pred.shape, -1, np.int32)
    units = [pred] if rank == 3 else [pred[b:b + 1] for b in range(n)]
    stats = np.zeros((len(units), len(classes), 3), np.int64)
    for u, unit in enumerate(units):
        d = unit.shape[0]
        ph, pw = h + 2, w + 2
        padded = np.full((d + 2, ph, pw), -1, np.int64)
        padded[1:-1, 1:-1, 1:-1] = unit
        val = padded.ravel().tolist()
        offsets = []
        for dz in ((-1, 0, 1) if rank == 3 else (0,)):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dz, dy, dx) != (0, 0, 0) and (connectivity == 2 or abs(dz) + abs(dy) + abs(dx) == 1):
                        offsets.append((dz * ph + dy) * pw + dx)
        seen = [False] * len(val)
        found = {c: [] for c in classes}                      # class -> [(first pixel, members)] in raster order of the first pixel
        for z in range(d):
            for y in range(h):
                for x in range(w):
                    p = ((z + 1) * ph + y + 1) * pw + x + 1
                    c = val[p]
                    if seen[p] or c not in found:
                        continue
                    seen[p] = True
                    stack, members = [p], []
                    while stack:
                        q = stack.pop()
                        members.append(q)
                        for o in offsets:
                            r = q + o
                            if val[r] == c and not seen[r]:
                                seen[r] = True
                                stack.append(r)
                    found[c].append(((z * h + y) * w + x, members))
        base = 0 if rank == 3 else u
        for k, c in enumerate(classes):
            comps = found[c]
            if not comps:
                continue
            best = 0
            for i in range(1, len(comps)):
                if len(comps[i][1]) > len(comps[best][1]):    # strictly larger: the earlier of equals stays
                    best = i
            stats[u, k] = (len(comps), len(comps[best][1]), sum(len(m) for _, m in comps))
            for i, (first, members) in enumerate(comps):
                for q in members:
                    z, rem = divmod(q, ph * pw)
                    y, x = divmod(rem, pw)
                    labels[base + z - 1, y - 1, x - 1] = first
                    if i != best:
                        out[base + z - 1, y - 1, x - 1] = fill
    return out, labels, stats


# ------------------------------------------------------------------------------------------ the mask zoo (values 0..3 and 5, N = 3)
def _rects(rng, h, w):
    m = np.zeros((h, w), np.int64)
    for c in (1, 2, 3, 1, 2, 3):
        y, x = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
        m[y:y + int(rng.integers(1, max(h // 3, 2))), x:x + int(rng.integers(1, max(w // 3, 2)))] = c
    return m


@lru_cache(maxsize=None)
def zoo(h, w):
    """[(name, pred)], int64 [3, h, w] each, read-only; h, w >= 8."""
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    out.append(("empty", np.zeros((3, h, w), np.int64)))
    p = np.zeros((3, h, w), np.int64)
    p[:, 0, 0], p[:, h - 1, w - 1], p[:, 0, w - 1], p[:, h - 1, 0] = 1, 1, 2, 3
    out.append(("corners", p))
    out.append(("full", np.stack([np.full((h, w), c, np.int64) for c in (1, 2, 1)])))
    board = np.where((yy + xx) % 2 == 0, 1, 2).astype(np.int64)
    out.append(("checkerboard", np.stack([board, 3 - board, board])))
    # two equal discs of class 1 (the tie: the earlier one stays); two unequal squares of class 2, the later one larger
    p = np.zeros((3, h, w), np.int64)
    r = max(1, min(h, w) // 6)
    for cy, cx in ((h // 4, w // 4), (h - 1 - h // 4, w - 1 - w // 4)):
        p[:, (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    p[:, 0:2, w - 2:w], p[:, h - 3:h, 0:3] = 2, 2
    out.append(("equal_discs", p))
    step = max(min(h, w) / 9.0, 1.0)
    ring = (np.sqrt((yy - h / 2) ** 2 + (xx - w / 2) ** 2) / step).astype(np.int64)
    out.append(("rings", np.stack([ring % 2 + 1, (ring + 1) % 2 + 1, ring % 3 + 1])))
    p = np.zeros((3, h, w), np.int64)
    p[:, :h - 1, ::2], p[:, h - 1, :] = 1, 1
    p[2] = p[2].T[:h, :w] if h == w else p[2][::-1]           # slice 2: the comb on its side (square) or joined in the first row
    out.append(("comb", p))
    p = np.zeros((3, h, w), np.int64)
    p[:, ::2, :] = 1
    for y in range(1, h, 2):
        p[:, y, (w - 1) if (y // 2) % 2 == 0 else 0] = 1
    p[1] = np.where(p[1] == 1, 3, 0)
    out.append(("serpentine", p))
    p = np.zeros((3, h, w), np.int64)
    for i in range(min(h, w)):
        p[:, i, i] = 1
        if p[0, i, w - 1 - i] == 0:
            p[:, i, w - 1 - i] = 2
    out.append(("diagonal", p))
    # blobs that touch only across a slice boundary: face to face (slices 0 / 1) and corner to corner (slices 1 / 2)
    p = np.zeros((3, h, w), np.int64)
    p[0, 0:2, 0:2], p[1, 0:2, 0:2], p[2, 2:4, 2:4] = 1, 1, 1
    p[1, h - 2:h, w - 3:w], p[2, h - 3:h, w - 3:w] = 1, 1
    p[0, h - 1, 0], p[2, h - 1, 0] = 3, 3
    out.append(("across_slices", p))
    p = np.stack([_rects(rng, h, w) for _ in range(3)])
    p[0][p[0] == 2] = 0
    p[2][p[2] == 3] = 0
    p[2][p[2] == 1] = 0
    out.append(("absent", p))
    out.append(("noise", np.where(rng.random((3, h, w)) < 0.55, rng.integers(1, 4, (3, h, w)), 0).astype(np.int64)))
    p = np.where(rng.random((3, h, w)) < 0.6, rng.integers(1, 4, (3, h, w)), 0).astype(np.int64)
    p[:, h // 3:h // 3 + 2, :], p[:, :, w // 2] = 5, 5
    out.append(("unlisted_value", p))
    for _, a in out:
        a.setflags(write=False)
    return out


CPU_SHAPES = ((8, 8), (24, 40), (37, 53), (65, 130))
GPU_SHAPES = ((8, 8), (24, 40), (37, 53), (64, 64), (65, 130), (130, 67))
CLASS_LISTS = ((1, 2, 3), (3, 1))


@lru_cache(maxsize=None)
def zoo_ref(h, w, classes, rank, connectivity):
    """{name: keep_ref(...)} of ``zoo(h, w)``: computed once, shared by every test that needs it, never written to."""
    return {name: keep_ref(p, classes, rank, connectivity) for name, p in zoo(h, w)}


def spiral(size=512):
    """One slice with a one-pixel-wide spiral of class 1 from the border towards the centre (a blank line between its turns) and a
    separate 3 x 3 block of class 1 in the centre, which the spiral stops short of.  Returns (pred [1, size, size], spiral length)."""
    m = np.zeros((size, size), np.int64)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    path = [(0, 0)]

    def free(a, b):
        return not (0 <= a < size and 0 <= b < size) or m[a, b] == 0

    while True:
        for _ in range(2):                                    # straight on, else one turn to the right, else the end
            ny, nx = y + dy, x + dx
            if 0 <= ny < size and 0 <= nx < size and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            break
        y, x = ny, nx
        m[y, x] = 1
        path.append((y, x))
    for yy, xx in path[-220:]:                                # clear the innermost turns: room for the block
        m[yy, xx] = 0
    c = size // 2
    m[c - 1:c + 2, c - 1:c + 2] = 1
    return m[None], len(path) - 220
