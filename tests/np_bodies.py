"""numpy restatement of rv_world_bodies_move (include/rvgrt.h), written from its definition: voxel by voxel
over a dense [z, y, x] occupancy, every float operation one separately rounded float32 operation.  Slow and
plain on purpose; the library's masked word tests are checked against it bit for bit."""
import math

import numpy as np

XN, XP, YN, YP, ZN, ZP, START_SOLID, EDGE, INVALID = 1, 2, 4, 8, 16, 32, 64, 128, 256
OPEN_EDGES = 1
F = np.float32
EPS = F(2.0 ** -7)


def solid(vox, open_edges, i, j, k):
    """(solid by the rule, a solid voxel inside the window) of cell (i, j, k)."""
    Z, Y, X = vox.shape
    if j >= Y:
        return False, False
    if j < 0:
        return True, False
    if i < 0 or i >= X or k < 0 or k >= Z:
        return (not open_edges), False
    v = bool(vox[k, j, i])
    return v, v


def occ(lo, size):
    """The cells an axis occupies: [floor(lo + EPS), ceil((lo + size) - EPS) - 1]."""
    lo, size = F(lo), F(size)
    return math.floor(F(lo + EPS)), math.ceil(F(F(lo + size) - EPS)) - 1


def box_cells(vox, open_edges, r):
    """(any cell solid, any window voxel solid) over the cells r = [(x0, x1), (y0, y1), (z0, z1)], inclusive."""
    any_solid = any_in = False
    for k in range(r[2][0], r[2][1] + 1):
        for j in range(r[1][0], r[1][1] + 1):
            for i in range(r[0][0], r[0][1] + 1):
                s, w = solid(vox, open_edges, i, j, k)
                any_solid |= s
                any_in |= w
    return any_solid, any_in


def valid(lo, size, delta):
    for a in range(3):
        if not (np.isfinite(lo[a]) and np.isfinite(size[a]) and np.isfinite(delta[a])):
            return False
        if not (abs(lo[a]) <= F(16384) and F(1 / 32) <= size[a] <= F(16) and abs(delta[a]) <= F(64)):
            return False
    return True


def move_one(vox, lo, size, delta, open_edges=False, slabs=None):
    """One body: (lo float32[3], flags).  slabs (a dict, optional) receives axis -> (blocking slab, the
    cross-section ranges it was tested with, the slabs scanned before it)."""
    lo = np.array(lo, F)
    size = np.asarray(size, F)
    delta = np.asarray(delta, F)
    if not valid(lo, size, delta):
        return lo, INVALID
    flags = START_SOLID if box_cells(vox, open_edges, [occ(lo[a], size[a]) for a in range(3)])[0] else 0
    for a in (1, 0, 2):
        d = delta[a]
        if d == 0:
            continue
        r = [occ(lo[b], size[b]) for b in range(3)]      # the cross-section at the current values
        t = F(lo[a] + d)
        c0, c1 = r[a]
        n0, n1 = occ(t, size[a])
        scan = range(c1 + 1, n1 + 1) if d > 0 else range(c0 - 1, n0 - 1, -1)
        before = []
        for i in scan:
            r[a] = (i, i)
            s, w = box_cells(vox, open_edges, r)
            if s:
                v = F(F(i) - size[a]) if d > 0 else F(i + 1)
                if (v > lo[a]) if d > 0 else (v < lo[a]):    # max / min that keep lo where the two are equal
                    lo[a] = v
                flags |= (2 if d > 0 else 1) << (2 * a)
                if not w:
                    flags |= EDGE
                if slabs is not None:
                    slabs[a] = (i, [tuple(x) for x in r], before)
                break
            before.append(i)
        else:
            lo[a] = t
    return lo, flags


def move(vox, lo, size, delta, flags=0):
    """n bodies: (lo (n, 3) float32, flags (n,) uint32).  size and delta broadcast against lo."""
    lo = np.asarray(lo, F).reshape(-1, 3)
    size = np.broadcast_to(np.asarray(size, F), lo.shape)
    delta = np.broadcast_to(np.asarray(delta, F), lo.shape)
    out = lo.copy()
    fl = np.zeros(len(lo), np.uint32)
    for n in range(len(lo)):
        if valid(lo[n], size[n], delta[n]):
            out[n], fl[n] = move_one(vox, lo[n], size[n], delta[n], bool(flags & OPEN_EDGES))
        else:
            fl[n] = INVALID                      # out[n] is the input's own bits
    return out, fl


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
SIZES = (1 / 32, 0.6, 1.0, 1.8, 2.0, 3.3)


def random_world(seed=5, n=32, density=0.08, floor=3):
    rng = np.random.default_rng(seed)
    vox = rng.uniform(size=(n, n, n)) < density
    vox[:, :floor, :] = True
    return vox


def random_bodies(rng, n, dims):
    """lo in [-2, dim + 2] per axis, half of the values snapped to integers; sizes from SIZES; deltas from
    {0, +-1, N(0, 3), N(0, 0.05)}."""
    lo = rng.uniform(size=(n, 3)) * (np.asarray(dims, np.float64) + 4.0) - 2.0
    snap = rng.uniform(size=(n, 3)) < 0.5
    lo = np.where(snap, np.round(lo), lo).astype(F)
    size = rng.choice(np.asarray(SIZES, F), (n, 3))
    kind = rng.integers(0, 5, (n, 3))
    delta = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                      [0.0, 1.0, -1.0, rng.normal(0, 3, (n, 3))], rng.normal(0, 0.05, (n, 3)))
    return lo, size.astype(F), np.clip(delta, -64, 64).astype(F)


def straddling_bodies(dims):
    """Bodies whose cross-sections cross every boundary of the word masks -- x = 7..8, 7..16 and 31..32, y =
    3..4 and 7..8, z = 7..8 -- and a 16-wide body, each pushed along every axis both ways from several
    heights.  dims = (X, Y, Z), X >= 34 not required: coordinates past the window meet its walls."""
    lo, size, delta = [], [], []
    spans = {0: [(7.0, 2.0), (7.0, 10.0), (31.0, 2.0), (6.5, 1.0)], 1: [(3.0, 2.0), (7.0, 2.0), (2.5, 3.3)],
             2: [(7.0, 2.0), (6.25, 1.8)]}
    for y in (3.0, 7.0, 10.5, dims[1] - 2.0):
        for (x, sx) in spans[0]:
            for (z, sz) in spans[2]:
                for (yy, sy) in [(y, 2.0)] + [s for s in spans[1]]:
                    for a in range(3):
                        for d in (-2.5, 1.75):
                            lo.append((x, yy, z))
                            size.append((sx, sy, sz))
                            delta.append(tuple(d if b == a else 0.0 for b in range(3)))
    for d in ((0, -40, 0), (3, -1, 0), (0, -1, -3), (-5, 2, 5)):
        lo.append((4.0, dims[1] - 20.0, 1.5))
        size.append((16.0, 16.0, 16.0))
        delta.append(d)
    return np.asarray(lo, F), np.asarray(size, F), np.asarray(delta, F)
