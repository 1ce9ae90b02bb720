"""rv_world_fall restated from its definition (include/rvgrt.h) over a dense [z, y, x] boolean array: the
components come from np_detached.detached, a component's clearance is found by trying e = 1, 2, ... on the
shifted component against everything that is not the component, and all components move at once.  Plain and
slow on purpose; it shares no code with the library.  It asserts the definition's facts 1-4 itself."""
import numpy as np

import np_detached as D

FALLEN = np.dtype([("comp", D.COMPONENT), ("fall", np.int32), ("flags", np.uint32)])
STOPPED = 1


def components(vox, box):
    """(COMPONENT records in seed order, one dense world-sized boolean array per component)."""
    x0, y0, z0, x1, y1, z1 = box
    comps, _, _, det = D.detached(vox, box)
    cells = []
    for c in comps:
        # the component of a seed: grow from it through the detached voxels
        part = np.zeros(det.shape, bool)
        sx, sy, sz = c["seed"]
        part[sz - z0, sy - y0, sx - x0] = True
        while True:
            grow = part.copy()
            grow[1:] |= part[:-1]
            grow[:-1] |= part[1:]
            grow[:, 1:] |= part[:, :-1]
            grow[:, :-1] |= part[:, 1:]
            grow[:, :, 1:] |= part[:, :, :-1]
            grow[:, :, :-1] |= part[:, :, 1:]
            grow &= det
            if np.array_equal(grow, part):
                break
            part = grow
        assert part.sum() == c["voxels"]
        full = np.zeros(vox.shape, bool)
        full[z0:z1, y0:y1, x0:x1] = part
        cells.append(full)
    return comps, cells


def lowered(a, e):
    """a moved down by e rows; None when a voxel would pass the floor."""
    if e == 0:
        return a.copy()
    if a[:, :e].any():
        return None
    out = np.zeros_like(a)
    out[:, :-e] = a[:, e:]
    return out


def clearance(vox, part):
    others = vox & ~part
    d = 0
    while True:
        low = lowered(part, d + 1)
        if low is None or (low & others).any():
            return d
        d += 1


def measured(vox, box):
    """What does not depend on max_fall, for fall(..., parts=): (components, their cells, their clearances)."""
    comps, cells = components(vox, box)
    return comps, cells, np.array([clearance(vox, p) for p in cells], np.int64)


def fall(vox, box, max_fall=0, parts=None):
    """(FALLEN records in seed order, detached voxels, the changed box as a tuple, the world after the move,
    the clearances)."""
    comps, cells, clear = parts or measured(vox, box)
    out = np.zeros(len(comps), FALLEN)
    out["comp"] = comps
    moved = np.zeros(vox.shape, bool)
    left = np.zeros(vox.shape, bool)
    landed = np.zeros(vox.shape, np.int32)
    for k, part in enumerate(cells):
        c = int(clear[k])
        assert c >= 1, "fact 1"
        f = c if max_fall == 0 else min(c, max_fall)
        out[k]["fall"] = f
        out[k]["flags"] = STOPPED if f == c else 0
        left |= part
        low = lowered(part, f)
        landed += low
        moved |= low
    rest = vox & ~left
    assert not (moved & rest).any(), "fact 2"
    assert landed.max(initial=0) <= 1, "fact 3"
    after = rest | moved
    assert after.sum() == vox.sum(), "fact 4"
    touched = left | moved
    if touched.any():
        zs, ys, xs = np.nonzero(touched)
        changed = (int(xs.min()), int(ys.min()), int(zs.min()), int(xs.max()) + 1, int(ys.max()) + 1, int(zs.max()) + 1)
    else:
        changed = (0, 0, 0, 0, 0, 0)
    return out, int(left.sum()), changed, after, clear


def settle(vox, box, max_fall=0, max_rounds=64):
    """fall repeated over each round's changed box until nothing is detached: (rounds that moved something, the
    union of the changed boxes, the final world)."""
    rounds, union = 0, None
    while rounds < max_rounds:
        out, _, changed, after, _ = fall(vox, box, max_fall)
        if len(out) == 0:
            break
        rounds += 1
        union = changed if union is None else (tuple(min(a, c) for a, c in zip(union[:3], changed[:3])) +
                                               tuple(max(a, c) for a, c in zip(union[3:], changed[3:])))
        vox, box = after, changed
    return rounds, union or (0, 0, 0, 0, 0, 0), vox


# ---------------------------------------------------------------- scenes the CPU and the GPU tests share
def ground(n=32, h=4):
    vox = np.zeros((n, n, n), bool)
    vox[:, :h, :] = True
    return vox


def island(y, slab=None):
    """A 3^3 block at (12, y, 12), over a ground slab of `slab` rows or over nothing."""
    vox = np.zeros((32, 32, 32), bool) if slab is None else ground(32, slab)
    vox[12:15, y:y + 3, 12:15] = True
    return vox


def stack():
    """Ground y < 4, block B 3^3 at y 8..10, block A 3^3 at y 14..16 above it.  Returns (vox, box)."""
    vox = ground()
    vox[12:15, 8:11, 12:15] = True
    vox[12:15, 14:17, 12:15] = True
    return vox, (8, 4, 8, 20, 20, 20)


def u_scene():
    """A: a bar at y 16 over x 10..20 with legs down to y 8 at x 10 and x 20; B: a 3 x 2 block at y 12..13
    under the bar; ground y < 4; all in the slice z = 12.  Returns (vox, box)."""
    vox = ground()
    vox[12, 16, 10:21] = True
    vox[12, 8:17, 10] = True
    vox[12, 8:17, 20] = True
    vox[12, 12:14, 14:17] = True
    return vox, (6, 4, 8, 26, 22, 18)


def c_shape():
    """One component in the slice z = 12: an upper arm at y 20 over x 8..19, a back at x 8 from y 17 to 20, a
    lower arm at y 17 over x 8..13, two empty rows under the upper arm's inner half.  Ground: 4 rows, 13
    under the lower arm, and a step up to y < 15 under the upper arm's open side, x 16..19, 5 under it: the
    step decides (5), not the own arm (2) and not the ground (13).  Returns (vox, box)."""
    vox = ground()
    vox[12, :15, 16:20] = True
    vox[12, 20, 8:20] = True
    vox[12, 17:21, 8] = True
    vox[12, 17, 8:14] = True
    return vox, (4, 10, 8, 28, 26, 18)


def checker_rows():
    """The checkerboard's rows 8..12 over an empty lower half.  Returns (vox, box)."""
    vox = np.zeros((32, 32, 32), bool)
    vox[:, 8:13, :] = D.checkerboard()[:, 8:13, :]
    return vox, (1, 8, 1, 31, 13, 31)
