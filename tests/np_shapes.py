"""rv_world_edit_shapes restated in numpy from the comment in include/rvgrt.h, not from the C: dense [z, y, x]
bools, int64 arithmetic on whole coordinate grids, one inequality per kind.  A shape is (kind, solid, c2, r2)
with c2 and r2 in half-voxels; voxel v has its centre at 2 v + 1."""
import numpy as np

ELLIPSOID, CYLINDER_X, CYLINDER_Y, CYLINDER_Z = range(4)
MAX_SHAPES, MAX_R2, MAX_C2 = 256, 512, 1 << 20


def inside(shape_zyx, shape):
    """Bool [z, y, x] of a window of that shape: the voxels whose centres the shape contains."""
    kind, _, c2, r2 = shape
    Z, Y, X = shape_zyx
    d = [2 * np.arange(n, dtype=np.int64) + 1 - int(c) for n, c in zip((X, Y, Z), c2)]
    dx2, dy2, dz2 = (d[0] ** 2)[None, None, :], (d[1] ** 2)[None, :, None], (d[2] ** 2)[:, None, None]
    qx, qy, qz = (int(r) ** 2 for r in r2)
    # |d| can exceed r2 far outside the shape: cap the squares so that the products stay inside int64, at a
    # value that is outside on every axis (q + 1 > q)
    dx2, dy2, dz2 = np.minimum(dx2, qx + 1), np.minimum(dy2, qy + 1), np.minimum(dz2, qz + 1)
    if kind == ELLIPSOID:
        return dx2 * (qy * qz) + dy2 * (qx * qz) + dz2 * (qx * qy) <= qx * qy * qz
    if kind == CYLINDER_Y:
        return (dy2 <= qy) & (dx2 * qz + dz2 * qx <= qx * qz)
    if kind == CYLINDER_X:
        return (dx2 <= qx) & (dy2 * qz + dz2 * qy <= qy * qz)
    if kind == CYLINDER_Z:
        return (dz2 <= qz) & (dx2 * qy + dy2 * qx <= qx * qy)
    raise ValueError(kind)


def apply(vox, shapes):
    """(vox', n_set, n_cleared): the shapes in list order, a later one winning voxel by voxel; the counts
    compare the world before the call with the world after it."""
    out = vox.copy()
    for s in shapes:
        out[inside(vox.shape, s)] = bool(s[1])
    return out, int((out & ~vox).sum()), int((vox & ~out).sum())


def box(lg, shape):
    """The clipped box (x0, y0, z0, x1, y1, z1) of one shape, all zero when empty."""
    lo, hi = [], []
    for a in range(3):
        D, c, r = 1 << lg[a], int(shape[2][a]), int(shape[3][a])
        lo.append(max(0, (c - r) // 2))          # Python's // rounds towards -inf
        hi.append(min(D, (c + r + 1) // 2))
    if any(h <= l for l, h in zip(lo, hi)):
        return (0,) * 6
    return tuple(lo) + tuple(hi)


def boxes(lg, shapes):
    """(each, all): every shape's clipped box and their union (all zero when every box is empty)."""
    each = [box(lg, s) for s in shapes]
    live = [b for b in each if b != (0,) * 6]
    if not live:
        return each, (0,) * 6
    return each, tuple(min(b[a] for b in live) for a in range(3)) + tuple(max(b[3 + a] for b in live) for a in range(3))
