"""Host-side restatements of the world calls that CPU and GPU tests share: rv_world_scroll_region's plan
and the scrolled window on the oracle, the column bits rv_world_persist keeps, and rv_gi_relight on the
oracle's grid."""
import numpy as np

from gpu_world import gi_dims, pack, voxels


# ---------------------------------------------------------------- rv_world_scroll
def expected_plan(lg, axis, d):
    """(trailing, leading, cells, full) restated: k = |d| / 2 cells; the final byte can change within 64
    cells of the face the old planes left through and of the entering planes."""
    S = [1 << (l - 1) for l in lg]
    Sa, k = S[axis], abs(d) // 2
    whole = (0, S[0], 0, S[1], 0, S[2])
    if d == 0:
        return (0,) * 6, (0,) * 6, 0, False
    if d > 0:
        tr, ld = (0, min(Sa, 64)), (max(0, Sa - k - 64), Sa)
        touch = ld[0] <= tr[1]
    else:
        tr, ld = (max(0, Sa - 64), Sa), (0, min(Sa, k + 64))
        touch = tr[0] <= ld[1]
    if abs(d) >= 2 * Sa or touch or 640 + 4 * k >= 4 * Sa:
        return whole, (0,) * 6, S[0] * S[1] * S[2], True
    boxes = []
    for r in (tr, ld):
        b = list(whole)
        b[2 * axis], b[2 * axis + 1] = r
        boxes.append(tuple(b))
    cross = S[0] * S[1] * S[2] // Sa
    return boxes[0], boxes[1], ((tr[1] - tr[0]) + (ld[1] - ld[0])) * cross, False


ORIGIN = (40, -24)   # the old window's origin on the terrain
# Seeds of the density-1e-6 worlds (4 solid voxels) in which the oracle alone shows a byte that differs
# >= 48 cells from the trailing face: one of the voxels leaves with the old planes and was the nearest
# solid of cells that far into the retained part.  (The entering terrain reaches as far by itself.)
SPARSE_SEEDS = {
    ((10, 6, 6), 0, 8): 1119, ((10, 6, 6), 0, -8): 1036, ((10, 6, 6), 0, 64): 1005, ((10, 6, 6), 0, -64): 1049,
    ((6, 6, 10), 2, 8): 1036, ((6, 6, 10), 2, -8): 1074, ((6, 6, 10), 2, 64): 1009, ((6, 6, 10), 2, -64): 1037,
    ((10, 6, 6), 0, 40): 1060, ((6, 6, 10), 2, 40): 1027,
}

_TERRAIN = {}


def terrain(oracle, lg, ox, oz):
    """Voxels [z, y, x] of the generated window at origin (ox, oz)."""
    key = (lg, ox, oz)
    if key not in _TERRAIN:
        _TERRAIN[key] = oracle.OracleWorld(*lg, ox=ox, oz=oz).fill().voxels()
    return _TERRAIN[key]


def scrolled(oracle, lg, axis, d, old_bits, origin=ORIGIN):
    """(expected bits, old CSDF moved to the new indices with 255 where a cell entered, expected CSDF) of a
    window at `origin` holding old_bits, moved by d voxels along axis."""
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = old_bits
    ow.build_csdf()
    S = tuple(1 << (l - 1) for l in lg)
    ax = 2 - axis   # numpy axis of [z, y, x]
    vox = np.roll(ow.voxels(), -d, axis=ax)
    old = np.roll(ow.csdf.reshape(S[2], S[1], S[0]), -d // 2, axis=ax)
    new_org = (origin[0] + (d if axis == 0 else 0), origin[1] + (d if axis == 2 else 0))
    gen = terrain(oracle, lg, *new_org)
    n = vox.shape[ax]
    ent = [slice(None)] * 3
    ent[ax] = slice(n - d, n) if d > 0 else slice(0, -d)
    vox[tuple(ent)] = gen[tuple(ent)]
    ent[ax] = slice(n // 2 - d // 2, n // 2) if d > 0 else slice(0, -d // 2)
    old[tuple(ent)] = 255
    nw = oracle.OracleWorld(*lg)
    nw.bits[:] = pack(vox)
    nw.build_csdf()
    return nw.bits, old, nw.csdf.reshape(S[2], S[1], S[0])


def reaches(axis, d, S, diff):
    """How far the differing cells reach from the trailing face and before the entering planes (cells)."""
    c = np.nonzero(diff)[2 - axis]
    Sa, k = S[axis], abs(d) // 2
    if d > 0:
        tr, ld = c[c < Sa // 2], c[c >= Sa // 2]
        return (int(tr.max()) if len(tr) else -1), (Sa - k - 1 - int(ld.min()) if len(ld) else -1)
    tr, ld = c[c >= Sa // 2], c[c < Sa // 2]
    return (Sa - 1 - int(tr.min()) if len(tr) else -1), (int(ld.max()) - k if len(ld) else -1)


# ---------------------------------------------------------------- rv_world_persist
def column_bits(vox, bx, bz):
    """Column bits of brick column (bx, bz): RV_WORLD_BITS' layout for log2 dims (3, ly, 3)."""
    return np.packbits(vox[8 * bz:8 * bz + 8, :, 8 * bx:8 * bx + 8].reshape(-1), bitorder="little").view(np.uint32)


# ---------------------------------------------------------------- rv_gi_relight
def _rows(lg, box):
    GX, GY, _ = gi_dims(lg)
    x0, y0, z0, x1, y1, z1 = box
    return [x0 + GX * (y + GY * z) for z in range(z0, z1) for y in range(y0, y1)], x1 - x0


def _in_box(lg, box):
    GX, GY, GZ = gi_dims(lg)
    m = np.zeros((GZ, GY, GX), bool)
    x0, y0, z0, x1, y1, z1 = box
    m[z0:z1, y0:y1, x0:x1] = True
    return m.ravel()


def _open_centres(bits, lg, box):
    """Box cells whose centre voxel 4c + 2 is not solid: the cells an update traces."""
    x0, y0, z0, x1, y1, z1 = box
    c = voxels(bits, lg)[2::4, 2::4, 2::4]
    return int((~c[z0:z1, y0:y1, x0:x1]).sum())


def expect_relight(ow, box, frame0, steps, init=False, saturate=False, in_place=False):
    """The relight on the oracle world's grid (changed in place; returned as a uint32 copy).  A step
    updates the box one x-row at a time, every row from the step's snapshot of the grid;
    in_place=True lets a row see the rows updated before it in the same step (the wrong answer)."""
    lg = (ow.lx, ow.ly, ow.lz)
    rows, nx = _rows(lg, box)
    g = ow.gi.view(np.uint32)
    if init:
        for first in rows:
            ow.gi_init(first=first, count=nx, saturate=saturate)
    for i in range(steps):
        snap = g.copy()
        new = []
        for first in rows:
            if not in_place:
                g[:] = snap
            ow.gi_update((frame0 + i) & 0xFFFFFFFF, first, nx)
            new.append(g[first:first + nx].copy())
        if not in_place:
            g[:] = snap
            for first, v in zip(rows, new):
                g[first:first + nx] = v
    return g.copy()
