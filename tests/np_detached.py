"""rv_world_detached restated from its definition (include/rvgrt.h) over a dense [z, y, x] boolean array:
anchors from the outside rule cell by cell, attachment by 6-neighbour dilation until nothing changes,
components by min-index propagation until nothing changes.  Plain and slow on purpose; it shares neither
code nor algorithm with the library (no bit words, no union-find)."""
import numpy as np

COMPONENT = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("seed", np.int32, 3), ("voxels", np.uint32)])


def outside_solid(vox, i, j, k):
    """The outside rule for cell (i, j, k)."""
    Z, Y, X = vox.shape
    if j >= Y:
        return False
    if j < 0:
        return True
    if i < 0 or i >= X or k < 0 or k >= Z:
        return True
    return bool(vox[k, j, i])


def _neighbours(a, fill):
    """The six shifted copies of a, `fill` where a neighbour lies outside the array."""
    out = []
    for axis in range(3):
        for d in (1, -1):
            s = np.full_like(a, fill)
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(0, -1) if d == 1 else slice(1, None)
            dst[axis] = slice(1, None) if d == 1 else slice(0, -1)
            s[tuple(dst)] = a[tuple(src)]
            out.append(s)
    return out


def anchored(vox, box):
    """[nz, ny, nx]: the solid voxels of the box with a solid neighbour outside it."""
    x0, y0, z0, x1, y1, z1 = box
    sub = vox[z0:z1, y0:y1, x0:x1]
    a = np.zeros(sub.shape, bool)
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                if not (x in (x0, x1 - 1) or y in (y0, y1 - 1) or z in (z0, z1 - 1)) or not vox[z, y, x]:
                    continue
                for (i, j, k) in ((x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1), (x, y, z + 1)):
                    inside = x0 <= i < x1 and y0 <= j < y1 and z0 <= k < z1
                    if not inside and outside_solid(vox, i, j, k):
                        a[z - z0, y - y0, x - x0] = True
    return a


def attached(vox, box):
    x0, y0, z0, x1, y1, z1 = box
    sub = vox[z0:z1, y0:y1, x0:x1]
    att = anchored(vox, box)
    while True:
        grow = att.copy()
        for s in _neighbours(att, False):
            grow |= s
        grow &= sub
        if np.array_equal(grow, att):
            return att
        att = grow


def detached(vox, box):
    """(components as COMPONENT records in ascending seed order, detached voxels, mask words, the dense
    [nz, ny, nx] detached array)."""
    x0, y0, z0, x1, y1, z1 = box
    sub = vox[z0:z1, y0:y1, x0:x1]
    nz, ny, nx = sub.shape
    V = nx * ny * nz
    det = sub & ~attached(vox, box)
    big = np.int64(V)
    lab = np.where(det, np.arange(V, dtype=np.int64).reshape(nz, ny, nx), big)
    while True:
        new = lab.copy()
        for s in _neighbours(lab, big):
            new = np.minimum(new, s)
        new = np.where(det, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    zs, ys, xs = np.nonzero(det)
    labels = lab[zs, ys, xs]
    order = np.argsort(labels, kind="stable")
    seeds, first, counts = np.unique(labels[order], return_index=True, return_counts=True)
    comps = np.zeros(len(seeds), COMPONENT)
    for c, (seed, f, n) in enumerate(zip(seeds, first, counts)):
        m = order[f:f + n]
        comps[c]["lo"] = (x0 + xs[m].min(), y0 + ys[m].min(), z0 + zs[m].min())
        comps[c]["hi"] = (x0 + xs[m].max() + 1, y0 + ys[m].max() + 1, z0 + zs[m].max() + 1)
        comps[c]["seed"] = (x0 + seed % nx, y0 + seed // nx % ny, z0 + seed // (nx * ny))
        comps[c]["voxels"] = n
    flat = np.zeros((V + 31) // 32 * 32, bool)
    flat[:V] = det.ravel()
    mask = np.packbits(flat, bitorder="little").view(np.uint32)
    return comps, int(det.sum()), mask, det


def cleared(vox, box):
    """The world after the detached voxels of the box have been cleared."""
    x0, y0, z0, x1, y1, z1 = box
    out = vox.copy()
    out[z0:z1, y0:y1, x0:x1] &= ~detached(vox, box)[3]
    return out


# ---------------------------------------------------------------- scenes the CPU and the GPU tests share
def long_path(n=32):
    """A one-voxel-thick boustrophedon path in an n^3 world: rows along x joined alternately at their ends in
    z, layers joined alternately in y.  Returns (vox, cells in path order, box, the one cell outside the box
    that touches the path: above its last voxel)."""
    vox = np.zeros((n, n, n), bool)
    layer = []
    for r, z in enumerate(range(1, n - 1, 2)):
        xs = list(range(1, n - 1))
        row = [(x, z) for x in (xs if r % 2 == 0 else xs[::-1])]
        if layer:
            layer.append((layer[-1][0], z - 1))
        layer += row
    cells = []
    ys = list(range(2, 20, 2))
    for k, y in enumerate(ys):
        order = layer if k % 2 == 0 else layer[::-1]
        if cells:
            cells.append((cells[-1][0], y - 1, cells[-1][2]))
        cells += [(x, y, z) for (x, z) in order]
    for (x, y, z) in cells:
        vox[z, y, x] = True
    last = cells[-1]
    box = (1, 2, 1, n - 1, ys[-1] + 1, n - 1)
    return vox, cells, box, (last[0], last[1] + 1, last[2])


def bars(anchor):
    """A 64 x 32 x 32 world with six 2-voxel bars that straddle a brick, a world word, a box-local word (the
    box starts at x = 5) along x, a brick word and a brick along y, a brick along z; with `anchor` a pillar
    joins each bar to row 0.  Returns (vox, box)."""
    vox = np.zeros((32, 32, 64), bool)
    ends = [((7, 10, 4), (8, 10, 4)), ((31, 10, 8), (32, 10, 8)), ((36, 10, 12), (37, 10, 12)),
            ((20, 3, 16), (20, 4, 16)), ((24, 7, 20), (24, 8, 20)), ((12, 10, 7), (12, 10, 8))]
    for a, b in ends:
        for (x, y, z) in (a, b):
            vox[z, y, x] = True
        if anchor:
            vox[a[2], :a[1], a[0]] = True
    return vox, (5, 0, 1, 45, 31, 31)


def checkerboard(n=32):
    z, y, x = np.indices((n, n, n))
    return ((x + y + z) & 1).astype(bool)
