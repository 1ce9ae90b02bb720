"""rv_world_edit_region (host only): the coarse-cell box whose CSDF bytes a voxel
edit's local rebuild recomputes.  It must hold every cell a whole-grid rebuild
would change -- checked against the oracle's build_csdf on long, sparse worlds,
where a flipped voxel's influence reaches its 63-cell limit -- and be no larger
than the edit's coarse extent grown by 64 cells per axis."""
import numpy as np
import pytest

from gpu_world import rv

WORLDS = [(10, 6, 6), (6, 10, 6), (6, 6, 10)]
DENSITIES = [0.0, 1e-6, 1e-4]


def sparse_world(oracle, lg, density, seed):
    w = oracle.OracleWorld(*lg)
    n = w.X * w.Y * w.Z
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, int(round(n * density)), replace=False)
    np.bitwise_or.at(w.bits, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return w, rng


def expected_bounds(lg, lo, hi):
    """E grown by 64 and clipped, for the voxel box [lo, hi)."""
    out = []
    for a in range(3):
        S = 1 << (lg[a] - 1)
        out += [max(0, (lo[a] >> 1) - 64), min(S, ((hi[a] - 1) >> 1) + 1 + 64)]
    return out


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("lg", WORLDS)
def test_region_holds_every_changed_cell(rv, oracle, lg, density):
    w, rng = sparse_world(oracle, lg, density, seed=1234 + sum(lg) * 7 + WORLDS.index(lg))
    w.build_csdf()
    base = w.csdf.copy()
    S = tuple(1 << (l - 1) for l in lg)
    long_axis = int(np.argmax(lg))
    voxels = [(w.X // 2, w.Y // 2, w.Z // 2)]
    voxels += [tuple(int(rng.integers(0, d)) for d in (w.X, w.Y, w.Z)) for _ in range(3)]
    reach = 0
    for (x, y, z) in voxels:
        was = w.solid(x, y, z)
        w.set_solid(x, y, z, not was)
        w.build_csdf()
        ch = np.nonzero((w.csdf != base).reshape(S[2], S[1], S[0]))
        region, cells = rv.edit_region(lg, [(x, y, z, x + 1, y + 1, z + 1, int(not was))])
        assert len(region) == 6
        assert cells == (region[1] - region[0]) * (region[3] - region[2]) * (region[5] - region[4])
        bound = expected_bounds(lg, (x, y, z), (x + 1, y + 1, z + 1))
        for a, c in enumerate((ch[2], ch[1], ch[0])):   # x, y, z coordinates of the changed cells
            lo, hi = region[2 * a], region[2 * a + 1]
            assert 0 <= lo < hi <= S[a]
            assert lo >= bound[2 * a] and hi <= bound[2 * a + 1], (a, region, bound)
            if len(c):
                assert lo <= c.min() and c.max() < hi, (a, (x, y, z), int(c.min()), int(c.max()), region)
                reach = max(reach, int(np.abs(c - ((x, y, z)[a] >> 1)).max()))
        assert region[2 * long_axis + 1] - region[2 * long_axis] < S[long_axis]   # a local region
        w.set_solid(x, y, z, was)
    assert reach <= 63
    if density <= 1e-6:
        assert reach == 63   # the sparse worlds do reach the limit: a smaller region would fail above


@pytest.mark.parametrize("lg", WORLDS + [(7, 7, 7)])
def test_region_clips_at_the_corners(rv, lg):
    X, Y, Z = (1 << l for l in lg)
    S = tuple(1 << (l - 1) for l in lg)
    r0, n0 = rv.edit_region(lg, [(0, 0, 0, 1, 1, 1, 1)])
    assert r0 == (0, min(S[0], 65), 0, min(S[1], 65), 0, min(S[2], 65))
    r1, n1 = rv.edit_region(lg, [(X - 1, Y - 1, Z - 1, X, Y, Z, 0)])
    assert r1 == (max(0, S[0] - 65), S[0], max(0, S[1] - 65), S[1], max(0, S[2] - 65), S[2])
    assert n0 == n1 == min(S[0], 65) * min(S[1], 65) * min(S[2], 65)
    # several boxes: one region around their bounding box; a whole-world box: the whole grid
    r2, n2 = rv.edit_region(lg, [(0, 0, 0, 1, 1, 1, 1), (X - 1, Y - 1, Z - 1, X, Y, Z, 0)])
    assert r2 == (0, S[0], 0, S[1], 0, S[2]) and n2 == S[0] * S[1] * S[2]
    assert rv.edit_region(lg, [(0, 0, 0, X, Y, Z, 0)]) == (r2, n2)
    assert rv.edit_region(lg, []) == ((0,) * 6, 0)


def test_unaligned_box_extent(rv):
    # voxels 5..12 -> coarse cells 2..6, 3..8 -> 1..4, 7..9 -> 3..4; grown by 64, clipped to 512 x 32 x 32
    region, cells = rv.edit_region((10, 6, 6), [(300, 3, 7, 301, 9, 10, 1), (5, 4, 8, 13, 5, 9, 0)])
    assert region == (0, 151 + 64, 0, 32, 0, 32)
    region, cells = rv.edit_region((10, 6, 6), [(301, 3, 7, 303, 9, 10, 1)])
    assert region == (150 - 64, 152 + 64, 0, 32, 0, 32) and cells == 130 * 32 * 32


def test_invalid_boxes_rejected(rv):
    lg = (7, 6, 8)
    X, Y, Z = 128, 64, 256
    bad = [(4, 4, 4, 4, 5, 5, 1), (4, 4, 4, 5, 4, 5, 1), (4, 4, 4, 5, 5, 3, 1),      # empty / reversed
           (-1, 0, 0, 1, 1, 1, 1), (0, -1, 0, 1, 1, 1, 0), (0, 0, -1, 1, 1, 1, 0),   # below the world
           (0, 0, 0, X + 1, 1, 1, 1), (0, 0, 0, 1, Y + 1, 1, 1), (0, 0, 0, 1, 1, Z + 1, 1),
           (0, 0, 0, 1, 1, 1, 2), (0, 0, 0, 1, 1, 1, -1)]                              # solid not 0 / 1
    good = (0, 0, 0, X, Y, Z, 1)
    rv.edit_region(lg, [good])
    for b in bad:
        with pytest.raises(rv.RvError):
            rv.edit_region(lg, [b])
        with pytest.raises(rv.RvError):
            rv.edit_region(lg, [good, b])   # every box is validated
    with pytest.raises(rv.RvError):
        rv.edit_region(lg, [good] * (rv._lib.RV_EDIT_MAX_BOXES + 1))
    rv.edit_region(lg, [good] * rv._lib.RV_EDIT_MAX_BOXES)
    with pytest.raises(rv.RvError):
        rv.edit_region((3, 6, 6), [(0, 0, 0, 1, 1, 1, 1)])
    L = rv._lib.load()
    assert L.rv_world_edit_region(6, 6, 6, None, 1, None, None) == rv._lib.RV_ERR_INVALID
    assert L.rv_world_edit(None, None, 0) == rv._lib.RV_ERR_INVALID
    assert L.rv_world_edit_info(None, None, None, None) == rv._lib.RV_ERR_INVALID
