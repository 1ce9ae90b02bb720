"""rv_world_scroll_region (host only): the two slabs of coarse cells whose CSDF
bytes a one-axis scroll's local rebuild recomputes, and the switch to the
whole-grid build.  The planner is checked against a numpy restatement; the
bound itself against the oracle: on long worlds the window is moved on the
host (numpy shift of the old bits, the entering slab from the oracle's fill at
the new origin), the CSDF rebuilt whole, and every byte that differs from the
shifted old CSDF must lie inside the two boxes -- with sparse worlds in which
the difference does reach 48 cells and more into either slab, so that a smaller
region would fail."""
import numpy as np
import pytest

WORLDS = [(9, 7, 7), (7, 7, 9), (10, 6, 6), (7, 7, 7)]


@pytest.fixture(scope="module")
def rv():
    import rvgrt_amd
    rvgrt_amd._lib.load()
    return rvgrt_amd


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


@pytest.mark.parametrize("lg", WORLDS)
def test_planner_matches_restatement(rv, lg):
    for axis in (0, 2):
        dim = 1 << lg[axis]
        for mag in (8, 64, 128, 256, dim, dim + 8, 4 * dim):
            for d in (mag, -mag):
                got = rv.scroll_region(lg, axis, d)
                assert got == expected_plan(lg, axis, d), (lg, axis, d)
                if abs(d) >= dim:
                    assert got[3] is True
        assert rv.scroll_region(lg, axis, 0) == ((0,) * 6, (0,) * 6, 0, False)


def test_full_crossover(rv):
    # a 512-voxel axis (256 cells): (640 + 4k) < 1024 up to k = 95; at equality the whole-grid build
    for lg, axis in (((9, 7, 7), 0), ((7, 7, 9), 2)):
        for sign in (1, -1):
            assert [rv.scroll_region(lg, axis, sign * d)[3] for d in (8, 64, 128, 184, 192, 256)] == \
                [False, False, False, False, True, True]
            tr, ld, cells, full = rv.scroll_region(lg, axis, sign * 184)
            assert ld[2 * axis + 1] - ld[2 * axis] == 92 + 64 and tr[2 * axis + 1] - tr[2 * axis] == 64
            assert cells == (92 + 128) * 64 * 64
    # 1024 voxels: 32 % of the whole build's cell passes at d = 8; whole from k = 352
    assert [rv.scroll_region((10, 6, 6), 0, d)[3] for d in (8, 256, 696, 704)] == [False, False, False, True]
    assert (640 + 4 * 4) / (4 * 512) == pytest.approx(0.32, abs=0.005)
    # 128 and 256 voxels: always the whole grid
    for lx in (7, 8):
        assert all(rv.scroll_region((lx, 6, 6), 0, d)[3] for d in (8, -8, 64, 128))
    # a step never splits: the x boxes span all of y and z, whatever those are
    tr, ld, cells, full = rv.scroll_region((10, 4, 13), 0, -8)
    assert tr == (512 - 64, 512, 0, 8, 0, 4096) and ld == (0, 68, 0, 8, 0, 4096) and not full


def test_invalid_arguments(rv):
    L = rv._lib.load()
    import ctypes as C
    reg = (C.c_int32 * 12)()
    INV = rv._lib.RV_ERR_INVALID
    assert L.rv_world_scroll_region(9, 7, 7, 0, 8, reg, None, None) == 0        # cells / full may be NULL
    assert L.rv_world_scroll_region(9, 7, 7, 0, 8, None, None, None) == INV
    assert L.rv_world_scroll_region(9, 7, 7, 1, 8, reg, None, None) == INV      # no y scroll
    assert L.rv_world_scroll_region(9, 7, 7, 3, 8, reg, None, None) == INV
    assert L.rv_world_scroll_region(9, 7, 7, 0, 4, reg, None, None) == INV      # whole bricks only
    assert L.rv_world_scroll_region(9, 7, 7, 2, -12, reg, None, None) == INV
    assert L.rv_world_scroll_region(3, 7, 7, 0, 8, reg, None, None) == INV
    assert L.rv_world_scroll(None, 8, 0) == INV
    assert L.rv_world_scroll_info(None, None, None, None, None, None) == INV


# ---------------------------------------------------------------- the bound, against the oracle
ORIGIN = (40, -24)   # the old window's origin on the terrain
# Seeds of the density-1e-6 worlds (4 solid voxels) in which the oracle alone shows a byte that differs
# >= 48 cells from the trailing face: one of the voxels leaves with the old planes and was the nearest
# solid of cells that far into the retained part.  (The entering terrain reaches as far by itself.)
SPARSE_SEEDS = {
    ((10, 6, 6), 0, 8): 1119, ((10, 6, 6), 0, -8): 1036, ((10, 6, 6), 0, 64): 1005, ((10, 6, 6), 0, -64): 1049,
    ((6, 6, 10), 2, 8): 1036, ((6, 6, 10), 2, -8): 1074, ((6, 6, 10), 2, 64): 1009, ((6, 6, 10), 2, -64): 1037,
    ((10, 6, 6), 0, 40): 1060, ((6, 6, 10), 2, 40): 1027,
}


def sparse_bits(n, density, seed):
    bits = np.zeros(n // 32, np.uint32)
    idx = np.random.default_rng(seed).choice(n, int(round(n * density)), replace=False)
    np.bitwise_or.at(bits, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return bits


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
    nw.bits[:] = np.packbits(vox.ravel(), bitorder="little").view(np.uint32)
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


@pytest.mark.parametrize("density", [0.0, 1e-6, 1e-4])
@pytest.mark.parametrize("d", [8, -8, 40, 64, -64])
@pytest.mark.parametrize("lg,axis", [((10, 6, 6), 0), ((6, 6, 10), 2)])
def test_slabs_hold_every_changed_cell(rv, oracle, lg, axis, d, density):
    S = tuple(1 << (l - 1) for l in lg)
    seed = SPARSE_SEEDS[(lg, axis, d)] if density == 1e-6 else 99 + axis + abs(d)
    bits, old, new = scrolled(oracle, lg, axis, d, sparse_bits(1 << sum(lg), density, seed))
    tr, ld, cells, full = rv.scroll_region(lg, axis, d)
    assert not full
    inside = np.zeros(new.shape, bool)
    for b in (tr, ld):
        inside[b[4]:b[5], b[2]:b[3], b[0]:b[1]] = True
    assert cells == int(inside.sum())
    diff = new != old
    assert diff.any() and not (diff & ~inside).any(), (lg, axis, d, density)
    t_reach, l_reach = reaches(axis, d, S, diff)
    print(f"{lg} axis {axis} d {d} density {density}: trailing reach {t_reach}, leading reach {l_reach}")
    assert t_reach <= 63 and l_reach <= 63
    if density <= 1e-6:
        assert l_reach >= 48   # the entering terrain, seen from the empty cells before it
    if density == 1e-6:
        assert t_reach >= 48   # a voxel that left: a smaller trailing slab would miss these cells
