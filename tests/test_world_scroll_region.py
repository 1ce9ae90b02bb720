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

from gpu_world import rv, sparse_bits
from np_world import SPARSE_SEEDS, expected_plan, reaches, scrolled

WORLDS = [(9, 7, 7), (7, 7, 9), (10, 6, 6), (7, 7, 7)]


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
@pytest.mark.parametrize("density", [0.0, 1e-6, 1e-4])
@pytest.mark.parametrize("d", [8, -8, 40, 64, -64])
@pytest.mark.parametrize("lg,axis", [((10, 6, 6), 0), ((6, 6, 10), 2)])
def test_slabs_hold_every_changed_cell(rv, oracle, lg, axis, d, density):
    S = tuple(1 << (l - 1) for l in lg)
    seed = SPARSE_SEEDS[(lg, axis, d)] if density == 1e-6 else 99 + axis + abs(d)
    bits, old, new = scrolled(oracle, lg, axis, d, sparse_bits(lg, density, seed))
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
