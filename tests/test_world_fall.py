"""rv_world_fall on the CPU: rv_world_fall_at -- the query and the clearance scan the kernels run, evaluated word
after word on the host over RV_WORLD_BITS words -- against the numpy restatement of the definition
(tests/np_fall.py), exactly: every field of every rv_fallen in order, both totals, the changed box and every
word of the world after the move."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import pack, rv
import np_detached as D
import np_fall as F
from test_world_detached import BOXES32, random32


def lg_of(vox):
    return tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])


def same(got, want, what):
    """got: the library's (components, n_comps, n_voxels, changed[, ...]); want: np_fall.fall's."""
    comps, n, v, changed = got[:4]
    assert n == len(want[0]) and v == want[1], (what, n, len(want[0]), v, want[1])
    assert tuple(changed) == tuple(want[2]), (what, changed, want[2])
    assert len(comps) == n
    for f in ("seed", "lo", "hi", "voxels"):
        assert np.array_equal(comps["comp"][f], want[0]["comp"][f]), (what, f)
    for f in ("fall", "flags"):
        assert np.array_equal(comps[f], want[0][f]), (what, f, comps[f], want[0][f])


def check(rv, vox, box, max_fall=0, what=None, parts=None):
    want = F.fall(vox, box, max_fall, parts)
    got = rv.fall_at(lg_of(vox), pack(vox), box, max_fall)
    same(got, want, (what, box, max_fall))
    assert np.array_equal(got[4], pack(want[3])), (what, box, max_fall, "bits")
    return want


# ---------------------------------------------------------------- random worlds
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("d", [0.1, 0.3, 0.6])
def test_random_worlds(rv, d, s):
    vox = random32(d, s)
    for box in BOXES32:
        parts = F.measured(vox, box)
        if d == 0.3 and box == BOXES32[0]:   # the input is not degenerate (seed 1: 1511 components, clearances 1..21)
            clear = parts[2]
            assert len(clear) >= 1000 and clear.min() == 1 and clear.max() >= 10 and (clear > 3).sum() >= 100
            assert (parts[0]["voxels"] > 1).sum() >= 100
        for max_fall in (0, 1, 3):
            want = check(rv, vox, box, max_fall, (d, s), parts)
            if max_fall:
                assert want[0]["fall"].max(initial=0) <= max_fall
                assert np.array_equal(want[0]["flags"] == F.STOPPED, parts[2] <= max_fall)


# ---------------------------------------------------------------- an island leaves the box
@pytest.mark.parametrize("fall", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("slab", [True, False])
def test_island(rv, fall, slab):
    # over a slab the block at y drops `fall` rows onto it; over nothing it drops y rows onto the floor
    y = 15 if slab else fall
    vox = F.island(y, y - fall if slab else None)
    box = (8, y, 8, 20, y + 6, 20)   # y0 above every landing row: the block leaves the box
    want = check(rv, vox, box, 0, ("island", fall, slab))
    assert len(want[0]) == 1 and want[0][0]["fall"] == fall and want[0][0]["flags"] == F.STOPPED
    assert want[0][0]["comp"]["lo"].tolist() == [12, y, 12]
    assert want[2] == (12, y - fall, 12, 15, y + 3, 15)
    assert want[3][12:15, y - fall:y - fall + 3, 12:15].all() and want[3].sum() == vox.sum()


# ---------------------------------------------------------------- rounds
def test_stack(rv):
    vox, box = F.stack()
    one = check(rv, vox, box, 0, "stack, first")
    assert one[0]["fall"].tolist() == [4, 3] and one[0]["flags"].tolist() == [1, 1]
    two = check(rv, one[3], one[2], 0, "stack, second")
    assert two[0]["fall"].tolist() == [4] and two[0][0]["comp"]["lo"].tolist() == [12, 11, 12]
    three = check(rv, two[3], two[2], 0, "stack, third")
    assert len(three[0]) == 0 and three[2] == (0, 0, 0, 0, 0, 0) and np.array_equal(three[3], two[3])
    assert two[3][13, :10, 13].all() and not two[3][13, 10:, 13].any()


def test_u(rv):
    vox, box = F.u_scene()
    one = check(rv, vox, box, 0, "U, first")
    assert one[0]["fall"].tolist() == [2, 8] and one[0]["comp"]["voxels"].tolist() == [27, 6]
    two = check(rv, one[3], one[2], 0, "U, second")
    assert two[0]["fall"].tolist() == [2] and two[0]["comp"]["voxels"].tolist() == [27]
    three = check(rv, two[3], two[2], 0, "U, third")
    assert len(three[0]) == 0


def test_c_shape(rv):
    vox, box = F.c_shape()
    want = check(rv, vox, box, 0, "C")
    assert len(want[0]) == 1 and want[0][0]["fall"] == 5 and want[0][0]["comp"]["voxels"] == 12 + 3 + 5
    # with the step taken away the ground under the lower arm decides, never the own arm
    vox[12, 4:15, 16:20] = False
    assert check(rv, vox, box, 0, "C, no step")[0][0]["fall"] == 13


def test_max_fall_on_the_stack(rv):
    vox, box = F.stack()
    for max_fall, falls, flags in [(1, [1, 1], [0, 0]), (3, [3, 3], [0, 1]), (4, [4, 3], [1, 1]), (32, [4, 3], [1, 1])]:
        want = check(rv, vox, box, max_fall, "stack")
        assert want[0]["fall"].tolist() == falls and want[0]["flags"].tolist() == flags, max_fall
    # one row per call reaches the world of the unlimited calls
    final = F.settle(vox, box)[2]
    calls = 0
    while True:
        want = check(rv, vox, box, 1, ("stack, step", calls))
        if len(want[0]) == 0:
            break
        vox, calls = want[3], calls + 1
        assert calls <= 16
    assert calls == 7 and np.array_equal(vox, final)


# ---------------------------------------------------------------- word, brick and dword boundaries
def test_bars_across_word_boundaries(rv):
    vox, box = D.bars(False)
    want = check(rv, vox, box, 0, "bars")
    assert len(want[0]) == 6 and (want[0]["flags"] == 1).all()
    assert sorted(want[0]["fall"].tolist()) == [3, 7, 10, 10, 10, 10]
    check(rv, vox, box, 2, "bars, limited")


def test_checkerboard_rows(rv):
    vox, box = F.checker_rows()
    want = check(rv, vox, box, 0, "checkerboard")
    y = want[0]["comp"]["lo"][:, 1]
    assert len(want[0]) == 2250 and (want[0]["comp"]["voxels"] == 1).all() and (y == 8).sum() == 450
    # rows 8 and 9 have nothing under them down to the floor (the cell right under a voxel is empty on the
    # board); a voxel of the rows above has the board's voxel two rows down, which moves separately
    assert np.array_equal(want[0]["fall"], np.where(y <= 9, y, 1)) and (want[0]["flags"] == 1).all()


# ---------------------------------------------------------------- arguments
def test_cap_null_pointers_and_in_place(rv):
    vox = random32(0.3, 2)
    box = BOXES32[1]
    want = F.fall(vox, box)
    got = rv.fall_at((5, 5, 5), pack(vox), box, cap=10, want_bits=False)
    assert got[1] == len(want[0]) > 10 and got[2] == want[1] and len(got[0]) == 10 and got[4] is None
    assert got[0].tobytes() == rv.fall_at((5, 5, 5), pack(vox), box)[0][:10].tobytes()
    got = rv.fall_at((5, 5, 5), pack(vox), box, cap=0)
    assert len(got[0]) == 0 and got[1] == len(want[0]) and np.array_equal(got[4], pack(want[3]))
    # bits_out == bits
    bits = pack(vox).copy()
    got = rv.fall_at((5, 5, 5), bits, box, in_place=True)
    same(got, want, "in place")
    assert got[4] is bits and np.array_equal(bits, pack(want[3]))
    # every out pointer NULL
    L = rv._lib.load()
    bits = pack(vox)
    b = rv._lib.rv_voxel_box(*box)
    assert L.rv_world_fall_at(5, 5, 5, bits.ctypes.data_as(C.c_void_p), C.byref(b), 0, None, 0, None, None, None, None,
                              0) == 0
    assert np.array_equal(bits, pack(vox))


def test_struct_sizes(rv):
    assert C.sizeof(rv._lib.rv_fallen) == 48 and rv.FALLEN_DTYPE.itemsize == 48 and F.FALLEN.itemsize == 48
    assert rv.RV_FALL_STOPPED == 1 == F.STOPPED


def test_status_codes(rv):
    L, lib = rv._lib.load(), rv._lib
    bits = pack(random32(0.3, 1))
    comps = np.zeros(8, rv.FALLEN_DTYPE)
    out = np.zeros(1024, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, v, ch = C.c_int64(), C.c_uint64(), lib.rv_voxel_box()

    def at(lg=(5, 5, 5), bits_=bits, box=(0, 0, 0, 32, 32, 32), max_fall=0, comps_=comps, cap=8, out_=out, nbytes=4096):
        b = None if box is None else C.byref(lib.rv_voxel_box(*box))
        return L.rv_world_fall_at(*lg, None if bits_ is None else p(bits_), b, max_fall,
                                  None if comps_ is None else p(comps_), cap, C.byref(n), C.byref(v), C.byref(ch),
                                  None if out_ is None else p(out_), nbytes)
    assert at() == lib.RV_OK and at(max_fall=32) == lib.RV_OK
    assert at(out_=None, nbytes=0) == lib.RV_OK and at(comps_=None, cap=0) == lib.RV_OK
    bad = [dict(box=None), dict(box=(4, 4, 4, 4, 8, 8)), dict(box=(4, 8, 4, 8, 8, 8)), dict(box=(4, 4, 9, 8, 8, 8)),
           dict(box=(-1, 0, 0, 8, 8, 8)), dict(box=(0, 0, 0, 33, 8, 8)), dict(box=(0, 0, 0, 8, 33, 8)),
           dict(box=(0, 0, -2, 8, 8, 8)), dict(cap=-1), dict(comps_=None, cap=1), dict(nbytes=4092),
           dict(max_fall=-1), dict(max_fall=33), dict(bits_=None), dict(lg=(4, 5, 5)), dict(lg=(5, 3, 5)),
           dict(lg=(5, 5, 14))]
    keep = out.copy()
    for kw in bad:
        assert at(**kw) == lib.RV_ERR_INVALID, kw
    assert np.array_equal(out, keep)
    # the entry points that take a context: a NULL context
    b = C.byref(lib.rv_voxel_box(0, 0, 0, 8, 8, 8))
    assert L.rv_world_fall(None, b, 0, None, 0, None, None, None) == lib.RV_ERR_INVALID
    assert L.rv_world_fall_info(None, None, None, None) == lib.RV_ERR_INVALID
