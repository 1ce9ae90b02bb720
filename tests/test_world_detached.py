"""rv_world_detached on the CPU: rv_world_detached_at -- the functions the kernels call, evaluated word after
word on the host over RV_WORLD_BITS words -- against the numpy restatement of the definition
(tests/np_detached.py), exactly: the mask words, n_voxels, n_comps and every field of every component in order."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import generated, pack, rv, synthetic_voxels, voxels
import np_detached as D


def lg_of(vox):
    return tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])


def same(got, want, what):
    """got: the library's (components, n_comps, n_voxels, mask); want: the restatement's."""
    comps, n, v, mask = got
    assert n == len(want[0]) and v == want[1], (what, n, len(want[0]), v, want[1])
    assert np.array_equal(mask, want[2]), (what, "mask")
    assert len(comps) == n
    for f in ("seed", "lo", "hi", "voxels"):
        assert np.array_equal(comps[f], want[0][f]), (what, f)


def check(rv, vox, box, what):
    want = D.detached(vox, box)
    same(rv.detached_at(lg_of(vox), pack(vox), box), want, what)
    return want


# ---------------------------------------------------------------- random worlds
BOXES32 = [(0, 0, 0, 32, 32, 32), (3, 5, 1, 29, 23, 31)]


def random32(d, s):
    return np.random.default_rng(s).random((32, 32, 32)) < d


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("d", [0.1, 0.3, 0.6])
def test_random_worlds(rv, d, s):
    vox = random32(d, s)
    for box in BOXES32:
        comps, nv, _, det = check(rv, vox, box, (d, s, box))
        if box == BOXES32[0]:
            sizes = comps["voxels"]
            if d == 0.3:   # the input is not degenerate
                assert len(comps) >= 500 and (sizes > 1).sum() >= 100 and sizes.max() >= 100
                assert nv >= 1000 and vox.sum() - nv >= 1000
            if d == 0.6:   # single voxels enclosed by nothing
                assert len(comps) >= 10


# ---------------------------------------------------------------- the outside rule, face by face
def island(at):
    vox = np.zeros((32, 32, 32), bool)
    x, y, z = at
    vox[z:z + 3, y:y + 3, x:x + 3] = True
    return vox


@pytest.mark.parametrize("axis,side", [(a, s) for a in range(3) for s in (0, 1)])
def test_anchor_by_a_voxel_outside(rv, axis, side):
    box = (8, 8, 8, 20, 20, 20)
    at = [12, 12, 12]
    at[axis] = 17 if side else 8
    out = [13, 13, 13]
    out[axis] = 20 if side else 7
    vox = island(at)
    comps, nv, _, _ = check(rv, vox, box, "floating")
    assert nv == 27 and len(comps) == 1 and comps[0]["seed"].tolist() == at
    vox[out[2], out[1], out[0]] = True
    assert check(rv, vox, box, "held")[1] == 0


def test_anchor_by_floor_walls_and_not_by_the_sky(rv):
    # touching y0 = 0: the floor holds it; touching y1 = Y: nothing above does
    assert check(rv, island((12, 0, 12)), (8, 0, 8, 20, 12, 20), "floor")[1] == 0
    assert check(rv, island((12, 29, 12)), (8, 20, 8, 20, 32, 20), "sky")[1] == 27
    # the window's walls
    assert check(rv, island((0, 12, 12)), (0, 8, 8, 12, 20, 20), "x0")[1] == 0
    assert check(rv, island((29, 12, 12)), (20, 8, 8, 32, 20, 20), "x1")[1] == 0
    assert check(rv, island((12, 12, 0)), (8, 8, 0, 20, 20, 12), "z0")[1] == 0
    assert check(rv, island((12, 12, 29)), (8, 8, 20, 20, 20, 32), "z1")[1] == 0
    # one voxel away from a wall nothing holds it
    assert check(rv, island((1, 12, 12)), (0, 8, 8, 12, 20, 20), "x0 + 1")[1] == 27


# ---------------------------------------------------------------- a long path
def test_long_path(rv):
    vox, cells, box, contact = D.long_path()
    assert len(cells) >= 4000 and vox.sum() == len(cells)
    comps, nv, _, _ = check(rv, vox, box, "path, loose")
    assert nv == len(cells) and len(comps) == 1 and comps[0]["voxels"] == len(cells)
    vox[contact[2], contact[1], contact[0]] = True
    assert check(rv, vox, box, "path, held at its end")[1] == 0


# ---------------------------------------------------------------- word boundaries and small boxes
def test_bars_across_word_boundaries(rv):
    vox, box = D.bars(False)
    comps, nv, _, _ = check(rv, vox, box, "bars, floating")
    assert len(comps) == 6 and (comps["voxels"] == 2).all() and nv == 12
    vox, box = D.bars(True)
    assert check(rv, vox, box, "bars, held")[1] == 0 and vox.sum() > 12


def test_single_voxel_boxes(rv):
    vox = np.zeros((32, 32, 32), bool)
    box = (10, 10, 10, 11, 11, 11)
    assert check(rv, vox, box, "empty")[1] == 0
    vox[10, 10, 10] = True
    assert check(rv, vox, box, "alone")[1] == 1
    vox[10, 10, 11] = True
    assert check(rv, vox, box, "held")[1] == 0


@pytest.mark.parametrize("box", [(7, 0, 0, 8, 32, 32), (0, 9, 0, 32, 10, 32), (0, 0, 11, 32, 32, 12),
                                 (31, 3, 2, 32, 30, 31), (2, 31, 3, 31, 32, 30)])
def test_boxes_one_voxel_thick(rv, box):
    want = check(rv, random32(0.3, 1), box, box)
    if box[0] in (7, 2):
        assert want[1] > 0


# ---------------------------------------------------------------- other worlds and arguments
@pytest.mark.parametrize("kind", ["pillars", "blocks"])
def test_synthetic(rv, kind):
    vox = synthetic_voxels(kind, 32, 32, 64, np.random.default_rng(3))
    check(rv, vox, (0, 0, 0, 32, 32, 64), kind)
    # above the floor: whatever does not reach the box's lower face or the walls hangs
    want = check(rv, vox, (2, 9, 3, 30, 32, 61), (kind, "upper part"))
    if kind == "blocks":
        assert want[1] > 0


def terrain_scene(oracle):
    """The oracle's 128^3 terrain with a 5 x 2 x 5 slab floating over it and a pillar cut by a one-voxel gap,
    both inside the box [32, 96)^3."""
    lg = (7, 7, 7)
    vox = voxels(generated(oracle, lg, (0, 0)), lg).copy()
    top = lambda x, z: int(vox[z, :, x].nonzero()[0].max()) + 1   # noqa: E731
    h = max(32, max(top(x, z) for x in range(60, 65) for z in range(60, 65)))   # the ground may lie below the box
    assert h + 6 < 96, h
    vox[60:65, h + 3:h + 5, 60:65] = True
    g0 = top(72, 72)
    g = max(32, g0)
    assert g + 10 < 96, g
    vox[72, g0:g + 9, 72] = True
    vox[72, g + 4, 72] = False
    return vox, (32, 32, 32, 96, 96, 96), (h, g)


def test_terrain_slab_and_cut_pillar(rv, oracle):
    vox, box, (h, g) = terrain_scene(oracle)
    comps, nv, _, _ = check(rv, vox, box, "terrain")
    found = {(tuple(c["lo"]), tuple(c["hi"]), int(c["voxels"])) for c in comps}
    assert ((60, h + 3, 60), (65, h + 5, 65), 50) in found
    assert ((72, g + 5, 72), (73, g + 9, 73), 4) in found


def test_checkerboard_and_cap(rv):
    board = D.checkerboard()
    box = (1, 1, 1, 31, 31, 31)
    comps, nv, _, _ = check(rv, board, box, "checkerboard, interior box")
    assert nv == 30 ** 3 // 2 == len(comps) and (comps["voxels"] == 1).all()
    # the whole board inside a larger world: 16384 one-voxel components
    vox = np.zeros((64, 64, 64), bool)
    vox[16:48, 16:48, 16:48] = board
    box = (16, 16, 16, 48, 48, 48)
    want = check(rv, vox, box, "checkerboard, whole")
    assert want[1] == 16384 == len(want[0])
    got = rv.detached_at((6, 6, 6), pack(vox), box, cap=10)
    assert got[1] == 16384 and got[2] == 16384 and len(got[0]) == 10
    for f in ("seed", "lo", "hi", "voxels"):
        assert np.array_equal(got[0][f], want[0][f][:10]), f


def test_optional_outputs(rv):
    vox = random32(0.3, 2)
    want = D.detached(vox, BOXES32[1])
    got = rv.detached_at((5, 5, 5), pack(vox), BOXES32[1], want_mask=False)
    assert got[3] is None and got[1] == len(want[0]) and got[2] == want[1]
    assert np.array_equal(got[0]["seed"], want[0]["seed"])
    got = rv.detached_at((5, 5, 5), pack(vox), BOXES32[1], cap=0)
    assert len(got[0]) == 0 and got[1] == len(want[0]) and np.array_equal(got[3], want[2])
    # every out pointer NULL
    L = rv._lib.load()
    bits = pack(vox)
    b = rv._lib.rv_voxel_box(*BOXES32[1])
    assert L.rv_world_detached_at(5, 5, 5, bits.ctypes.data_as(C.c_void_p), C.byref(b), None, 0, None, None, None, 0) == 0


def test_struct_sizes(rv):
    assert C.sizeof(rv._lib.rv_component) == 40 and C.sizeof(rv._lib.rv_voxel_box) == 24
    assert rv.COMPONENT_DTYPE.itemsize == 40 and D.COMPONENT.itemsize == 40
    assert rv._lib.RV_DETACHED_MAX_VOXELS == 128 ** 3


def test_status_codes(rv):
    L, lib = rv._lib.load(), rv._lib
    bits = pack(random32(0.3, 1))
    big = np.zeros(256 ** 3 // 32, np.uint32)
    comps = np.zeros(8, rv.COMPONENT_DTYPE)
    mask = np.zeros(1024, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, v = C.c_int64(), C.c_uint64()

    def at(lg=(5, 5, 5), bits_=bits, box=(0, 0, 0, 32, 32, 32), comps_=comps, cap=8, mask_=mask, nbytes=4096):
        b = None if box is None else C.byref(lib.rv_voxel_box(*box))
        return L.rv_world_detached_at(*lg, None if bits_ is None else p(bits_), b, None if comps_ is None else p(comps_),
                                      cap, C.byref(n), C.byref(v), None if mask_ is None else p(mask_), nbytes)
    assert at() == lib.RV_OK
    assert at(mask_=None, nbytes=0) == lib.RV_OK and at(comps_=None, cap=0) == lib.RV_OK
    bad = [dict(box=None), dict(box=(4, 4, 4, 4, 8, 8)), dict(box=(4, 8, 4, 8, 8, 8)), dict(box=(4, 4, 9, 8, 8, 8)),
           dict(box=(-1, 0, 0, 8, 8, 8)), dict(box=(0, 0, 0, 33, 8, 8)), dict(box=(0, 0, 0, 8, 33, 8)),
           dict(box=(0, 0, -2, 8, 8, 8)), dict(cap=-1), dict(comps_=None, cap=1), dict(nbytes=4092),
           dict(bits_=None), dict(lg=(4, 5, 5)), dict(lg=(5, 3, 5)), dict(lg=(5, 5, 14)),
           dict(lg=(8, 8, 8), bits_=big, box=(0, 0, 0, 129, 128, 128), mask_=None, nbytes=0)]   # V above the cap
    for kw in bad:
        assert at(**kw) == lib.RV_ERR_INVALID, kw
    assert at(lg=(8, 8, 8), bits_=big, box=(0, 0, 0, 128, 128, 128), mask_=None, nbytes=0) == lib.RV_OK   # V at the cap
    # the entry points that take a context: a NULL context
    b = C.byref(lib.rv_voxel_box(0, 0, 0, 8, 8, 8))
    assert L.rv_world_detached(None, b, 0, None, 0, None, None, None, 0) == lib.RV_ERR_INVALID
    assert L.rv_world_detached_info(None, None, None, None) == lib.RV_ERR_INVALID
