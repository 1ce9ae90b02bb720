"""rv_world_detached on the GPU: the union-find kernels over the brick records against the numpy restatement
(tests/np_detached.py) run on the context's exported bits -- mask words, counts and every field of every
component, exactly -- and, where the world is at least 32 wide, against rv_world_detached_at.  Then what the
call promises around the query: frames do not notice it, RV_DETACHED_CLEAR ends like the rv_world_edit that
clears the same voxels, persistence, scrolling, scratch regrowth, counters and status codes."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import dims, pack, rv, same_frames, same_tables, same_world, synthetic_voxels, tables, voxels, world
import np_bodies as B
import np_detached as D
from test_world_detached import BOXES32, island, random32, same

pytestmark = pytest.mark.gpu

CLEAR = 1


def lg_of(vox):
    return tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])


def _context(rv, lg, vox=None, **kw):
    r = rv.StateRender(lg, 64, 64, **kw)
    if vox is None:
        r.world_build()
    else:
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
    return r


def _exported(rv, r, lg):
    bits = r.world_export(rv.RV_WORLD_BITS)
    return bits, voxels(bits, lg)


def check(rv, r, lg, box, what, vox=None, bits=None):
    """The context's answer for the box equals the restatement's on its exported bits (and the host form's)."""
    if vox is None:
        bits, vox = _exported(rv, r, lg)
    want = D.detached(vox, box)
    got = r.world_detached(box)
    same(got, want, what)
    if lg[0] >= 5 and bits is not None:
        at = rv.detached_at(lg, bits, box)
        same(at, want, (what, "host form"))
    return want


def x_runs(det, box):
    """The detached voxels as clear boxes for rv_world_edit, one per run along x."""
    x0, y0, z0 = box[:3]
    out = []
    for z, y in zip(*np.nonzero(det.any(axis=2))):
        row = np.concatenate([[False], det[z, y], [False]])
        edge = np.flatnonzero(row[1:] != row[:-1])
        for a, b in zip(edge[::2], edge[1::2]):
            out.append((x0 + int(a), y0 + int(y), z0 + int(z), x0 + int(b), y0 + int(y) + 1, z0 + int(z) + 1, 0))
    return out


# ---------------------------------------------------------------- 1. the query against the restatement
def test_cpu_cases_32(rv):
    r = rv.StateRender((5, 5, 5), 64, 64)
    for d in (0.1, 0.3, 0.6):
        vox = random32(d, 1)
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        for box in BOXES32 + [(7, 0, 0, 8, 32, 32), (0, 9, 0, 32, 10, 32), (0, 0, 11, 32, 32, 12), (10, 10, 10, 11, 11, 11)]:
            check(rv, r, (5, 5, 5), box, (d, box), vox, pack(vox))
    # the outside rule: an island on each face of the box, loose and held by a voxel outside; floor, sky, walls
    for axis in range(3):
        for side in (0, 1):
            at, out = [12, 12, 12], [13, 13, 13]
            at[axis], out[axis] = (17, 20) if side else (8, 7)
            vox = island(at)
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            assert check(rv, r, (5, 5, 5), (8, 8, 8, 20, 20, 20), ("loose", axis, side), vox)[1] == 27
            vox[out[2], out[1], out[0]] = True
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            assert check(rv, r, (5, 5, 5), (8, 8, 8, 20, 20, 20), ("held", axis, side), vox)[1] == 0
    for at, box, n in [((12, 0, 12), (8, 0, 8, 20, 12, 20), 0), ((12, 29, 12), (8, 20, 8, 20, 32, 20), 27),
                       ((0, 12, 12), (0, 8, 8, 12, 20, 20), 0), ((29, 12, 12), (20, 8, 8, 32, 20, 20), 0),
                       ((12, 12, 0), (8, 8, 0, 20, 20, 12), 0), ((12, 12, 29), (8, 8, 20, 20, 20, 32), 0),
                       ((1, 12, 12), (0, 8, 8, 12, 20, 20), 27)]:
        vox = island(at)
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        assert check(rv, r, (5, 5, 5), box, (at, box), vox)[1] == n
    # the checkerboard: one-voxel components only, and cap
    board = D.checkerboard()
    r.world_import(rv.RV_WORLD_BITS, pack(board))
    box = (1, 1, 1, 31, 31, 31)
    want = check(rv, r, (5, 5, 5), box, "checkerboard", board, pack(board))
    assert want[1] == 13500 == len(want[0])
    got = r.world_detached(box, cap=10)
    assert got[1] == 13500 and got[2] == 13500 and len(got[0]) == 10
    for f in ("seed", "lo", "hi", "voxels"):
        assert np.array_equal(got[0][f], want[0][f][:10]), f
    got = r.world_detached(box, cap=0, want_mask=False)
    assert got[1] == 13500 and got[3] is None and len(got[0]) == 0
    r.close()


@pytest.mark.parametrize("held", [False, True])
def test_long_path(rv, held):
    vox, cells, box, contact = D.long_path()
    if held:
        vox[contact[2], contact[1], contact[0]] = True
    r = _context(rv, (5, 5, 5), vox)
    want = check(rv, r, (5, 5, 5), box, ("path", held), vox, pack(vox))
    assert want[1] == (0 if held else len(cells)) and len(want[0]) == (0 if held else 1)
    r.close()


def test_bars_and_ragged_worlds(rv):
    for anchor in (False, True):
        vox, box = D.bars(anchor)
        r = _context(rv, (6, 5, 5), vox)
        want = check(rv, r, (6, 5, 5), box, ("bars", anchor), vox, pack(vox))
        assert want[1] == (0 if anchor else 12)
        r.close()
    lg = (5, 7, 6)
    vox = synthetic_voxels("blocks", 32, 128, 64, np.random.default_rng(21))
    r = _context(rv, lg, vox)
    assert check(rv, r, lg, (0, 0, 0, 32, 128, 64), "ragged, whole", vox, pack(vox))[1] > 0
    check(rv, r, lg, (3, 2, 5, 30, 125, 59), "ragged, inner", vox, pack(vox))
    r.close()
    vox = np.random.default_rng(22).random((16, 16, 16)) < 0.3
    r = _context(rv, (4, 4, 4), vox)
    assert check(rv, r, (4, 4, 4), (0, 0, 0, 16, 16, 16), "tiny", vox)[1] > 0
    check(rv, r, (4, 4, 4), (1, 2, 3, 15, 16, 14), "tiny, inner", vox)
    r.close()


def terrain_edit(vox):
    """Edit boxes that put a 5 x 2 x 5 slab over the terrain and a pillar cut by a one-voxel gap, both inside
    [32, 96)^3 of the 128^3 columns starting at x = 0 (vox: [z, y, x])."""
    top = lambda x, z: int(vox[z, :, x].nonzero()[0].max()) + 1   # noqa: E731
    h = max(32, max(top(x, z) for x in range(60, 65) for z in range(60, 65)))
    g0 = top(72, 72)
    g = max(32, g0)
    assert h + 6 < 96 and g + 10 < 96
    return [(60, h + 3, 60, 65, h + 5, 65, 1), (72, g0, 72, 73, g + 9, 73, 1), (72, g + 4, 72, 73, g + 5, 73, 0)], (h, g)


def test_terrain_slab_and_cut_pillar(rv):
    lg = (7, 7, 7)
    r = _context(rv, lg)
    boxes, (h, g) = terrain_edit(_exported(rv, r, lg)[1])
    r.world_edit(boxes)
    bits, vox = _exported(rv, r, lg)
    comps = check(rv, r, lg, (32, 32, 32, 96, 96, 96), "terrain", vox, bits)[0]
    found = {(tuple(c["lo"]), tuple(c["hi"]), int(c["voxels"])) for c in comps}
    assert ((60, h + 3, 60), (65, h + 5, 65), 50) in found and ((72, g + 5, 72), (73, g + 9, 73), 4) in found
    r.close()


def test_many_waves_race(rv):
    """128 x 32 x 128 at density 0.3: 16 K word lanes, enough waves on enough CUs for the merges to race.  Two
    calls give identical bytes."""
    lg = (7, 5, 7)
    vox = np.random.default_rng(5).random((128, 32, 128)) < 0.3
    r = _context(rv, lg, vox)
    box = (0, 0, 0, 128, 32, 128)
    want = check(rv, r, lg, box, "race", vox, pack(vox))
    assert len(want[0]) > 5000 and want[0]["voxels"].max() > 100
    a, b = r.world_detached(box), r.world_detached(box)
    assert a[1:3] == b[1:3] and a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    r.close()


# ---------------------------------------------------------------- 2. the frames do not notice
@pytest.mark.parametrize("mode,in_flight", [("seq", 2), ("group", 1)])
def test_frames_are_untouched(rv, atlas, mode, in_flight):
    """A twin renders the same pipelined or grouped frames without the calls in between: queries, and clears
    that find nothing (whatever the generated terrain had loose in the box both contexts cleared before)."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H = (7, 7, 7), 160, 96
    flags = rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2 * n, pan=0.01, ref_compat=True)
    box = (40, 8, 40, 104, 72, 104)
    r, t = (rv.StateRender(lg, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=4096) for _ in range(2))
    try:
        for c in (r, t):
            c.world_build()
            c.world_detached(box, CLEAR, cap=0, want_mask=False)
            c.gi_update(0)
            if in_flight > 1:
                c.set_frames_in_flight(in_flight)
            if mode == "group":
                c.set_frame_group(2)
        info, calls = r.world_edit_info(), r.world_detached_info()[0]
        first = None
        for k0 in (0, n):
            got = r.world_detached((32, 0, 32, 96, 64, 96))
            assert r.world_detached(box, CLEAR)[2] == 0
            for c in (r, t):
                c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
            assert r.world_detached(box, CLEAR, cap=0)[2] == 0
            again = r.world_detached((32, 0, 32, 96, 64, 96))
            same_frames(rv, r, t, k0)
            first = first or got
            for x in (got, again):
                assert x[1:3] == first[1:3] and x[0].tobytes() == first[0].tobytes() and np.array_equal(x[3], first[3])
        assert r.world_edit_info() == info == t.world_edit_info()
        assert r.world_detached_info()[0] > calls and t.world_detached_info()[0] == calls
        assert r.flow_info() == t.flow_info()
    finally:
        r.close()
        t.close()


# ---------------------------------------------------------------- 3. RV_DETACHED_CLEAR
@pytest.mark.parametrize("lg,full", [((9, 7, 7), False), ((7, 7, 7), True)])
def test_clear_equals_the_edit(rv, lg, full):
    box = (32, 32, 32, 96, 96, 96)
    r, t = _context(rv, lg), _context(rv, lg)
    scene, (h, g) = terrain_edit(_exported(rv, r, lg)[1])
    for c in (r, t):
        c.world_edit(scene)
    bits, vox = _exported(rv, r, lg)
    want = D.detached(vox, box)
    runs = x_runs(want[3], box)
    assert 14 <= len(runs) <= 1024 and want[1] >= 54

    # a body falls onto the slab while it is there
    body = ([(62.2, h + 12.0, 62.2)], (0.6, 0.6, 0.6), (0.0, -11.0, 0.0))
    on = r.bodies_move(*body)
    assert on[1][0] == B.YN and on[0][0][1] == h + 5.0

    r.world_persist(True)
    got = r.world_detached(box, CLEAR)
    same(got, want, "the results are those of before the clear")
    t.world_edit(runs)
    same_world(rv, r, t, "bits and csdf")
    same_tables(tables(rv, r), tables(rv, t), "exits")
    assert r.world_edit_info() == t.world_edit_info() and r.world_edit_info()[2] is full
    # ... and a bits import of the restated world + a whole-grid build
    u = rv.StateRender(lg, 64, 64)
    u.world_import(rv.RV_WORLD_BITS, pack(D.cleared(vox, box)))
    u.csdf_build()
    same_world(rv, r, u, "restated")
    u.close()
    # persistence: the columns under each component's bounding box
    cols = {(bx, bz) for c in want[0] for bx in range(c["lo"][0] >> 3, ((c["hi"][0] - 1) >> 3) + 1)
            for bz in range(c["lo"][2] >> 3, ((c["hi"][2] - 1) >> 3) + 1)}
    assert r.world_persist_info()["dirty_columns"] == len(cols)
    # the body now passes through where the slab was, as in the twin
    through = r.bodies_move(*body)
    assert through[1][0] == 0 and through[0][0][1] == h + 1.0
    tw = t.bodies_move(*body)
    assert np.array_equal(through[0], tw[0]) and np.array_equal(through[1], tw[1])
    # a second clear finds nothing and changes nothing
    info, w0 = r.world_edit_info(), world(rv, r)
    again = r.world_detached(box, CLEAR)
    assert again[1] == 0 and again[2] == 0 and not again[3].any()
    assert r.world_edit_info() == info
    for a, b in zip(world(rv, r), w0):
        assert np.array_equal(a, b)
    assert r.world_detached_info() == (2, 2 * 64 ** 3, want[1])
    r.close()
    t.close()


# ---------------------------------------------------------------- 4. after a scroll
def test_after_a_scroll(rv):
    lg = (7, 7, 7)
    r = _context(rv, lg, seed=(24, -8))
    scene, _ = terrain_edit(_exported(rv, r, lg)[1])
    r.world_edit(scene)
    box = np.array([40, 32, 40, 88, 96, 88])
    before = r.world_detached(tuple(box))
    assert before[1] >= 2
    rng = np.random.default_rng(7)
    for (dx, dz) in ((8, 0), (0, -16)):
        r.world_scroll(dx, dz)
        shift = np.array([dx, 0, dz])
        box = box - np.tile(shift, 2)
        got = r.world_detached(tuple(box))
        assert got[1:3] == before[1:3] and np.array_equal(got[3], before[3])
        for f in ("seed", "lo", "hi"):
            assert np.array_equal(got[0][f] + shift, before[0][f]), (dx, dz, f)
        assert np.array_equal(got[0]["voxels"], before[0]["voxels"])
        before = got
        lo = rng.integers(0, 64, 3)
        hi = lo + rng.integers(20, 64, 3)
        bits, vox = _exported(rv, r, lg)
        check(rv, r, lg, tuple(int(v) for v in np.concatenate([lo, hi])), ("anywhere", dx, dz), vox, bits)
    r.close()


# ---------------------------------------------------------------- 5. scratch regrowth
def test_scratch_regrowth(rv):
    vox = np.random.default_rng(9).random((64, 64, 64)) < 0.3
    boxes = [(20, 20, 20, 28, 28, 28), (0, 0, 0, 64, 64, 64), (20, 20, 20, 28, 28, 28)]
    fresh = []
    for box in boxes[:2]:
        f = _context(rv, (6, 6, 6), vox)
        fresh.append(f.world_detached(box))
        f.close()
    fresh.append(fresh[0])
    assert fresh[0][2] > 0 and fresh[1][2] > 0
    r = _context(rv, (6, 6, 6), vox)
    for box, want in zip(boxes, fresh):
        got = r.world_detached(box)
        assert got[1:3] == want[1:3] and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[3], want[3])
    r.close()


# ---------------------------------------------------------------- 6. status codes and counters
def test_status_codes_and_counters(rv):
    L, lib = rv._lib.load(), rv._lib
    r = rv.StateRender((5, 5, 5), 64, 64)
    comps = np.zeros(8, rv.COMPONENT_DTYPE)
    mask = np.zeros(1024, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, v = C.c_int64(), C.c_uint64()

    def call(box=(0, 0, 0, 32, 32, 32), flags=0, comps_=comps, cap=8, mask_=mask, nbytes=4096):
        b = None if box is None else C.byref(lib.rv_voxel_box(*box))
        return L.rv_world_detached(r._h, b, flags, None if comps_ is None else p(comps_), cap, C.byref(n), C.byref(v),
                                   None if mask_ is None else p(mask_), nbytes)
    try:
        assert call() == lib.RV_ERR_STATE
        with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
            r.world_detached((0, 0, 0, 8, 8, 8))
        vox = random32(0.3, 1)
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
        assert r.world_detached_info() == (0, 0, 0)
        before, info = world(rv, r), r.world_edit_info()
        bad = [dict(box=None), dict(box=(4, 4, 4, 4, 8, 8)), dict(box=(4, 8, 4, 8, 8, 8)), dict(box=(4, 4, 9, 8, 8, 8)),
               dict(box=(-1, 0, 0, 8, 8, 8)), dict(box=(0, 0, 0, 33, 8, 8)), dict(box=(0, 0, 0, 8, 33, 8)),
               dict(box=(0, 0, -2, 8, 8, 8)), dict(flags=2), dict(flags=-1), dict(flags=3), dict(cap=-1),
               dict(comps_=None, cap=1), dict(nbytes=4092)]
        for kw in bad:
            assert call(**kw) == lib.RV_ERR_INVALID, kw
            assert call(**{**kw, "flags": kw.get("flags", 0) | CLEAR}) == lib.RV_ERR_INVALID, kw
        for a, b in zip(world(rv, r), before):
            assert np.array_equal(a, b)
        assert r.world_edit_info() == info and r.world_detached_info() == (0, 0, 0)
        assert call() == lib.RV_OK and call(mask_=None, nbytes=0) == lib.RV_OK and call(comps_=None, cap=0) == lib.RV_OK
        assert L.rv_world_detached(r._h, C.byref(lib.rv_voxel_box(0, 0, 0, 32, 32, 32)), 0, None, 0, None, None, None,
                                   0) == lib.RV_OK
        assert r.world_detached_info() == (4, 4 * 32 ** 3, 0)
        want = D.detached(vox, (0, 0, 0, 32, 16, 32))
        assert call(box=(0, 0, 0, 32, 16, 32), flags=CLEAR) == lib.RV_OK and v.value == want[1] > 0
        assert r.world_detached_info() == (5, 4 * 32 ** 3 + 32 * 16 * 32, want[1])
        assert r.world_edit_info()[0] == info[0] + 1
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(D.cleared(vox, (0, 0, 0, 32, 16, 32))))
        c, s, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.rv_world_detached_info(r._h, None, None, None) == lib.RV_OK
        assert L.rv_world_detached_info(r._h, C.byref(c), C.byref(s), C.byref(k)) == lib.RV_OK
        assert (c.value, s.value, k.value) == r.world_detached_info()
    finally:
        r.close()
