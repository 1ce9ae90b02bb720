"""rv_world_fall on the GPU: the clearance and stamp kernels over the brick records against the numpy restatement
(tests/np_fall.py) -- every field of every rv_fallen, the totals, the changed box and the exported bits, exactly
-- and against rv_world_fall_at.  Then what the call promises around the move: the whole state equals a twin
that imported the moved world and built its CSDF, rv_world_edit_info reports it like the edit of the same
voxels, a call that finds nothing touches nothing, settling, persistence, scrolling, scratch regrowth, bodies,
counters and status codes."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import pack, rv, same_frames, same_tables, same_world, tables, voxels, world
import np_bodies as B
import np_detached as D
import np_fall as F
from test_gpu_world_detached import x_runs
from test_world_detached import BOXES32, random32
from test_world_fall import lg_of, same

pytestmark = pytest.mark.gpu

W = H = 64


def _context(rv, vox, atlas=None):
    lg = lg_of(vox)
    r = rv.StateRender(lg, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas) if atlas is not None else rv.StateRender(lg, W, H)
    r.world_import(rv.RV_WORLD_BITS, pack(vox))
    r.csdf_build()
    return r


def _camera(rv, lg):
    X, Y, Z = (1 << l for l in lg)
    return rv.camera_from_pose((0.86 * X, 0.6 * Y, 0.94 * Z), 2.44, -3.4415927, W, H)


def check(rv, r, vox, box, max_fall=0, what=None, parts=None):
    """The context (holding vox) moves as the restatement and the host form do; returns the restatement's."""
    want = F.fall(vox, box, max_fall, parts)
    got = r.world_fall(box, max_fall)
    same(got, want, (what, box, max_fall))
    lg = lg_of(vox)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[3])), (what, box, max_fall, "bits")
    at = rv.fall_at(lg, pack(vox), box, max_fall)
    same(at, want, (what, box, max_fall, "host form"))
    assert np.array_equal(at[4], pack(want[3]))
    return want


def edit_of(vox, box, after):
    """The rv_world_edit boxes of the same change: the detached voxels cleared, then the moved ones set, one box
    per run along x."""
    det = np.zeros(vox.shape, bool)
    x0, y0, z0, x1, y1, z1 = box
    det[z0:z1, y0:y1, x0:x1] = D.detached(vox, box)[3]
    moved = after & ~(vox & ~det)
    return x_runs(det, (0, 0, 0)) + [b[:6] + (1,) for b in x_runs(moved, (0, 0, 0))]


SCENES = {
    "stack": lambda: F.stack() + (0,),
    "stack, limited": lambda: F.stack() + (3,),
    "U": lambda: F.u_scene() + (0,),
    "C": lambda: F.c_shape() + (0,),
    "bars": lambda: D.bars(False) + (0,),
    "checkerboard": lambda: F.checker_rows() + (0,),
    "island 1": lambda: (F.island(15, 14), (8, 15, 8, 20, 21, 20), 0),
    "island 3": lambda: (F.island(15, 12), (8, 15, 8, 20, 21, 20), 0),
    "island 4": lambda: (F.island(15, 11), (8, 15, 8, 20, 21, 20), 0),
    "island 5": lambda: (F.island(15, 10), (8, 15, 8, 20, 21, 20), 0),
    "island 9": lambda: (F.island(15, 6), (8, 15, 8, 20, 21, 20), 0),
    "island 9, floor": lambda: (F.island(9), (8, 9, 8, 20, 15, 20), 0),
    "random": lambda: (random32(0.3, 1), BOXES32[1], 0),
    "random, limited": lambda: (random32(0.3, 2), BOXES32[0], 3),
}


# ---------------------------------------------------------------- 1. the move, and the whole state after it
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_equals_the_twin(rv, atlas, name):
    vox, box, max_fall = SCENES[name]()
    lg = lg_of(vox)
    r, t, u = _context(rv, vox, atlas), _context(rv, vox, atlas), None
    try:
        cam, vp = _camera(rv, lg)
        r.gi_update(0)
        r.frame(cam, vp)
        info = r.world_edit_info()
        want = check(rv, r, vox, box, max_fall, name)
        assert len(want[0]) > 0 and want[3].sum() == vox.sum()
        # a twin that makes the same change by rv_world_edit
        boxes = edit_of(vox, box, want[3])
        assert len(boxes) <= 1024 or name in ("checkerboard", "random", "random, limited")
        if len(boxes) <= 1024:
            t.world_edit(boxes)
            same_world(rv, r, t, "the edit")
            assert r.world_edit_info() == t.world_edit_info() and r.world_edit_info()[0] == info[0] + 1
        # a twin that imported the restated world and built its CSDF whole
        u = _context(rv, want[3], atlas)
        u.frame(cam, vp)   # as many frames as r
        u.world_import(rv.RV_WORLD_GI, r.world_export(rv.RV_WORLD_GI))
        same_world(rv, r, u, "restated")
        same_tables(tables(rv, r), tables(rv, u), "exits")
        for c in (r, u):
            c.frame(cam, vp)
        same_frames(rv, r, u, name)
    finally:
        for c in (r, t, u):
            if c is not None:
                c.close()


@pytest.mark.parametrize("d", [0.1, 0.3, 0.6])
def test_random_worlds(rv, d):
    r = rv.StateRender((5, 5, 5), W, H)
    try:
        for s in (1, 2):
            vox = random32(d, s)
            for box in BOXES32:
                parts = F.measured(vox, box)
                for max_fall in (0, 1, 3):
                    r.world_import(rv.RV_WORLD_BITS, pack(vox))
                    check(rv, r, vox, box, max_fall, (d, s), parts)
    finally:
        r.close()


# ---------------------------------------------------------------- 2. a call that finds nothing
@pytest.mark.parametrize("mode,in_flight", [("seq", 2), ("group", 1)])
def test_nothing_detached_touches_nothing(rv, atlas, mode, in_flight):
    """A twin renders the same pipelined or grouped frames without the calls in between: they find nothing (both
    contexts settled the box before), so they wait for nothing and discard no work computed ahead."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, w, h = (7, 7, 7), 160, 96
    flags = rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(TEST_POSES_128["P0"], w, h, 2 * n, pan=0.01, ref_compat=True)
    box = (40, 8, 40, 104, 72, 104)
    r, t = (rv.StateRender(lg, w, h, flags=flags, atlas=atlas, gi_rays_per_frame=4096) for _ in range(2))
    try:
        for c in (r, t):
            c.world_build()
            c.world_detached(box, rv.RV_DETACHED_CLEAR, cap=0, want_mask=False)
            c.gi_update(0)
            if in_flight > 1:
                c.set_frames_in_flight(in_flight)
            if mode == "group":
                c.set_frame_group(2)
        info, calls, w0 = r.world_edit_info(), r.world_fall_info(), world(rv, r)
        for k0 in (0, n):
            assert r.world_fall(box)[1:] == (0, 0, (0, 0, 0, 0, 0, 0))
            for c in (r, t):
                c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
            assert r.world_fall(box, 2, cap=0)[1:] == (0, 0, (0, 0, 0, 0, 0, 0))
            same_frames(rv, r, t, k0)
        assert r.world_edit_info() == info == t.world_edit_info()
        assert r.world_fall_info() == (calls[0] + 4, 0, 0) and t.world_fall_info() == calls
        assert r.flow_info() == t.flow_info()
        for a, b in zip(world(rv, r), w0):
            assert np.array_equal(a, b)
    finally:
        r.close()
        t.close()


# ---------------------------------------------------------------- 3. rounds
@pytest.mark.parametrize("scene", ["stack", "U"])
def test_settle(rv, scene):
    vox, box = F.stack() if scene == "stack" else F.u_scene()
    rounds, union, final = F.settle(vox, box)
    assert rounds == 2
    r = _context(rv, vox)
    try:
        assert r.world_settle(box) == (rounds, union)
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(final))
        assert r.world_detached(union)[1:3] == (0, 0)
        assert r.world_fall_info()[0] == 3 and r.world_fall_info()[1] == 3
        assert r.world_settle(box) == (0, (0, 0, 0, 0, 0, 0))
        # one row per call: as the restatement, and on the stack the same final world
        steps = F.settle(vox, box, 1)
        assert steps[0] > rounds and (scene != "stack" or np.array_equal(steps[2], final))
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        assert r.world_settle(box, max_fall=1) == steps[:2]
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(steps[2]))
        # max_rounds bounds the calls that move something
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        assert r.world_settle(box, max_rounds=1)[0] == 1
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(F.fall(vox, box)[3]))
    finally:
        r.close()


# ---------------------------------------------------------------- 4. persistence and scrolling
def _carved(rv):
    """The generated 32^3 window with everything from row 8 up cleared and a 3^3 block put at (12, 20, 12)."""
    r = rv.StateRender((5, 5, 5), W, H)
    r.world_build()
    r.world_edit([(0, 8, 0, 32, 32, 32, 0), (12, 20, 12, 15, 23, 15, 1)])
    return r


def test_persistence(rv):
    lg = (5, 5, 5)
    r = _carved(rv)
    try:
        r.world_persist(True)
        vox = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
        box = (4, 8, 4, 28, 32, 28)
        want = check(rv, r, vox, box, 0, "carved")
        assert len(want[0]) == 1 and want[0][0]["fall"] >= 12
        cols = {(bx, bz) for c in want[0]["comp"] for bx in range(c["lo"][0] >> 3, ((c["hi"][0] - 1) >> 3) + 1)
                for bz in range(c["lo"][2] >> 3, ((c["hi"][2] - 1) >> 3) + 1)}
        assert cols == {(1, 1)} and r.world_persist_info()["dirty_columns"] == len(cols)
        # away and back: the dirty column comes back as it was left, the fallen block where it landed
        r.world_scroll(16, 0)
        assert r.world_persist_info()["stored_columns"] == 1
        r.world_scroll(-16, 0)
        back = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
        assert np.array_equal(back[8:16, :, 8:16], want[3][8:16, :, 8:16])
        y = 20 - int(want[0][0]["fall"])
        assert back[12:15, y:y + 3, 12:15].all() and not back[12:15, y + 3:, 12:15].any()
    finally:
        r.close()


def test_after_a_scroll(rv):
    lg = (5, 5, 5)
    r = _carved(rv)
    try:
        r.world_scroll(8, -8)
        vox = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
        assert vox[20:23, 20:23, 4:7].all()   # the block moved with the window
        want = check(rv, r, vox, (0, 8, 8, 24, 32, 32), 0, "scrolled")
        assert [c["lo"].tolist() for c in want[0]["comp"]] == [[4, 20, 20]]
    finally:
        r.close()


# ---------------------------------------------------------------- 5. scratch regrowth
def test_scratch_regrowth(rv):
    vox = np.zeros((32, 32, 64), bool)
    vox[:, :, :32] = random32(0.3, 1)
    vox[:, :, 32:] = random32(0.3, 2)
    boxes = [(0, 0, 0, 64, 32, 32), (20, 20, 20, 28, 28, 28), (0, 0, 0, 64, 32, 32)]
    r = _context(rv, vox)
    try:
        parts = {box: F.measured(vox, box) for box in set(boxes)}
        for box in boxes:
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            assert len(check(rv, r, vox, box, 0, ("regrowth", box), parts[box])[0]) > 0
    finally:
        r.close()


# ---------------------------------------------------------------- 6. bodies see the new bits
def test_a_body_stands_on_the_fallen_block(rv):
    vox, box = F.stack()
    r = _context(rv, vox)
    try:
        body = ([(13.2, 24.0, 13.2)], (0.6, 0.6, 0.6), (0.0, -20.0, 0.0))
        on = r.bodies_move(*body)
        assert on[1][0] == B.YN and on[0][0][1] == 17.0
        assert r.world_settle(box)[0] == 2
        on = r.bodies_move(*body)
        assert on[1][0] == B.YN and on[0][0][1] == 10.0   # the column is solid for y 0..9
    finally:
        r.close()


# ---------------------------------------------------------------- 7. status codes and counters
def test_status_codes_and_counters(rv):
    L, lib = rv._lib.load(), rv._lib
    r = rv.StateRender((5, 5, 5), W, H)
    comps = np.zeros(8, rv.FALLEN_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, v, ch = C.c_int64(), C.c_uint64(), lib.rv_voxel_box()

    def call(box=(0, 0, 0, 32, 32, 32), max_fall=0, comps_=comps, cap=8):
        b = None if box is None else C.byref(lib.rv_voxel_box(*box))
        return L.rv_world_fall(r._h, b, max_fall, None if comps_ is None else p(comps_), cap, C.byref(n), C.byref(v),
                               C.byref(ch))
    try:
        assert call() == lib.RV_ERR_STATE
        with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
            r.world_fall((0, 0, 0, 8, 8, 8))
        vox, box = F.stack()
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
        assert r.world_fall_info() == (0, 0, 0)
        before, info = world(rv, r), r.world_edit_info()
        bad = [dict(box=None), dict(box=(4, 4, 4, 4, 8, 8)), dict(box=(4, 8, 4, 8, 8, 8)), dict(box=(4, 4, 9, 8, 8, 8)),
               dict(box=(-1, 0, 0, 8, 8, 8)), dict(box=(0, 0, 0, 33, 8, 8)), dict(box=(0, 0, 0, 8, 33, 8)),
               dict(box=(0, 0, -2, 8, 8, 8)), dict(cap=-1), dict(comps_=None, cap=1), dict(max_fall=-1),
               dict(max_fall=33)]
        for kw in bad:
            assert call(**{"box": box, **kw}) == lib.RV_ERR_INVALID, kw
        for a, b in zip(world(rv, r), before):
            assert np.array_equal(a, b)
        assert r.world_edit_info() == info and r.world_fall_info() == (0, 0, 0) and r.world_detached_info() == (0, 0, 0)
        # every out pointer NULL; cap below the total
        assert L.rv_world_fall(r._h, C.byref(lib.rv_voxel_box(*box)), 32, None, 0, None, None, None) == lib.RV_OK
        one = F.fall(vox, box)
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(one[3]))
        assert r.world_fall_info() == (1, 2, 54) and r.world_edit_info()[0] == info[0] + 1
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        assert call(box=box, cap=1) == lib.RV_OK and (n.value, v.value) == (2, 54)
        assert comps[0]["fall"] == 4 and comps[0]["flags"] == 1 and comps[0]["comp"]["lo"].tolist() == [12, 8, 12]
        assert not comps[1:].view(np.uint8).any()
        assert (ch.x0, ch.y0, ch.z0, ch.x1, ch.y1, ch.z1) == one[2]
        assert r.world_fall_info() == (2, 4, 108) and r.world_detached_info() == (0, 0, 0)
        c, k, m = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert L.rv_world_fall_info(r._h, None, None, None) == lib.RV_OK
        assert L.rv_world_fall_info(r._h, C.byref(c), C.byref(k), C.byref(m)) == lib.RV_OK
        assert (c.value, k.value, m.value) == r.world_fall_info()
    finally:
        r.close()
