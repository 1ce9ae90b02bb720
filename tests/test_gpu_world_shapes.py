"""rv_world_edit_shapes on the GPU: k_edit_shapes over the brick records against the numpy restatement
(tests/np_shapes.py) and against rv_world_edit_shapes_at -- the exported bits and both counts, exactly -- on the
scenes of tests/test_world_shapes.py.  Then what the call promises around the bits: the whole state equals a
twin that made the same change by rv_world_edit x-runs and a twin that imported the restated world and built
its CSDF, rv_world_edit_info reports the call like the edit of the union box, a call that changes nothing touches
nothing, persistence, detached voxels, world_blast, bodies, scratch regrowth, a seeded mixed session against a
host model, and the status codes."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import (generated, pack, rv, same_frames, same_tables, same_world, sun, synthetic_voxels,  # noqa: F401
                       tables, voxels, world)
import np_bodies as B
import np_fall as F
import np_shapes as S
from test_gpu_world_detached import x_runs
from test_gpu_world_fall import _camera, _context
from test_world_shapes import CX, CY, CZ, E, lg_of, random_shapes, scenes, sphere

pytestmark = pytest.mark.gpu

W = H = 64
ZERO = (0,) * 6


def check(rv, r, vox, shapes, what=None):
    """The context (holding vox) changes as the restatement and the host form do; returns the restatement's."""
    lg = lg_of(vox)
    want = S.apply(vox, shapes)
    got = r.world_edit_shapes(shapes)
    assert got == want[1:], (what, got, want[1:])
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0])), (what, "bits")
    at = rv.edit_shapes_at(lg, pack(vox), shapes)
    assert at[1:] == want[1:] and np.array_equal(at[0], pack(want[0])), (what, "host form")
    return want


# ---------------------------------------------------------------- 1. device = restatement = host form
@pytest.mark.parametrize("lg", [(5, 5, 5), (6, 6, 6), (7, 5, 6)])
def test_scenes(rv, lg):
    X, Y, Z = (1 << l for l in lg)
    worlds = {"empty": np.zeros((Z, Y, X), bool), "solid": np.ones((Z, Y, X), bool),
              "random": np.random.default_rng(3).random((Z, Y, X)) < 0.5}
    r = rv.StateRender(lg, W, H)
    try:
        for name, shapes in scenes(lg).items():
            assert name != "many" or len(shapes) == rv._lib.RV_EDIT_MAX_SHAPES
            for wname, vox in worlds.items():
                r.world_import(rv.RV_WORLD_BITS, pack(vox))
                want = check(rv, r, vox, shapes, (lg, name, wname))
                assert wname != "random" or want[1] + want[2] > 0, (lg, name)   # the scene did something
    finally:
        r.close()


@pytest.mark.parametrize("seed", range(3))
def test_random_lists(rv, seed):
    rng = np.random.default_rng(200 + seed)
    vox = rng.random((128, 32, 64)) < 0.5   # 64 x 32 x 128
    lg = lg_of(vox)
    r = rv.StateRender(lg, W, H)
    try:
        for n in (1, 3, 8):
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            check(rv, r, vox, random_shapes(rng, lg, n), (seed, n))
    finally:
        r.close()


# ---------------------------------------------------------------- 2. the whole state equals a twin
def _blocks(lg, seed):
    X, Y, Z = (1 << l for l in lg)
    return synthetic_voxels("blocks", X, Y, Z, np.random.default_rng(seed))


# name -> (log2 dims, shapes, whether the whole-grid CSDF build runs).  The local rebuild needs an axis longer
# than 256 voxels: the rebuilt region is the union box grown by 64 coarse cells, and its input boxes by 128.
TWIN_SCENES = {
    # a crater next to a boulder that straddles the brick boundary x = 208, in a long window: the local rebuild
    "local": ((9, 5, 5), [sphere((401, 21, 33), 14, 0), (E, 1, (416, 33, 32), (9, 5, 7))], False),
    # a crater in the wall x = 0, a shaft, a dome on the floor: the whole-grid build
    "whole": ((6, 6, 6), [sphere((0, 40, 67), 22, 0), (CY, 0, (81, 64, 48), (7, 50, 7)), sphere((65, 4, 65), 16)], True),
    # a shell through the window's far z face and a tunnel along x through everything
    "faces": ((7, 5, 6), [sphere((120, 30, 126), 20), sphere((120, 30, 126), 12, 0), (CX, 0, (128, 33, 90), (512, 5, 6))],
              True),
}


@pytest.mark.parametrize("name", list(TWIN_SCENES))
def test_scene_equals_the_twin(rv, atlas, name):
    lg, shapes, full = TWIN_SCENES[name]
    vox = _blocks(lg, 7)
    r, t, u = _context(rv, vox, atlas), _context(rv, vox, atlas), None
    try:
        cam, vp = _camera(rv, lg)
        r.gi_update(0)
        r.frame(cam, vp)
        info = r.world_edit_info()
        want = check(rv, r, vox, shapes, name)
        assert want[1] > 0 and want[2] > 0
        each, union = rv.edit_shapes_box(lg, shapes)
        assert (each, union) == S.boxes(lg, shapes) and ZERO not in each
        assert r.world_edit_info() == (info[0] + 1, rv.edit_region(lg, [union + (0,)])[1], full)
        # a twin that makes the same change by rv_world_edit, one box per run along x
        boxes = x_runs(vox & ~want[0], ZERO) + [b[:6] + (1,) for b in x_runs(want[0] & ~vox, ZERO)]
        assert 0 < len(boxes) <= rv._lib.RV_EDIT_MAX_BOXES
        t.world_edit(boxes)
        same_world(rv, r, t, "the edit")
        same_tables(tables(rv, r), tables(rv, t), "the edit's exits")
        # a twin that imported the restated world and built its CSDF whole
        u = _context(rv, want[0], atlas)
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


# ---------------------------------------------------------------- 3. nothing changed, nothing touched
@pytest.mark.parametrize("mode,in_flight", [("seq", 2), ("group", 1)])
def test_nothing_changed_touches_nothing(rv, atlas, mode, in_flight):
    """A twin renders the same pipelined or grouped frames without the calls in between: they clear air, set
    solid voxels or lie outside the window, so they discard no work computed ahead and mark no column."""
    from rvgrt_amd.configs import camera_path
    lg, flags = (6, 6, 6), rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(((55.0, 40.0, 60.0), 2.44, -3.4415927), W, H, 2 * n, pan=0.01, ref_compat=True)
    r, t = (rv.StateRender(lg, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=1024) for _ in range(2))
    try:
        for c in (r, t):
            c.world_build()
            c.gi_update(0)
            if in_flight > 1:
                c.set_frames_in_flight(in_flight)
            if mode == "group":
                c.set_frame_group(2)
        r.world_persist(True)
        vox = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
        air, rock = np.argwhere(~vox), np.argwhere(vox)
        pick = lambda a, k: tuple(2 * int(v) + 1 for v in a[(k * 7919) % len(a)][::-1])   # noqa: E731 -- [z, y, x] -> c2
        idle = [sphere(pick(air, k), 1, 0) for k in range(5)] + [sphere(pick(rock, k), 1, 1) for k in range(5)] + \
            [sphere((-30, 64, 64), 20, 0), (CY, 1, (64, 64, 2 * 64 + 9), (8, 512, 8))]
        assert S.apply(vox, idle)[1:] == (0, 0)
        info, w0 = r.world_edit_info(), world(rv, r)
        for k0 in (0, n):
            assert r.world_edit_shapes(idle) == (0, 0)
            for c in (r, t):
                c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
            assert r.world_edit_shapes(idle[:3]) == (0, 0)
            same_frames(rv, r, t, k0)
        assert r.world_edit_info() == (info[0], 0, False) and t.world_edit_info() == info
        assert r.flow_info() == t.flow_info()
        assert r.world_persist_info()["dirty_columns"] == 0
        for a, b in zip(world(rv, r), w0):
            assert np.array_equal(a, b)
    finally:
        r.close()
        t.close()


# ---------------------------------------------------------------- 4. with the rest
def _columns(boxes):
    return {(bx, bz) for b in boxes if b != ZERO for bx in range(b[0] >> 3, ((b[3] - 1) >> 3) + 1)
            for bz in range(b[2] >> 3, ((b[5] - 1) >> 3) + 1)}


def test_persistence_and_scrolling(rv, oracle):
    """The dirty columns are exactly those under the non-empty clipped boxes; a crater that scrolls out and back
    is restored bit for bit."""
    lg, origin = (6, 6, 6), (40, -24)
    r = rv.StateRender(lg, W, H, seed=origin)
    try:
        r.world_build()
        bits = generated(oracle, lg, origin)
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), bits)
        vox = voxels(bits, lg)
        top = int(np.flatnonzero(vox[20, :, 12])[-1])   # the surface at (12, ., 20)
        az, ay, ax = (int(v) for v in np.argwhere(~vox)[int((~vox).sum()) // 2])   # a voxel of air
        # a crater at the surface, a shape outside the window, and a post set around that voxel
        shapes = [sphere((25, 2 * top + 1, 41), 13, 0), sphere((-40, 64, 64), 20, 0),
                  (CY, 1, (2 * ax + 1, 2 * ay + 1, 2 * az + 1), (5, 9, 3))]
        r.world_persist(True)
        want = check(rv, r, vox, shapes, "crater")
        assert want[2] > 100 and want[1] > 0
        each, _ = S.boxes(lg, shapes)
        assert each[1] == ZERO and len(_columns(each)) >= 5
        assert r.world_persist_info()["dirty_columns"] == len(_columns(each))
        r.world_persist_flush()
        keys = {(origin[0] + 8 * bx, origin[1] + 8 * bz) for bx, bz in _columns(each)}
        assert {tuple(k) for k in r.world_store_list().tolist()} == keys
        r.world_scroll(64, 0)    # every column leaves ...
        assert r.world_persist_info()["dirty_columns"] == 0
        r.world_scroll(-64, 0)   # ... and the edited ones come back as they were left
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0]))
        assert r.world_persist_info()["dirty_columns"] == len(keys)
    finally:
        r.close()


def _pillar():
    """A floor, and a 3 x 3 pillar from it to row 21 at (15..17, ., 15..17)."""
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :4] = True
    vox[15:18, 4:22, 15:18] = True
    return vox


def test_detached_after_a_carve(rv):
    vox = _pillar()
    r = _context(rv, vox)
    try:
        want = check(rv, r, vox, [sphere((33, 21, 33), 8, 0)], "undercut")   # through the pillar at rows 7..13
        assert not want[0][15:18, 8:13, 15:18].any()
        comps, n, v, _ = r.world_detached((8, 4, 8, 24, 32, 24))
        top = want[0][15:18, 13:22, 15:18]
        assert n == 1 and v == int(top.sum()) and comps[0]["hi"].tolist() == [18, 22, 18]
        assert comps[0]["lo"][1] >= 10
    finally:
        r.close()


def _lamp():
    """A floor, a post on it from row 4 to row 11 at (16, ., 16) and a 3 x 3 cap on the post, at row 12."""
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :4] = True
    vox[16, 4:12, 16] = True
    vox[15:18, 12, 15:18] = True
    return vox


def test_blast(rv, atlas):
    """The blast takes the post out from under the cap (rows 5..11); the cap, inside the settled box, comes down
    onto the stub."""
    vox = _lamp()
    r = _context(rv, vox, atlas)
    try:
        r.gi_update(0)
        calls = r.gi_relight_info()[0]
        out = r.world_blast((16, 8, 16), 3, settle=True, relight=2)
        cleared = S.apply(vox, [sphere((33, 17, 33), 6, 0)])
        assert out["edit"] == cleared[1:] == (0, 7) and out["box"] == S.boxes((5, 5, 5), [sphere((33, 17, 33), 6, 0)])[1]
        assert out["settle"] is not None and sum(rounds for rounds, _ in out["settle"]) >= 1   # the top came down
        after = voxels(r.world_export(rv.RV_WORLD_BITS), (5, 5, 5))
        assert int(after.sum()) == int(vox.sum()) - out["edit"][1]
        assert after[15:18, 5, 15:18].all() and not after[:, 6:, :].any()   # the cap on the stub (row 4)
        union = out["box"]
        for _, b in out["settle"]:
            if b != ZERO:
                union = tuple(min(union[a], b[a]) for a in range(3)) + tuple(max(union[3 + a], b[3 + a]) for a in range(3))
        grown = tuple(max(union[a] - 1, 0) for a in range(3)) + tuple(min(union[3 + a] + 1, 32) for a in range(3))
        assert r.world_detached(grown)[1:3] == (0, 0)
        assert out["relight"] is not None and r.gi_relight_info()[0] == calls + 1
        # the same world as the restatement: the carve, then the settling
        assert np.array_equal(after, F.settle(cleared[0], tuple(max(out["box"][a] - 1, 0) for a in range(3)) +
                                              tuple(min(out["box"][3 + a] + 1, 32) for a in range(3)))[2])
        # without settling or relighting: a plain clear; outside the window: nothing
        assert r.world_blast((5, 2, 5), 2, settle=False)["settle"] is None
        assert r.world_blast((-40, 2, 5), 2) == {"edit": (0, 0), "box": ZERO, "settle": None, "relight": None}
    finally:
        r.close()


def test_bodies_see_the_crater(rv):
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :16] = True
    r = _context(rv, vox)
    try:
        body = ([(15.7, 24.0, 15.7)], (0.6, 0.6, 0.6), (0.0, -20.0, 0.0))
        on = r.bodies_move(*body)
        assert on[1][0] == B.YN and on[0][0][1] == 16.0
        want = check(rv, r, vox, [sphere((33, 31, 33), 10, 0)], "crater")
        on, ref = r.bodies_move(*body), B.move(want[0], *body, 0)
        assert on[1][0] == B.YN and on[0][0][1] == ref[0][0][1] == 11.0
    finally:
        r.close()


def test_scratch_regrowth(rv):
    lg = (6, 5, 6)
    vox = np.random.default_rng(11).random((64, 32, 64)) < 0.4
    rng = np.random.default_rng(12)
    r = _context(rv, vox)
    try:
        for n in (2, rv._lib.RV_EDIT_MAX_SHAPES, 3, 40):
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            want = check(rv, r, vox, random_shapes(rng, lg, n, rmax=12), ("regrowth", n))
            assert want[1] + want[2] > 0
    finally:
        r.close()


# ---------------------------------------------------------------- 5. a seeded mixed session
def _session_model(oracle, lg, origin):
    """np_session.Session with the two calls it does not know: shaped edits and falls, restated from the header."""
    import np_session as NS

    class ShapeSession(NS.Session):
        def _finish(self, box):
            region, cells = NS.edit_region(self.lg, [box + (0,)])
            half = [1 << (l - 1) for l in self.lg]
            self.edits += 1
            self.edit_cells, self.edit_full = cells, region == (0, half[0], 0, half[1], 0, half[2])

        def shapes(self, shapes):
            if not shapes:
                return
            after, n_set, n_cleared = S.apply(self.vox, shapes)
            self.last = (n_set, n_cleared)
            if n_set + n_cleared == 0:
                self.edit_cells, self.edit_full = 0, False
                return
            each, union = S.boxes(self.lg, shapes)
            self.vox = after
            if self.persist_on:
                for b in each:
                    self._mark(sorted(_columns([b])))
            self._finish(union)

        def fall(self, box):
            comps, _, changed, after, _ = F.fall(self.vox, box)
            self.last = len(comps)
            if len(comps) == 0:
                return
            self.vox = after
            if self.persist_on:
                for c in comps["comp"]:
                    self._mark(sorted(_columns([tuple(c["lo"].tolist()) + tuple(c["hi"].tolist())])))
            self._finish(tuple(changed))

    return NS, ShapeSession(oracle, lg, origin, gi=False)


def _session_trace(NS, m, seed, n):
    """n calls drawn from the seed on a model of its own: shaped edits (craters at the surface, boulders in
    them, shapes through the faces), box edits, scrolls along x, persistence off and on, falls, flushes."""
    rng = np.random.default_rng(seed)
    X, Y, Z = (1 << l for l in m.lg)
    trace, last = [("persist", 1)], None
    m.apply(trace[0])
    while len(trace) < n:
        k = rng.uniform()
        if k < 0.40:
            c = (int(rng.integers(-4, 2 * X + 5)), int(rng.integers(20, 2 * Y + 5)), int(rng.integers(-4, 2 * Z + 5)))
            shapes = [sphere(c, int(rng.integers(6, 22)), 0)]
            if rng.uniform() < 0.6:   # something left floating in the crater
                shapes.append((int(rng.integers(0, 4)), 1, tuple(int(v + rng.integers(-3, 4)) for v in c),
                               tuple(int(v) for v in rng.integers(1, 7, 3))))
            if rng.uniform() < 0.3:
                shapes += random_shapes(rng, m.lg, int(rng.integers(1, 4)), rmax=14)
            last = S.boxes(m.lg, shapes)[1]
            op = ("shapes", tuple(shapes))
        elif k < 0.50:
            op = ("shapes", (sphere((2 * X + 60, Y, Z), 20, 0),)) if rng.uniform() < 0.5 else \
                ("shapes", (sphere((33, 2 * Y + 41, 33), 40, 0),))   # outside; above the window's top rows
        elif k < 0.62:
            op = ("edit", tuple(NS._small_box(rng, m, "any") for _ in range(int(rng.integers(1, 3)))))
        elif k < 0.78:
            op = ("scroll", 8 * int(rng.choice([-4, -2, -1, 1, 2, 4])), 0 if rng.uniform() < 0.8 else 8 * int(rng.choice([-1, 1])))
            last = None
        elif k < 0.90 and last is not None and last != ZERO:
            op = ("fall", tuple(max(last[a] - 1, 0) for a in range(3)) + tuple(min(last[3 + a] + 1, d) for a, d in
                                                                              zip(range(3), (X, Y, Z))))
        elif k < 0.95:
            op = ("persist", int(not m.persist_on))
        else:
            op = ("flush",)
        m.apply(op)
        trace.append(op)
    return trace + [("persist", 1), ("flush",)]


def test_mixed_session(rv, oracle, sun):
    import np_exits as EX
    from test_gpu_world_session import _same_store
    lg, origin, seed, n = (9, 5, 5), (40, -24), 1, 38
    NS, gen = _session_model(oracle, lg, origin)
    trace = _session_trace(NS, gen, seed, n)
    names = [op[0] for op in trace]
    assert len(trace) == n + 2 and min(names.count(k) for k in ("shapes", "edit", "scroll", "fall", "persist")) >= 2
    _, m = _session_model(oracle, lg, origin)
    r = rv.StateRender(lg, W, H, seed=origin)
    fell = changed = idle = 0
    try:
        r.world_build()
        for i, op in enumerate(trace):
            what = f"seed {seed}, call {i} {op!r}"
            if op[0] == "shapes":
                got = r.world_edit_shapes(op[1])
            elif op[0] == "fall":
                got = r.world_fall(op[1], cap=0)[1]
            elif op[0] == "edit":
                r.world_edit(op[1])
            elif op[0] == "scroll":
                r.world_scroll(*op[1:])
            elif op[0] == "persist":
                r.world_persist(op[1])
            else:
                r.world_persist_flush()
            m.apply(op)
            if op[0] in ("shapes", "fall"):
                assert got == m.last, (what, got, m.last)
                fell += op[0] == "fall" and got > 0
                changed += op[0] == "shapes" and sum(got) > 0
                idle += op[0] == "shapes" and sum(got) == 0
            bits, csdf = world(rv, r)
            assert np.array_equal(bits, m.bits()), (what, "bits")
            assert np.array_equal(csdf, m.csdf()), (what, "csdf")
            EX.check_tables(EX.reference(m.vox, sun), *tables(rv, r), (what, "tables"))
            assert r.world_edit_info() == m.edit_info(), (what, "edit info", r.world_edit_info(), m.edit_info())
            assert r.world_scroll_info() == m.scroll_info(), (what, "scroll info")
            _same_store(rv, r, m, what)     # the dirty set's size, the store's keys and entries
            cols = m.dirty_columns()
            for c, col in zip(cols, r.world_columns_read(cols) if cols else []):
                assert np.array_equal(col, m.column_bits(*c)), (what, "column", c)
        # the last flush stored every dirty column of the window: the dirty sets are the same sets
        assert set(m.store) >= {m.key(*c) for c in m.dirty_columns()}
        assert fell >= 1 and changed >= 5 and idle >= 1, (fell, changed, idle)
        assert m.captured >= 1 and m.restored >= 1 and any(not f for _, _, f in m.steps), (m.captured, m.restored)
    finally:
        r.close()


# ---------------------------------------------------------------- 6. status codes
def test_status_codes(rv):
    from rvgrt_amd.render import _edit_shapes
    L, lib = rv._lib.load(), rv._lib
    r = rv.StateRender((5, 5, 5), W, H)
    a, b = C.c_uint64(77), C.c_uint64(77)
    good = sphere((33, 33, 33), 12, 0)

    def call(shapes, n=None):
        arr = _edit_shapes(shapes) if shapes is not None else None
        return L.rv_world_edit_shapes(r._h, arr, len(shapes) if n is None else n, C.byref(a), C.byref(b))
    try:
        assert call([good]) == lib.RV_ERR_STATE
        with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
            r.world_edit_shapes([good])
        vox = np.random.default_rng(2).random((32, 32, 32)) < 0.5
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
        r.world_persist(True)
        before, info = world(rv, r), r.world_edit_info()
        bad = [([good], -1), ([good] * (S.MAX_SHAPES + 1), None), (None, 1), ([good, (4, 0) + good[2:]], None),
               ([good, (-1, 0) + good[2:]], None), ([good, (E, 2) + good[2:]], None),
               ([good, (E, 1, (33, 33, 33), (0, 4, 4))], None), ([good, (E, 1, (33, 33, 33), (4, 4, S.MAX_R2 + 1))], None),
               ([good, (E, 1, (33, S.MAX_C2 + 1, 33), (4, 4, 4))], None), ([good, (E, 1, (-S.MAX_C2 - 1, 33, 33), (4, 4, 4))], None)]
        for shapes, n in bad:
            assert call(shapes, n) == lib.RV_ERR_INVALID, (shapes and shapes[-1], n)
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_edit_shapes([(9, 0) + good[2:]])
        for x, y in zip(world(rv, r), before):
            assert np.array_equal(x, y)
        assert r.world_edit_info() == info and (a.value, b.value) == (77, 77)
        assert r.world_persist_info()["dirty_columns"] == 0
        # n == 0; NULL counts; the caps themselves
        assert call([], 0) == lib.RV_OK and call(None, 0) == lib.RV_OK and r.world_edit_info() == info
        assert L.rv_world_edit_shapes(r._h, _edit_shapes([good]), 1, None, None) == lib.RV_OK
        assert r.world_edit_info()[0] == info[0] + 1
        edge = [(E, 1, (S.MAX_C2, 33, 33), (S.MAX_R2,) * 3), (CZ, 1, (33, 33, 33), (S.MAX_R2, 1, S.MAX_R2))] * (S.MAX_SHAPES // 2)
        assert call(edge) == lib.RV_OK and a.value == int((~S.apply(vox, [good])[0][:, 16, :]).sum()) and b.value == 0
    finally:
        r.close()
