"""rv_world_stamp and the pattern objects on the GPU: k_stamp over the brick records against the numpy restatement
(tests/np_stamp.py) and against rv_world_stamp_at -- the exported bits, both counts and the changed box, exactly --
on the scenes of tests/test_world_stamp.py.  Then the patterns (create, capture, read, destroy, ids, lifetime),
and what the call promises around the bits: the whole state equals a twin that made the same change by
rv_world_edit x-runs and a twin that imported the restated world and built its CSDF, rv_world_edit_info reports
the call like the edit of the union box, a call that changes nothing touches nothing and a capture discards no
work computed ahead, persistence, detached voxels, the info sums, the status codes, and a seeded mixed session
against a host model."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import (generated, pack, rv, same_frames, same_tables, same_world, sun, synthetic_voxels,  # noqa: F401
                       tables, voxels, world)
import np_stamp as N
from test_gpu_world_detached import x_runs
from test_gpu_world_fall import _camera, _context
from test_world_stamp import CLEAR, COPY, FX, FZ, LGS, SET, SWAP, lg_of, rand_pattern, random_stamps, scenes, worlds

pytestmark = pytest.mark.gpu

W = H = 64
ZERO = N.ZERO


def upload(r, pats):
    return [r.pattern_create(p) for p in pats]


def mapped(ids, stamps):
    return [(ids[s[0]],) + tuple(s[1:]) for s in stamps]


def check(rv, r, vox, pats, ids, stamps, what=None):
    """The context (holding vox, and pats under ids) changes as the restatement and the host form do; returns the
    restatement's."""
    lg = lg_of(vox)
    want = N.apply(vox, pats, stamps)
    got = r.world_stamp(mapped(ids, stamps))
    assert got == want[1:] + (N.boxes(lg, pats, stamps)[1],), (what, got, want[1:])
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0])), (what, "bits")
    at = rv.stamp_at(lg, pack(vox), pats, stamps)
    assert at[1:] == want[1:] and np.array_equal(at[0], pack(want[0])), (what, "host form")
    return want


# ---------------------------------------------------------------- 1. device = restatement = host form
@pytest.mark.parametrize("lg", LGS)
def test_scenes(rv, lg):
    r = rv.StateRender(lg, W, H)
    try:
        for name, (pats, stamps) in scenes(lg).items():
            ids = upload(r, pats)
            assert ids == list(range(len(pats)))
            for wname, vox in worlds(lg).items():
                r.world_import(rv.RV_WORLD_BITS, pack(vox))
                want = check(rv, r, vox, pats, ids, stamps, (lg, name, wname))
                assert wname != "random" or want[1] + want[2] > 0, (lg, name)   # the scene did something
            for i in ids:
                r.pattern_destroy(i)
    finally:
        r.close()


@pytest.mark.parametrize("seed", range(3))
def test_random_lists(rv, seed):
    rng = np.random.default_rng(600 + seed)
    vox = rng.random((128, 32, 64)) < 0.5   # 64 x 32 x 128
    lg = lg_of(vox)
    pats = [rand_pattern(rng, int(rng.integers(1, 70)), int(rng.integers(1, 12)), int(rng.integers(1, 40))) for _ in range(4)]
    r = rv.StateRender(lg, W, H)
    try:
        ids = upload(r, pats)
        for n in (1, 3, 9):
            r.world_import(rv.RV_WORLD_BITS, pack(vox))
            check(rv, r, vox, pats, ids, random_stamps(rng, lg, pats, n, margin=3), (seed, n))
    finally:
        r.close()


# ---------------------------------------------------------------- 2. patterns
def test_create_reads_back_with_junk_zeroed(rv):
    L = rv._lib.load()
    rng = np.random.default_rng(71)
    r = rv.StateRender((5, 5, 5), W, H)   # no world: create, read and destroy need none
    try:
        for k, (nx, ny, nz) in enumerate([(1, 1, 1), (31, 3, 2), (32, 2, 3), (33, 3, 2), (37, 5, 4), (256, 2, 3), (3, 256, 2),
                                          (2, 3, 256)]):
            pat = rand_pattern(rng, nx, ny, nz)
            dims, words = rv.render.pattern_bits(pat)
            junk = words.copy()
            if nx % 32:
                junk[(nx - 1) // 32::(nx + 31) // 32] |= np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
            pid = C.c_int32(-1)
            assert L.rv_pattern_create(r._h, nx, ny, nz, junk.ctypes.data_as(C.c_void_p), junk.nbytes, C.byref(pid)) == 0
            assert pid.value == k
            d = (C.c_int32 * 3)()
            back = np.full(words.size, 0xA5A5A5A5, np.uint32)
            assert L.rv_pattern_read(r._h, k, d, back.ctypes.data_as(C.c_void_p), back.nbytes) == 0
            assert tuple(d) == (nx, ny, nz) and np.array_equal(back, words), (nx, ny, nz)
            assert np.array_equal(r.pattern_read(k), pat)
        assert r.world_stamp_info()[2] == 8
    finally:
        r.close()


@pytest.mark.parametrize("lg,boxes", [
    # x0 no multiple of 8; boxes across brick boundaries in x, y and z; one voxel; the whole world
    ((5, 5, 5), [(3, 2, 5, 29, 31, 30), (7, 3, 6, 9, 6, 10), (5, 0, 0, 32, 32, 32), (1, 1, 1, 2, 2, 2), (31, 31, 31, 32, 32, 32),
                 (0, 0, 0, 32, 32, 32)]),
    # rows of three pattern words, of 32 voxels from x0 = 7 (five brick words), and of the full 256
    ((9, 5, 5), [(13, 3, 9, 83, 30, 25), (7, 1, 2, 39, 5, 9), (3, 1, 2, 259, 31, 30), (255, 0, 0, 511, 32, 32), (256, 5, 5, 512, 6, 32)]),
])
def test_capture_equals_the_slice(rv, lg, boxes):
    X, Y, Z = (1 << l for l in lg)
    vox = np.random.default_rng(72).random((Z, Y, X)) < 0.5
    r = _context(rv, vox)
    try:
        for k, b in enumerate(boxes):
            pid = r.pattern_capture(b)
            assert pid == k
            assert np.array_equal(r.pattern_read(pid), vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]]), b
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(vox))
    finally:
        r.close()


def test_capture_then_copy_and_move(rv):
    lg = (6, 5, 6)
    vox = np.random.default_rng(73).random((64, 32, 64)) < 0.4
    r = _context(rv, vox)
    try:
        b = (5, 3, 9, 42, 17, 30)
        pat = vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]].copy()
        pid = r.pattern_capture(b)
        # pasted elsewhere, turned and mirrored: the transposed layout of a captured pattern
        for stamps in ([(0, COPY, 0, (20, 11, 31))], [(0, COPY, SWAP | FX, (33, 9, 3)), (0, SET, FZ, (-7, 20, 50))],
                       [(0, COPY, SWAP | FZ | FX, (1, -3, 13)), (0, CLEAR, SWAP, (40, 25, 40))]):
            vox = check(rv, r, vox, [pat], [pid], stamps, stamps)[0]
        r.pattern_destroy(pid)
        # world_move against its restatement: overlapping, apart, and partly out of the window
        for box, delta in (((10, 4, 10, 30, 20, 27), (3, 0, -2)), ((3, 1, 2, 20, 9, 12), (30, 15, 40)), ((40, 10, 40, 60, 30, 60), (9, 5, 9)),
                           ((8, 8, 8, 16, 16, 16), (0, 0, 0))):
            want = N.move(vox, box, delta)
            got = r.world_move(box, delta)
            to = tuple(box[a] + delta[a] for a in range(3)) + tuple(box[3 + a] + delta[a] for a in range(3))
            clip = tuple(max(v, 0) for v in to[:3]) + tuple(min(v, d) for v, d in zip(to[3:], (64, 32, 64)))
            union = tuple(min(box[a], clip[a]) for a in range(3)) + tuple(max(box[3 + a], clip[3 + a]) for a in range(3))
            assert got == want[1:] + (union,), (box, delta, got)
            assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0])), (box, delta)
            vox = want[0]
        assert r.world_stamp_info()[2] == 0   # world_move leaves no pattern behind
    finally:
        r.close()


def test_ids_are_lowest_free_and_the_slots_fill(rv):
    L, lib = rv._lib.load(), rv._lib
    vox = np.random.default_rng(74).random((32, 32, 32)) < 0.5
    r = _context(rv, vox)
    try:
        one = np.ones((2, 3, 4), bool)
        assert [r.pattern_create(one) for _ in range(4)] == [0, 1, 2, 3]
        r.pattern_destroy(1)
        r.pattern_destroy(2)
        assert r.pattern_capture((1, 1, 1, 5, 5, 5)) == 1 and r.pattern_create(one) == 2 and r.pattern_create(one) == 4
        r.pattern_destroy(0)
        # a stamp that names a destroyed id: RV_ERR_INVALID, the world untouched, even behind a good stamp
        before, info = world(rv, r), r.world_edit_info()
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_stamp([(1, COPY, 0, (3, 3, 3)), (0, COPY, 0, (9, 9, 9))])
        for x, y in zip(world(rv, r), before):
            assert np.array_equal(x, y)
        assert r.world_edit_info() == info
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.pattern_destroy(0)
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.pattern_read(0)
        assert r.pattern_create(one) == 0
        # all RV_PATTERN_MAX slots, then one more
        for k in range(5, lib.RV_PATTERN_MAX):
            assert r.pattern_create(one) == k
        live, nbytes = r.world_stamp_info()[2:]
        assert live == lib.RV_PATTERN_MAX and nbytes == 255 * 4 * 2 * 3 + 4 * 4 * 4   # 255 of 4 x 3 x 2, one capture of 4^3
        pid = C.c_int32(-7)
        dims, words = rv.render.pattern_bits(one)
        assert L.rv_pattern_create(r._h, 4, 3, 2, words.ctypes.data_as(C.c_void_p), words.nbytes, C.byref(pid)) == lib.RV_ERR_INVALID
        b = lib.rv_voxel_box(0, 0, 0, 4, 4, 4)
        assert L.rv_pattern_capture(r._h, C.byref(b), C.byref(pid)) == lib.RV_ERR_INVALID and pid.value == -7
        r.pattern_destroy(200)
        assert r.pattern_capture((0, 0, 0, 4, 4, 4)) == 200
        assert np.array_equal(r.pattern_read(200), vox[:4, :4, :4]) and np.array_equal(r.pattern_read(255), one)
    finally:
        r.close()


def test_patterns_survive_world_calls(rv, oracle):
    lg, origin = (6, 6, 6), (40, -24)
    rng = np.random.default_rng(75)
    pat = rand_pattern(rng, 37, 9, 11)
    r = rv.StateRender(lg, W, H, seed=origin)
    try:
        pid = r.pattern_create(pat)          # before any world
        r.world_build()
        cap = r.pattern_capture((3, 20, 5, 40, 44, 30))
        kept = r.pattern_read(cap)
        assert np.array_equal(kept, voxels(generated(oracle, lg, origin), lg)[5:30, 20:44, 3:40])
        r.world_edit([(0, 0, 0, 64, 64, 64, 0)])
        r.world_scroll(16, -8)
        vox = rng.random((64, 64, 64)) < 0.5
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.world_build()
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        assert np.array_equal(r.pattern_read(pid), pat) and np.array_equal(r.pattern_read(cap), kept)
        check(rv, r, vox, [pat, kept], [pid, cap], [(0, COPY, 5, (7, 3, 9)), (1, SET, 2, (30, 41, 50))], "after the world calls")
    finally:
        r.close()


# ---------------------------------------------------------------- 3. the whole state equals a twin
def _blocks(lg, seed):
    X, Y, Z = (1 << l for l in lg)
    return synthetic_voxels("blocks", X, Y, Z, np.random.default_rng(seed))


def _twin_patterns():
    rng = np.random.default_rng(81)
    return [rand_pattern(rng, 9, 8, 7, 0.4), np.ones((5, 4, 6), bool), rand_pattern(rng, 11, 5, 6, 0.5)]


# name -> (log2 dims, stamps, whether the whole-grid CSDF build runs).  The local rebuild needs an axis longer
# than 256 voxels: the rebuilt region is the union box grown by 64 coarse cells, and its input boxes by 128.
TWIN_SCENES = {
    # a tree set on the floor across the brick boundary x = 208, a pit cleared into the floor beside it, a copy
    "local": ((9, 5, 5), [(0, SET, SWAP | FX, (204, 2, 13)), (1, CLEAR, 0, (196, 0, 11)), (2, COPY, FZ, (213, 1, 20))], False),
    # the same through the wall x = 0 and at the top rows: the whole-grid build
    "whole": ((6, 6, 6), [(0, SET, 0, (-4, 2, 30)), (1, CLEAR, SWAP, (20, 0, 21)), (2, COPY, FX | FZ, (30, 1, 40)),
                          (0, SET, 7, (50, 59, 50))], True),
}


@pytest.mark.parametrize("name", list(TWIN_SCENES))
def test_scene_equals_the_twin(rv, atlas, name):
    lg, stamps, full = TWIN_SCENES[name]
    vox, pats = _blocks(lg, 7), _twin_patterns()
    r, t, u = _context(rv, vox, atlas), _context(rv, vox, atlas), None
    try:
        ids = upload(r, pats)
        cam, vp = _camera(rv, lg)
        r.gi_update(0)
        r.frame(cam, vp)
        info = r.world_edit_info()
        want = check(rv, r, vox, pats, ids, stamps, name)
        assert want[1] > 0 and want[2] > 0
        each, union = rv.stamp_box(lg, pats, stamps)
        assert (each, union) == N.boxes(lg, pats, stamps) and ZERO not in each
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


# ---------------------------------------------------------------- 4. around the bits
@pytest.mark.parametrize("mode,in_flight", [("seq", 2), ("group", 1)])
def test_nothing_changed_touches_nothing(rv, atlas, mode, in_flight):
    """A twin renders the same pipelined or grouped frames without the calls in between: captures, which are
    queries, and stamps that set solid voxels, clear air, copy a captured box back onto itself or lie outside the
    window.  They discard no work computed ahead -- the frames, the GI grid and rv_flow_info equal the twin's --
    and mark no column."""
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
        pick = lambda a, k: tuple(int(v) for v in a[(k * 7919) % len(a)][::-1])   # noqa: E731 -- [z, y, x] -> (x, y, z)
        dot = r.pattern_create(np.ones((1, 1, 1), bool))
        box = (9, 20, 13, 46, 50, 40)
        info, w0 = r.world_edit_info(), world(rv, r)
        for k0 in (0, n):
            cap = r.pattern_capture(box)
            idle = [(dot, CLEAR, k, pick(air, k)) for k in range(5)] + [(dot, SET, k, pick(rock, k)) for k in range(5)] + \
                [(cap, COPY, 0, box[:3]), (cap, COPY, 3, (-60, 5, 5)), (dot, SET, 0, (64, 3, 3))]
            assert r.world_stamp(idle)[:2] == (0, 0)
            for c in (r, t):
                c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
            again = r.pattern_capture(box)     # a capture between the calls of a pipelined loop
            assert np.array_equal(r.pattern_read(again), vox[box[2]:box[5], box[1]:box[4], box[0]:box[3]])
            assert r.world_stamp(idle[:3]) == (0, 0, N.boxes(lg, {dot: (1, 1, 1)}, idle[:3])[1])
            assert r.world_stamp([(cap, COPY, 3, (-60, 5, 5)), (dot, SET, 0, (64, 3, 3))]) == (0, 0, ZERO)   # all outside
            same_frames(rv, r, t, k0)
            r.pattern_destroy(cap)
            r.pattern_destroy(again)
        assert r.world_edit_info() == (info[0], 0, False) and t.world_edit_info() == info
        assert r.flow_info() == t.flow_info()
        assert r.world_persist_info()["dirty_columns"] == 0
        for a, b in zip(world(rv, r), w0):
            assert np.array_equal(a, b)
    finally:
        r.close()
        t.close()


def _columns(boxes):
    return {(bx, bz) for b in boxes if b != ZERO for bx in range(b[0] >> 3, ((b[3] - 1) >> 3) + 1)
            for bz in range(b[2] >> 3, ((b[5] - 1) >> 3) + 1)}


def _tree():
    """A 5 x 9 x 5 tree: a trunk of 5 voxels under a crown."""
    t = np.zeros((5, 9, 5), bool)
    t[2, :6, 2] = True
    t[:, 5:8, :] = True
    t[1:4, 8, 1:4] = True
    return t


def test_persistence_and_scrolling(rv, oracle):
    """The dirty columns are exactly those under the non-empty clipped boxes, stamp by stamp; a stamped tree that
    scrolls out and back is restored bit for bit."""
    lg, origin = (6, 6, 6), (40, -24)
    r = rv.StateRender(lg, W, H, seed=origin)
    try:
        r.world_build()
        bits = generated(oracle, lg, origin)
        vox = voxels(bits, lg)
        top = int(np.flatnonzero(vox[20, :, 12])[-1])   # the surface at (12, ., 20)
        # the first column, in (z, x) order, with room for a tree above its surface
        tops = np.where(vox.any(axis=1), 63 - np.argmax(vox[:, ::-1, :], axis=1), -1)   # [z, x]
        gz, gx = (int(v) for v in np.argwhere(tops + 10 <= 64)[0])
        ground = int(tops[gz, gx]) + 1
        pats = [_tree(), np.ones((3, 6, 7), bool)]
        ids = upload(r, pats)
        # a tree standing on that column, one outside the window, one through the wall z = 63 (inside the rock or
        # not), and a trench cleared into the ground across the brick border x = 40
        stamps = [(0, SET, 0, (gx - 2, ground, gz - 2)), (0, SET, 0, (-9, 30, 5)), (0, SET, SWAP, (30, 50, 61)),
                  (1, CLEAR, 0, (37, top - 3, 44))]
        r.world_persist(True)
        want = check(rv, r, vox, pats, ids, stamps, "trees")
        assert want[1] > 0 and want[2] > 0
        each, _ = N.boxes(lg, pats, stamps)
        assert each[1] == ZERO and len(_columns(each)) >= 5
        assert r.world_persist_info()["dirty_columns"] == len(_columns(each))
        r.world_persist_flush()
        keys = {(origin[0] + 8 * bx, origin[1] + 8 * bz) for bx, bz in _columns(each)}
        assert {tuple(k) for k in r.world_store_list().tolist()} == keys
        r.world_scroll(64, 0)    # every column leaves ...
        assert r.world_persist_info()["dirty_columns"] == 0
        r.world_scroll(-64, 0)   # ... and the stamped ones come back as they were left
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0]))
        assert r.world_persist_info()["dirty_columns"] == len(keys)
        assert np.array_equal(r.pattern_read(ids[0]), pats[0])
    finally:
        r.close()


def test_detached_finds_a_floating_stamp(rv):
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :4] = True
    r = _context(rv, vox)
    try:
        tree = _tree()
        pid = r.pattern_create(tree)
        want = check(rv, r, vox, [tree], [pid], [(0, SET, 0, (10, 4, 10)), (0, SET, FX | FZ, (20, 9, 18))], "two trees")
        assert want[1] == 2 * int(tree.sum())
        comps, n, v, _ = r.world_detached((4, 4, 4, 30, 30, 30))     # one stands on the floor, one hangs in the air
        assert n == 1 and v == int(tree.sum())
        assert comps[0]["lo"].tolist() == [20, 9, 18] and comps[0]["hi"].tolist() == [25, 18, 23]
    finally:
        r.close()


def test_info_sums(rv):
    vox = np.random.default_rng(91).random((32, 32, 32)) < 0.5
    r = _context(rv, vox)
    try:
        assert r.world_stamp_info() == (0, 0, 0, 0)
        a, b = r.pattern_create(np.ones((3, 2, 33), bool)), r.pattern_capture((0, 0, 0, 5, 6, 7))
        assert r.world_stamp_info() == (0, 0, 2, 4 * 2 * 2 * 3 + 4 * 1 * 6 * 7)
        r.world_stamp([])                                                     # n == 0: no call
        r.world_stamp([(a, SET, 0, (40, 0, 0))])                             # outside: no launch
        assert r.world_stamp_info()[:2] == (0, 0)
        r.world_stamp([(a, SET, 0, (3, 3, 3)), (b, COPY, 0, (-40, 0, 0)), (b, COPY, 1, (9, 9, 9))])
        r.world_stamp([(a, SET, 0, (3, 3, 3))])                              # changes nothing, but launched
        assert r.world_stamp_info() == (2, 3, 2, 4 * 2 * 2 * 3 + 4 * 1 * 6 * 7)
        r.pattern_destroy(a)
        assert r.world_stamp_info() == (2, 3, 1, 4 * 1 * 6 * 7)
    finally:
        r.close()


# ---------------------------------------------------------------- 5. a seeded mixed session
def _session_model(oracle, lg, origin):
    """The shaped-edit session model with the pattern and stamp calls, restated from the header."""
    from test_gpu_world_shapes import _session_model as shapes_model
    NS, base = shapes_model(oracle, lg, origin)

    class StampSession(type(base)):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.pats, self.stamp_calls, self.stamp_applied = {}, 0, 0

        def _slot(self):
            return min(set(range(N.MAX_PATTERNS)) - set(self.pats))

        def create(self, pat):
            self.last = self._slot()
            self.pats[self.last] = pat.copy()

        def capture(self, b):
            self.last = self._slot()
            self.pats[self.last] = self.vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]].copy()

        def pattern_destroy(self, pid):
            del self.pats[pid]

        def stamp(self, stamps):
            after, n_set, n_cleared = N.apply(self.vox, self.pats, stamps)
            each, union = N.boxes(self.lg, self.pats, stamps)
            self.last = (n_set, n_cleared, union)
            if union == ZERO:      # nothing launched: the record of the last call is zeroed all the same
                self.edit_cells, self.edit_full = 0, False
                return
            self.stamp_calls += 1
            self.stamp_applied += sum(b != ZERO for b in each)
            if n_set + n_cleared == 0:
                self.edit_cells, self.edit_full = 0, False
                return
            self.vox = after
            if self.persist_on:
                for b in each:
                    self._mark(sorted(_columns([b])))
            self._finish(union)

    return NS, StampSession(oracle, lg, origin, gi=False)


def _session_trace(NS, m, seed, n):
    """n calls drawn from the seed on a model of its own: stamps of created and captured patterns (trees on the
    surface, pastes through the faces, masked pastes, stamps outside), captures, destroys, box and shaped edits,
    scrolls along both axes, falls, persistence off and on, flushes."""
    from test_world_shapes import sphere
    rng = np.random.default_rng(seed)
    X, Y, Z = (1 << l for l in m.lg)
    trace, last = [("persist", 1), ("create", _tree()), ("create", np.ones((7, 9, 7), bool))], None
    for op in trace:
        m.apply(op)
    while len(trace) < n:
        k = rng.uniform()
        ids = sorted(m.pats)
        if k < 0.35:
            stamps = []
            for _ in range(int(rng.integers(1, 5))):
                x, z = int(rng.integers(-4, X)), int(rng.integers(-4, Z))
                col = m.vox[min(max(z + 2, 0), Z - 1), :, min(max(x + 2, 0), X - 1)]
                y = int(np.flatnonzero(col)[-1]) + 1 if col.any() and rng.uniform() < 0.7 else int(rng.integers(-3, Y))
                if rng.uniform() < 0.25:   # a masked paste
                    stamps += [(1, CLEAR, 0, (x, y, z)), (0, SET, int(rng.integers(0, 8)), (x + 1, y, z + 1))]
                else:
                    stamps.append((int(rng.choice(ids)), int(rng.integers(0, 3)), int(rng.integers(0, 8)), (x, y, z)))
            last = N.boxes(m.lg, m.pats, stamps)[1]
            op = ("stamp", tuple(stamps))
        elif k < 0.42:
            op = ("stamp", ((int(rng.choice(ids)), COPY, 1, (X + 3, 2, 2)), (0, SET, 0, (5, Y, 5))))   # outside
        elif k < 0.54 and len(ids) < 8:
            x0, y0, z0 = int(rng.integers(0, X - 1)), int(rng.integers(0, Y - 1)), int(rng.integers(0, Z - 1))
            op = ("capture", (x0, y0, z0, int(rng.integers(x0 + 1, min(X, x0 + 40) + 1)), int(rng.integers(y0 + 1, min(Y, y0 + 12) + 1)),
                              int(rng.integers(z0 + 1, min(Z, z0 + 20) + 1))))
        elif k < 0.60 and len(ids) > 2:
            op = ("pattern_destroy", int(rng.choice(ids[2:])))
        elif k < 0.68:
            op = ("edit", tuple(NS._small_box(rng, m, "any") for _ in range(int(rng.integers(1, 3)))))
        elif k < 0.74:
            c = (int(rng.integers(0, 2 * X)), int(rng.integers(20, 2 * Y)), int(rng.integers(0, 2 * Z)))
            op = ("shapes", (sphere(c, int(rng.integers(6, 16)), 0),))
        elif k < 0.86:
            d = 8 * int(rng.choice([-2, -1, 1, 2]))
            op = ("scroll", d, 0) if rng.uniform() < 0.6 else ("scroll", 0, d)
            last = None
        elif k < 0.93 and last is not None and last != ZERO:
            op = ("fall", tuple(max(last[a] - 1, 0) for a in range(3)) + tuple(min(last[3 + a] + 1, d) for a, d in
                                                                              zip(range(3), (X, Y, Z))))
        elif k < 0.97:
            op = ("persist", int(not m.persist_on))
        else:
            op = ("flush",)
        m.apply(op)
        trace.append(op)
    return trace + [("persist", 1), ("flush",)]


def test_mixed_session(rv, oracle, sun):
    import np_exits as EX
    from test_gpu_world_session import _same_store
    lg, origin, seed, n = (6, 5, 6), (40, -24), 18, 44
    NS, gen = _session_model(oracle, lg, origin)
    trace = _session_trace(NS, gen, seed, n)
    names = [op[0] for op in trace]
    assert len(trace) == n + 2 and min(names.count(k) for k in ("stamp", "capture", "edit", "shapes", "scroll", "fall")) >= 2, names
    _, m = _session_model(oracle, lg, origin)
    r = rv.StateRender(lg, W, H, seed=origin)
    changed = idle = 0
    try:
        r.world_build()
        for i, op in enumerate(trace):
            what = f"seed {seed}, call {i} {op[0]}"
            got = None
            if op[0] == "stamp":
                got = r.world_stamp(op[1])
            elif op[0] == "create":
                got = r.pattern_create(op[1])
            elif op[0] == "capture":
                got = r.pattern_capture(op[1])
            elif op[0] == "pattern_destroy":
                r.pattern_destroy(op[1])
            elif op[0] == "shapes":
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
            if got is not None:
                assert got == m.last, (what, got, m.last)
            if op[0] == "stamp":
                changed += sum(got[:2]) > 0
                idle += sum(got[:2]) == 0
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
            info = r.world_stamp_info()
            assert info[:3] == (m.stamp_calls, m.stamp_applied, len(m.pats)), (what, info)
            for pid, pat in m.pats.items():
                assert np.array_equal(r.pattern_read(pid), pat), (what, "pattern", pid)
        assert changed >= 5 and idle >= 1, (changed, idle)
        assert m.captured >= 1 and m.restored >= 1, (m.captured, m.restored)
    finally:
        r.close()


# ---------------------------------------------------------------- 6. status codes
def test_status_codes(rv):
    from rvgrt_amd.render import _stamps
    L, lib = rv._lib.load(), rv._lib
    r = rv.StateRender((5, 5, 5), W, H)
    a, b, ch = C.c_uint64(77), C.c_uint64(77), lib.rv_voxel_box(7, 7, 7, 7, 7, 7)
    pid = C.c_int32(-7)
    one = np.ones((4, 4, 4), bool)
    dims, words = rv.render.pattern_bits(one)
    wp = words.ctypes.data_as(C.c_void_p)

    def call(stamps, n=None):
        arr = _stamps(stamps) if stamps is not None else None
        return L.rv_world_stamp(r._h, arr, len(stamps) if n is None else n, C.byref(a), C.byref(b), C.byref(ch))

    def create(nx, ny, nz, p=wp, nbytes=words.nbytes, out=C.byref(pid)):
        return L.rv_pattern_create(r._h, nx, ny, nz, p, nbytes, out)
    try:
        # before a world: patterns can be made, read and destroyed; stamps and captures cannot run
        assert create(4, 4, 4) == lib.RV_OK and pid.value == 0
        good = (0, COPY, 0, (3, 3, 3))
        assert call([good]) == lib.RV_ERR_STATE
        box = lib.rv_voxel_box(1, 1, 1, 9, 9, 9)
        assert L.rv_pattern_capture(r._h, C.byref(box), C.byref(pid)) == lib.RV_ERR_STATE and pid.value == 0
        with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
            r.world_stamp([good])
        # rv_pattern_create / read / destroy
        pid.value = -7
        for nx, ny, nz in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (257, 1, 1), (1, 257, 1), (1, 1, 257), (-1, 4, 4)]:
            assert create(nx, ny, nz) == lib.RV_ERR_INVALID, (nx, ny, nz)
        assert create(4, 4, 4, nbytes=words.nbytes - 1) == lib.RV_ERR_INVALID
        assert create(33, 4, 4) == lib.RV_ERR_INVALID          # two words a row: bytes below the size
        assert create(4, 4, 4, p=None) == lib.RV_ERR_INVALID and create(4, 4, 4, out=None) == lib.RV_ERR_INVALID
        assert pid.value == -7 and r.world_stamp_info()[2:] == (1, 64)
        d = (C.c_int32 * 3)(9, 9, 9)
        back = np.zeros(words.size, np.uint32)
        bp = back.ctypes.data_as(C.c_void_p)
        for bad_id in (-1, 1, 255, 256):
            assert L.rv_pattern_read(r._h, bad_id, d, bp, back.nbytes) == lib.RV_ERR_INVALID
            assert L.rv_pattern_destroy(r._h, bad_id) == lib.RV_ERR_INVALID
        assert L.rv_pattern_read(r._h, 0, None, bp, back.nbytes) == lib.RV_ERR_INVALID
        assert L.rv_pattern_read(r._h, 0, d, bp, back.nbytes - 1) == lib.RV_ERR_INVALID
        assert tuple(d) == (9, 9, 9) and not back.any()
        assert L.rv_pattern_read(r._h, 0, d, None, 0) == lib.RV_OK and tuple(d) == (4, 4, 4)   # dims only
        # rv_world_stamp and rv_pattern_capture on a world
        vox = np.random.default_rng(2).random((32, 32, 32)) < 0.5
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
        r.world_persist(True)
        before, info = world(rv, r), r.world_edit_info()
        bad = [([good], -1), ([good] * (N.MAX_STAMPS + 1), None), (None, 1), ([good, (1, COPY, 0, (3, 3, 3))], None),
               ([good, (-1, COPY, 0, (3, 3, 3))], None), ([good, (256, COPY, 0, (3, 3, 3))], None),
               ([good, (0, 3, 0, (3, 3, 3))], None), ([good, (0, -1, 0, (3, 3, 3))], None),
               ([good, (0, SET, 8, (3, 3, 3))], None), ([good, (0, SET, -1, (3, 3, 3))], None),
               ([good, (0, SET, 0, (N.MAX_AT + 1, 3, 3))], None), ([good, (0, SET, 0, (3, -N.MAX_AT - 1, 3))], None),
               ([good, (0, SET, 0, (3, 3, N.MAX_AT + 1))], None)]
        for stamps, n in bad:
            assert call(stamps, n) == lib.RV_ERR_INVALID, (stamps and stamps[-1], n)
        for bx in [(0, 0, 0, 0, 4, 4), (4, 4, 4, 4, 9, 9), (-1, 0, 0, 4, 4, 4), (0, 0, 0, 33, 4, 4), (0, 30, 0, 4, 33, 4),
                   (5, 5, 5, 4, 9, 9)]:
            vb = lib.rv_voxel_box(*bx)
            assert L.rv_pattern_capture(r._h, C.byref(vb), C.byref(pid)) == lib.RV_ERR_INVALID, bx
        assert L.rv_pattern_capture(r._h, None, C.byref(pid)) == lib.RV_ERR_INVALID
        assert L.rv_pattern_capture(r._h, C.byref(box), None) == lib.RV_ERR_INVALID
        for x, y in zip(world(rv, r), before):
            assert np.array_equal(x, y)
        assert r.world_edit_info() == info and (a.value, b.value) == (77, 77) and ch.x1 == 7 and pid.value == -7
        assert r.world_persist_info()["dirty_columns"] == 0 and r.world_stamp_info() == (0, 0, 1, 64)
        # n == 0; NULL outs; the caps themselves
        assert call([], 0) == lib.RV_OK and call(None, 0) == lib.RV_OK and r.world_edit_info() == info
        assert (a.value, b.value, ch.x1) == (0, 0, 0)
        assert L.rv_world_stamp(r._h, _stamps([good]), 1, None, None, None) == lib.RV_OK
        assert r.world_edit_info()[0] == info[0] + 1
        edge = [(0, SET, 7, (N.MAX_AT, -N.MAX_AT, N.MAX_AT)), (0, SET, 0, (28, 28, 28))] * (N.MAX_STAMPS // 2)
        assert call(edge) == lib.RV_OK and a.value == int((~vox[28:32, 28:32, 28:32]).sum()) and b.value == 0
        assert (ch.x0, ch.y0, ch.z0, ch.x1, ch.y1, ch.z1) == (28, 28, 28, 32, 32, 32)
    finally:
        r.close()
