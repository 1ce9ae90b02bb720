"""Seeded random sessions of world calls -- rv_world_edit, rv_gi_relight, rv_world_scroll, the texture origin,
rv_world_persist and the store, rv_world_bodies_move -- strung together in an order nobody planned and
checked after every call against the host model of tests/np_session.py, which restates the window from
include/rvgrt.h and knows nothing of kept work, local rebuilds or scratch.  Frames are judged by a cold twin
context that keeps nothing, never makes a world call and is handed the model's world.  The seeds are those
tests/test_world_session.py proves to contain captures, restores, replaced entries and the rest.  Every
comparison is bit-exact; every assertion message carries the seed, the index of the call and the trace so
far, which np_session.replay and `_world_session` / `_frame_session` below run literally."""
import numpy as np
import pytest

from gpu_world import (dims, draw, gi, rv, run_ranks, same_frames, same_tables, shifted, sun, tables,  # noqa: F401
                       world)
import np_bodies as B
import np_exits as E
import np_session as S

pytestmark = pytest.mark.gpu

W, H = 160, 96


def _call(rv, r, op, lg):
    """One call of a trace on a context.  ("bodies", seed) and ("frames", k) belong to the caller."""
    name, a = op[0], op[1:]
    if name == "edit":
        r.world_edit(a[0])
    elif name == "scroll":
        r.world_scroll(*a)
    elif name == "flush":
        r.world_persist_flush()
    elif name == "build":
        r.world_build()
    elif name == "persist":
        r.world_persist(a[0])
    elif name == "store_put":
        r.world_store_put(a[0], a[1], S.put_column(lg, a[2]))
    elif name == "store_clear":
        r.world_store_clear()
    elif name == "texture_origin_set":
        r.texture_origin_set(*a)
    elif name == "texture_follow_scroll":
        r.texture_follow_scroll(a[0])
    elif name == "relight":
        r.gi_relight(a[0], a[1], a[2], init=a[3])
    elif name == "bad_put":       # a key no column can have: RV_ERR_INVALID, the store as it was
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_store_put(a[0], a[1], S.put_column(lg, 0))
    elif name == "bad_get":       # a key that is not in the store
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_store_get(*a)
    else:
        raise ValueError(op)


def _same_bodies(rv, r, m, seed, n, what):
    """rv_world_bodies_move in both edge modes against the numpy restatement on the model's voxels."""
    lo, size, delta = B.random_bodies(np.random.default_rng(seed), n, dims(m.lg))
    for mode in (0, B.OPEN_EDGES):
        got, want = r.bodies_move(lo, size, delta, mode), B.move(m.vox, lo, size, delta, mode)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "bodies lo", mode)
        assert np.array_equal(got[1], want[1]), (what, "bodies flags", mode)
    calls, bodies = m.bodies
    m.bodies = (calls + 2, bodies + 2 * n)


def _same_store(rv, r, m, what):
    assert r.world_persist_info() == m.persist_info(), (what, "persist info", r.world_persist_info(), m.persist_info())
    keys = m.store_list()
    assert [tuple(k) for k in r.world_store_list().tolist()] == keys, (what, "store list")
    for k in keys:
        assert np.array_equal(r.world_store_get(*k), m.store[k]), (what, "store entry", k)


def _check(rv, oracle, sun, r, m, rng, what):
    """Everything a context can report against the model."""
    lg = m.lg
    X, Y, Z = dims(lg)
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, m.bits()), (what, "bits")
    assert np.array_equal(csdf, m.csdf()), (what, "csdf")
    E.check_tables(E.reference(m.vox, sun), *tables(rv, r), (what, "tables"))
    assert np.array_equal(gi(rv, r), m.gi), (what, "gi")
    assert r.world_scroll_info() == m.scroll_info(), (what, "scroll info", r.world_scroll_info(), m.scroll_info())
    assert r.world_edit_info() == m.edit_info(), (what, "edit info", r.world_edit_info(), m.edit_info())
    assert r.gi_relight_info() == m.relights, (what, "relight info")
    _same_store(rv, r, m, what)
    assert r.texture_origin() == (m.tex, m.follow), (what, "texture origin", r.texture_origin())
    cols = [(int(rng.integers(X // 8)), int(rng.integers(Z // 8))) for _ in range(4)] + m.dirty_columns()
    for c, got in zip(cols, r.world_columns_read(cols)):
        assert np.array_equal(got, m.column_bits(*c)), (what, "column", c)
    pos = (rng.uniform(size=(300, 3)) * np.array([X, Y, Z])).astype(np.float32)
    pos[:100] = np.floor(pos[:100]) + np.float32(0.5)
    assert np.array_equal(r.texture_tiles(pos), rv.texture_tile_at(m.tex[0], m.tex[1], pos)), (what, "tiles")
    _same_bodies(rv, r, m, int(rng.integers(1 << 30)), 200, what)
    assert r.bodies_info() == m.bodies, (what, "bodies info")


def _label(seed, trace, i):
    return f"seed {seed}, call {i} {trace[i] if i >= 0 else 'none yet'}; the trace so far: {list(trace[:i + 1])!r}"


# ---------------------------------------------------------------- a. world sessions
def _world_session(rv, oracle, sun, atlas, lg, trace, seed=None):
    """The trace on a 64 x 64 context with no frames, everything checked after every call.  At ("build",) a
    fresh context first takes the model's store and then builds the same window at the model's origin."""
    r = rv.StateRender(lg, 64, 64, atlas=atlas, seed=S.ORIGIN)
    r.world_build()
    m = S.Session(oracle, lg, S.ORIGIN, atlas=atlas)
    rng = np.random.default_rng(17)
    _check(rv, oracle, sun, r, m, rng, _label(seed, trace, -1))
    for i, op in enumerate(trace):
        what = _label(seed, trace, i)
        fresh = None
        if op[0] == "build":
            fresh = rv.StateRender(lg, 64, 64, atlas=atlas, seed=m.origin)
            fresh.world_persist(m.persist_on)
            for k, v in m.store.items():
                fresh.world_store_put(k[0], k[1], v)
        if op[0] == "bodies":
            _same_bodies(rv, r, m, op[1], 200, what)
        else:
            _call(rv, r, op, lg)
        m.apply(op)
        _check(rv, oracle, sun, r, m, rng, what)
        if fresh is not None:
            fresh.world_build()
            bits, csdf = world(rv, fresh)
            assert np.array_equal(bits, m.bits()), (what, "loaded bits")
            assert np.array_equal(csdf, r.world_export(rv.RV_WORLD_CSDF)), (what, "loaded csdf")
            same_tables(tables(rv, fresh), tables(rv, r), (what, "loaded tables"))
            assert fresh.world_persist_info()["restored_total"] == m.restored_in_build, (what, "loaded restores")
            fresh.close()
    info = r.world_persist_info()
    r.close()
    return m, info


@pytest.mark.parametrize("lg,seed,n", S.WORLD_SESSIONS)
def test_world_session(rv, oracle, sun, atlas, lg, seed, n):
    trace = S.ops(seed, lg, n, oracle=oracle, ending=S.ENDING)
    m, info = _world_session(rv, oracle, sun, atlas, lg, trace, seed)
    # the context's own counters say that the session held what it was chosen for
    assert info["captured_total"] >= 1 and info["restored_total"] >= 1, (seed, info, trace)
    assert m.edits >= 1 and m.scrolls >= 1, (seed, m.edits, m.scrolls, trace)


@pytest.mark.parametrize("name", sorted(S.LITERAL_SESSIONS))
def test_literal_session(rv, oracle, sun, atlas, name):
    """The traces written out by hand in np_session.LITERAL_SESSIONS, replayed like the random ones."""
    trace = S.LITERAL_SESSIONS[name]
    m, info = _world_session(rv, oracle, sun, atlas, (7, 7, 7), trace, name)
    c = S.coverage(m)
    assert info["captured_total"] == m.captured >= 1 and info["restored_total"] == m.restored >= 1, (name, info, trace)
    if name == "put_of_a_dirty_column":
        assert c["put_overwritten"] == 2 and c["put_consumed"] == 1 and c["restore_after_reedit"] == 1, (name, c, trace)
    else:
        assert "persist_toggle" in S.kinds(m, trace) and m.relights[0] == 2, (name, trace)


# ---------------------------------------------------------------- b. frame sessions
def _frame_contexts(rv, atlas, lg, n):
    cs = [rv.StateRender(lg, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, gi_rays_per_frame=4096, seed=S.ORIGIN)
          for _ in range(n)]
    for c in cs:
        c.world_build()
        c.gi_update(0)
    return cs


def _cold(t):
    """A context that computes nothing ahead and keeps nothing."""
    t.set_flow(0)
    t.set_gi_async(0)
    t.set_pipeline(0)


def _feed(rv, t, m):
    """The model's world into the twin."""
    t.world_import(rv.RV_WORLD_BITS, m.bits())
    t.world_import(rv.RV_WORLD_CSDF, m.csdf())
    t.world_import(rv.RV_WORLD_GI, m.gi)
    t.texture_origin_set(*m.tex)


def _world_call(rv, rs, t, m, op, what):
    """One world call on every subject and on the model; the subjects' bits, store and GI grid against the
    model's; then the twin is fed.  A relight under a texture origin other than (0, 0), which the oracle
    cannot sample, is made by the fed twin instead and the model takes the twin's grid."""
    lg = m.lg
    for r in rs:
        if op[0] == "bodies":
            _same_bodies(rv, r, m, op[1], 200, what)
        else:
            _call(rv, r, op, lg)
    by_twin = op[0] == "relight" and m.tex != (0, 0)
    if by_twin:
        t.gi_relight(op[1], op[2], op[3], init=op[4])
        m.gi = gi(rv, t).copy()
        m.count_relight(op[1], op[3])
        m.calls += 1
    else:
        m.apply(op)
    for q, r in enumerate(rs):
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), m.bits()), (what, "bits", q)
        assert np.array_equal(gi(rv, r), m.gi), (what, "gi", q)
        assert r.world_scroll_info()[3] == m.origin and r.texture_origin() == (m.tex, m.follow), (what, "origins", q)
        assert r.gi_relight_info() == m.relights, (what, "relight info", q)
        _same_store(rv, r, m, (what, q))
    if not by_twin and op[0] not in ("bodies", "flush", "store_put", "persist"):
        _feed(rv, t, m)


def _frame_session(rv, oracle, atlas, mode, in_flight, trace, seed, anchored):
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, flags = (7, 7, 7), rv.RV_FLAGS_REFERENCE
    nframes = sum(op[1] for op in trace if op[0] == "frames")
    seq = camera_path(TEST_POSES_128["P0"], W, H, nframes + 1, pan=0.01, ref_compat=True)
    r, t = _frame_contexts(rv, atlas, lg, 2)
    _cold(t)
    if in_flight > 1:
        for c in (r, t):
            c.set_frames_in_flight(in_flight)
    if mode == "group":
        r.set_frame_group(2)
        assert r.frame_group_effective() == 2
    m = S.Session(oracle, lg, S.ORIGIN, atlas=atlas)
    m.gi = gi(rv, t).copy()
    if anchored:    # textures anchored to the terrain for good, as the header recommends
        for c in (r, t, m):
            c.texture_origin_set(*S.ORIGIN)
        r.texture_follow_scroll(1)
        m.texture_follow_scroll(1)
    k, shift, world_calls = 0, [0, 0], 0
    for i, op in enumerate(trace):
        what = (mode, _label(seed, trace, i))
        if op[0] != "frames":
            _world_call(rv, [r], t, m, op, what)
            world_calls += 1
            if op[0] == "scroll":
                shift = [shift[0] + op[1], shift[1] + op[2]]
            continue
        descs = [shifted(rv, d, *shift) for d in seq[k:k + op[1] + 1]]
        k += op[1]
        for c in (r, t):
            if mode == "draw":
                for d in descs[:-1]:
                    c.update_gi_data()
                    draw(c, d)
            else:   # the subject keeps the next frame's pre-pass and update: the next world call meets them
                c.render_frame_seq(descs[:-1], next_desc=descs[-1], flags=flags, gi_per_frame=True)
        same_frames(rv, r, t, what)
        m.gi = gi(rv, t).copy()
        assert r.flow_info()[2] == 0, what
    end = (mode, _label(seed, trace, len(trace) - 1))
    assert world_calls >= 4 and k == nframes, (end, world_calls, k)
    if mode == "draw":      # the flow path ran
        assert r.flow_info()[0] and r.flow_info()[1] == nframes and not t.flow_info()[0], (end, r.flow_info())
    r.close()
    t.close()
    return m


@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("mode,in_flight", [("draw", 1), ("seq", 2), ("group", 1)])
def test_frame_session(rv, oracle, atlas, mode, in_flight, anchored):
    """One or two frames between world calls, the subject with its mode's work computed ahead (a flow frame's
    speculated update; the pipelined or grouped loop's kept pre-pass and update), the twin cold.  The world
    calls are judged by the model, the frames by the twin.  With anchored, following textures the texture
    origin is never (0, 0) and the oracle cannot restate a relight, so the fed twin makes the same
    rv_gi_relight call: that checks that the call is ordered after the frames and discards the kept work,
    not the relight's arithmetic, which test_gpu_gi_relight.py and test_gpu_tex_anchor.py own."""
    seed, n = S.FRAME_SESSIONS[anchored]
    trace = S.ops(seed, (7, 7, 7), n, S.ANCHORED_MIX if anchored else S.FRAME_MIX, oracle=oracle, frames=True,
                  purpose=0.5)
    m = _frame_session(rv, oracle, atlas, mode, in_flight, trace, seed, anchored)
    assert m.scrolls >= 1 and m.edits >= 1 and m.relights[0] >= 1, (seed, trace)
    assert (m.tex != (0, 0)) == anchored, (seed, m.tex, trace)


# ---------------------------------------------------------------- c. a two-rank session
@pytest.mark.parametrize("group", [0, 2])
def test_two_rank_session(rv, oracle, atlas, group):
    """Two loopback ranks with persistence on make every call, store_put included; rank 0's gathered frame
    and every rank's GI grid equal the cold twin's, every rank's bits, persist info and store the model's."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, flags, N = (7, 7, 7), rv.RV_FLAGS_REFERENCE, 2
    seed, n = S.RANK_SESSION
    trace = S.ops(seed, lg, n, S.FRAME_MIX, oracle=oracle, frames=True, purpose=0.5)
    nframes = sum(op[1] for op in trace if op[0] == "frames")
    seq = camera_path(TEST_POSES_128["P0"], W, H, nframes + 1, pan=0.02, ref_compat=True)
    *rs, t = _frame_contexts(rv, atlas, lg, N + 1)
    _cold(t)
    loop = rv.LoopbackGroup(N, timeout_ms=60000)
    comms = []
    for q, c in enumerate(rs):
        c.set_tile_shard(32, q, N)
        if group:
            c.set_frame_group(group)
        comms.append(rv.Comm.loopback(c, loop, q))
    m = S.Session(oracle, lg, S.ORIGIN, atlas=atlas)
    m.gi = gi(rv, t).copy()
    k, shift = 0, [0, 0]
    for i, op in enumerate(trace):
        what = (group, _label(seed, trace, i))
        if op[0] != "frames":
            _world_call(rv, rs, t, m, op, what)
            if op[0] == "scroll":
                shift = [shift[0] + op[1], shift[1] + op[2]]
            continue
        descs = [shifted(rv, d, *shift) for d in seq[k:k + op[1] + 1]]
        k += op[1]
        run_ranks([lambda q=q: rs[q].render_frame_seq(descs[:-1], next_desc=descs[-1], flags=flags, gi_per_frame=True,
                                                      comm=comms[q]) for q in range(N)])
        for c in comms:
            c.wait(60000)
        for d in descs[:-1]:
            t.update_gi_data()
            t.frame(d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp), time=d.time,
                    jx=d.jitter_x, jy=d.jitter_y, flags=flags)
        assert np.array_equal(rs[0].readback(rv.RV_IMAGE_COLOR), t.readback(rv.RV_IMAGE_COLOR)), (what, "colour")
        m.gi = gi(rv, t).copy()
        for q, c in enumerate(rs):
            assert np.array_equal(gi(rv, c), m.gi), (what, "gi", q)
    assert m.captured >= 1 and m.restored >= 1 and m.relights[0] >= 1, (seed, trace)
    for c in comms:
        c.close()
    for c in rs + [t]:
        c.close()
    loop.close()
