"""The host model of tests/np_session.py against the yardsticks the project already has, and the sessions
that tests/test_gpu_world_session.py replays: every committed seed must contain, in the model's trace
alone, the things the GPU sessions exist to meet.  No GPU."""
import numpy as np
import pytest

from gpu_world import dims, generated, rv, step  # noqa: F401
import np_session as S
import np_world as R

LG = (7, 7, 7)


def _model(oracle, lg=LG, persist=True):
    m = S.Session(oracle, lg, R.ORIGIN, gi=False)
    m.persist(persist)
    return m


def _boxes(bx, bz, variant=0):
    """Two edits inside brick column (bx, bz) of a world 128 high (those of test_gpu_world_persist.py)."""
    x, z = 8 * bx, 8 * bz
    if variant == 0:
        return ((x + 1, 90, z + 1, x + 7, 126, z + 7, 1), (x + 2, 0, z + 2, x + 6, 100, z + 6, 0))
    return ((x, 60, z, x + 8, 80, z + 8, 1), (x + 3, 0, z + 1, x + 5, 128, z + 4, 0))


# ---------------------------------------------------------------- the model against the yardsticks
@pytest.mark.parametrize("lg,axis,d", [((9, 7, 7), 0, 8), ((9, 7, 7), 0, -40), ((9, 7, 7), 2, 24), ((7, 7, 9), 2, -64),
                                       ((7, 7, 9), 0, 16), ((7, 7, 7), 0, -128), ((7, 7, 7), 2, 136)])
def test_one_axis_scroll_is_np_world_scrolled(rv, oracle, lg, axis, d):
    m = _model(oracle, lg)
    m.edit(_boxes(1, 5))                       # retained or not, an edited column is no generator's
    old = m.bits()
    m.persist(0)
    m.scroll(*step(axis, d))
    if abs(d) < dims(lg)[axis]:
        assert np.array_equal(m.bits(), R.scrolled(oracle, lg, axis, d, old)[0])
    else:
        assert np.array_equal(m.bits(), generated(oracle, lg, m.origin))
    plan = rv.scroll_region(lg, axis, d)
    assert m.scroll_info() == (1, plan[2], plan[3], (R.ORIGIN[0] + step(axis, d)[0], R.ORIGIN[1] + step(axis, d)[1]))
    assert m.steps == [(axis, d, plan[3])]


def test_scrolls_compose_and_undo(oracle):
    a, b = _model(oracle, persist=False), _model(oracle, persist=False)
    a.scroll(8, 0)
    a.scroll(16, 0)
    b.scroll(24, 0)
    assert np.array_equal(a.bits(), b.bits()) and a.origin == b.origin
    home = generated(oracle, LG, R.ORIGIN)
    for d in ((8, -16), (-64, 0), (0, 136)):
        b = _model(oracle, persist=False)
        b.scroll(*d)
        b.scroll(-d[0], -d[1])
        assert np.array_equal(b.bits(), home) and b.origin == R.ORIGIN
    info = b.scroll_info()
    b.scroll(0, 0)
    assert b.scroll_info() == info


def test_gi_moves_with_the_window(oracle, atlas):
    """Retained cells keep their value at the new index; entering cells are gi_init's in the new world."""
    m = S.Session(oracle, LG, R.ORIGIN, atlas=atlas)
    G = 32
    before = m.gi.reshape(G, G, G).copy()
    before[:, :, :] += np.arange(G, dtype=np.uint32)[None, None, :]      # tell the cells apart
    m.gi = before.ravel().copy()
    m.scroll(16, 0)
    after = m.gi.reshape(G, G, G)
    assert np.array_equal(after[:, :, :G - 4], before[:, :, 4:])
    ow = oracle.OracleWorld(*LG, atlas=atlas, ox=m.origin[0], oz=m.origin[1]).build(gi_sweeps=0)
    assert np.array_equal(after[:, :, G - 4:], ow.gi.view(np.uint32).reshape(G, G, G)[:, :, G - 4:])
    m.edit(_boxes(3, 3))
    assert np.array_equal(m.gi, after.ravel())                             # edits leave the grid alone


@pytest.mark.parametrize("on", [True, False])
def test_an_edited_column_survives_only_with_persistence(oracle, on):
    m = _model(oracle, persist=on)
    m.edit(_boxes(1, 5))
    edited = m.bits()
    assert not np.array_equal(edited, generated(oracle, LG, R.ORIGIN))
    assert m.persist_info()["dirty_columns"] == (1 if on else 0)
    m.scroll(16, 0)
    assert m.store_list() == ([(R.ORIGIN[0] + 8, R.ORIGIN[1] + 40)] if on else [])
    m.scroll(-16, 0)
    assert np.array_equal(m.bits(), edited if on else generated(oracle, LG, R.ORIGIN))
    want = {"on": on, "dirty_columns": int(on), "stored_columns": 0, "stored_bytes": 0, "captured_total": int(on),
            "restored_total": int(on)}
    assert m.persist_info() == want


def test_newer_wins_flush_keeps_dirty_and_the_list_is_sorted(oracle):
    m = _model(oracle)
    m.edit(_boxes(1, 5))
    m.flush()
    key = m.key(1, 5)
    first = m.store_get(*key).copy()
    assert m.persist_info()["dirty_columns"] == 1 and m.captured == 1          # a flush leaves the column dirty
    m.edit(_boxes(1, 5, variant=1))
    second = m.column_bits(1, 5).copy()
    assert not np.array_equal(first, second)
    m.scroll(16, 0)                                                             # the newer copy replaces the entry
    assert np.array_equal(m.store_get(*key), second) and m.captured == 2 and not m.dirty
    assert [e[1] for e in m.log].count("replaced") == 1
    m.scroll(-16, 0)
    assert np.array_equal(m.column_bits(1, 5), second) and m.restored == 1 and m.dirty == {key}
    # a box that changes nothing marks nothing and does not count
    edits = m.edits
    m.edit(((64, 0, 64, 65, 1, 65, int(m.vox[64, 0, 64])),))
    assert m.edits == edits and m.dirty == {key} and m.edit_info()[1:] == (0, False)
    # (wz, wx) order, negative keys included
    for wx, wz in ((48, -32), (-16, 8), (8, -32), (40, 8)):
        m.store_put(wx, wz, S.put_column(LG, wx + wz))
    assert m.store_list() == [(8, -32), (48, -32), (-16, 8), (40, 8)]
    with pytest.raises(ValueError):
        m.store_put(41, 8, S.put_column(LG, 0))
    with pytest.raises(ValueError):
        m.store_get(0, 0)
    m.store_clear()
    assert not m.store and not m.dirty


def test_store_put_is_used_or_replaced(oracle):
    """A put of a key outside the window is used when its column enters; one of a clean column of the window
    when the column comes back; one of a dirty column is replaced when the column leaves."""
    m = _model(oracle)
    out, clean, dirty = m.key(16, 3), m.key(0, 3), m.key(0, 9)
    m.edit(_boxes(0, 9))
    edited = m.column_bits(0, 9).copy()
    for k, key in enumerate((out, clean, dirty)):
        m.store_put(key[0], key[1], S.put_column(LG, k))
    m.scroll(8, 0)
    assert np.array_equal(m.column_bits(15, 3), S.put_column(LG, 0))            # entered with the stored bits
    assert clean in m.store and not np.array_equal(m.store[dirty], S.put_column(LG, 2))
    m.scroll(-8, 0)
    assert np.array_equal(m.column_bits(0, 3), S.put_column(LG, 1))
    assert np.array_equal(m.column_bits(0, 9), edited) and m.restored == 3
    c = S.coverage(m)
    assert c["put_consumed"] == 2 and c["put_overwritten"] == 1 and c["replaced"] == 1
    # build: the dirty set is cleared, then every stored key in the window is restored
    m.flush()
    assert set(m.store) == {out, clean, dirty}     # the first went out again, dirty, with the scroll back
    m.build()
    assert m.dirty == {clean, dirty} and set(m.store) == {out} and m.restored_in_build == 2
    assert np.array_equal(m.column_bits(0, 3), S.put_column(LG, 1))


def test_import_marks_every_column(oracle):
    m = _model(oracle)
    m.import_bits(generated(oracle, LG, (0, 0)))
    assert len(m.dirty) == 256 and np.array_equal(m.bits(), generated(oracle, LG, (0, 0)))


def test_texture_origin_follows(oracle):
    m = _model(oracle)
    m.texture_origin_set(*R.ORIGIN)
    m.scroll(8, -16)
    assert m.tex == R.ORIGIN
    m.texture_follow_scroll(1)
    m.scroll(8, -16)
    assert (m.tex, m.follow) == ((R.ORIGIN[0] + 8, R.ORIGIN[1] - 16), True)


@pytest.mark.parametrize("lg", [(9, 7, 7), (7, 7, 9), (7, 7, 7)])
def test_regions_and_boxes_are_the_abis(rv, oracle, lg):
    """edit_region, the whole-grid rule and relight_box of the model against the host-only ABI functions,
    over the boxes the generator makes."""
    X, Y, Z = dims(lg)
    S3 = (X // 2, Y // 2, Z // 2)
    seen = set()
    for seed in range(3):
        for op in S.ops(900 + seed, lg, 12, {"scroll": 5}, oracle=oracle):
            if op[0] == "edit":
                region, cells = rv.edit_region(lg, op[1])
                assert S.edit_region(lg, op[1]) == (region, cells)
                seen.add(region == (0, S3[0], 0, S3[1], 0, S3[2]))
                for margin in (0, 1, 3):
                    assert S.relight_box(lg, op[1], margin) == rv.relight_box(lg, op[1], margin)
    assert seen == ({True} if lg == (7, 7, 7) else {True, False})


# ---------------------------------------------------------------- the generator and the committed seeds
def test_a_trace_is_its_seed_and_replays(oracle):
    a = S.ops(7, LG, 16, oracle=oracle, ending=S.ENDING)
    assert a == S.ops(7, LG, 16, oracle=oracle, ending=S.ENDING) and len(a) == 16
    assert a[0] == ("persist", 1) and tuple(a[-2:]) == S.ENDING
    assert a != S.ops(8, LG, 16, oracle=oracle, ending=S.ENDING)
    assert eval(repr(a)) == a                                  # plain tuples: a failure's message can be replayed
    m, n = S.replay(oracle, LG, a, gi=False), S.replay(oracle, LG, a, gi=False)
    assert np.array_equal(m.bits(), n.bits()) and m.persist_info() == n.persist_info() and m.calls == 16


NEEDS = ("capture", "restore", "restore_after_reedit", "replaced", "noop_edit", "diagonal", "emptied", "put_consumed",
         "put_overwritten")


@pytest.mark.parametrize("lg,seed,n", S.WORLD_SESSIONS)
def test_world_sessions_hold_what_they_are_for(rv, oracle, lg, seed, n):
    assert 12 <= n <= 16
    trace = S.ops(seed, lg, n, oracle=oracle, ending=S.ENDING)
    m = S.replay(oracle, lg, trace, gi=False)
    c = S.coverage(m)
    for need in NEEDS:
        assert c[need] >= 1, (seed, need, trace)
    for axis, d, full in m.steps:
        assert rv.scroll_region(lg, axis, d)[3] == full, (seed, axis, d)
    if lg == (7, 7, 7):        # everything takes the whole-grid path
        assert c["edit_local"] == c["step_local"] == 0 and c["edit_full"] >= 1 and c["step_full"] >= 1
    else:
        for need in ("edit_local", "edit_full", "step_local", "step_full"):
            assert c[need] >= 1, (seed, need, trace)
    names = {op[0] for op in trace}
    assert {"edit", "scroll", "store_put", "flush", "build", "persist"} <= names, (seed, names)


def test_the_shapes_are_covered():
    shapes = [s[0] for s in S.WORLD_SESSIONS]
    for lg in ((9, 7, 7), (7, 7, 9), (7, 7, 7)):
        assert 2 <= shapes.count(lg) <= 3
    assert len(set(S.WORLD_SESSIONS)) == len(S.WORLD_SESSIONS)


def test_every_call_of_the_mix_is_replayed(oracle):
    """The world sessions that the GPU file replays -- the committed seeds and the literal traces, each checked
    in full after every call -- hold together every call of MIX: persistence off, a world call without it and
    on again, both invalid store calls, and a relight with and without INIT among them."""
    met = set()
    for lg, seed, n in S.WORLD_SESSIONS:
        trace = S.ops(seed, lg, n, oracle=oracle, ending=S.ENDING)
        met |= S.kinds(S.replay(oracle, lg, trace, gi=False), trace)
    for trace in S.LITERAL_SESSIONS.values():
        met |= S.kinds(S.replay(oracle, LG, trace, gi=False), trace)
    assert met == set(S.MIX) | {"relight_init"}, sorted((set(S.MIX) | {"relight_init"}) ^ met)


def test_literal_persist_off_and_on(oracle):
    """What the trace is for happens in the model: with persistence off an edit marks nothing and a scroll
    captures nothing and clears nothing; the key of the column that left is still dirty when persistence is on
    again, over its regenerated terrain; the build after store_clear forgets the edit made without it."""
    trace = S.LITERAL_SESSIONS["persist_off_and_on"]
    on = trace.index(("persist", 1), 1)
    m = S.replay(oracle, LG, trace[:on + 1], gi=False)
    assert m.edits == 2 and m.dirty == {(40, -8)} and not m.store and m.captured == 0 and m.column_of((40, -8)) is None
    m = S.replay(oracle, LG, trace[:on + 2], gi=False)              # home again
    assert np.array_equal(m.column_bits(0, 2), R.column_bits(R.terrain(oracle, LG, *R.ORIGIN), 0, 2))
    assert not np.array_equal(m.bits(), generated(oracle, LG, R.ORIGIN)) and m.persist_info()["dirty_columns"] == 1
    m = S.replay(oracle, LG, trace, gi=False)
    assert (m.captured, m.restored, m.restored_in_build) == (2, 1, 0) and m.relights == (2, 1280, 1920)
    assert np.array_equal(m.bits(), generated(oracle, LG, R.ORIGIN)) and not m.dirty and not m.store


def _frame_trace(oracle, anchored):
    seed, n = S.FRAME_SESSIONS[anchored]
    return S.ops(seed, LG, n, S.ANCHORED_MIX if anchored else S.FRAME_MIX, oracle=oracle, frames=True, purpose=0.5)


@pytest.mark.parametrize("anchored", [False, True])
def test_frame_sessions_hold_what_they_are_for(oracle, anchored):
    trace = _frame_trace(oracle, anchored)
    calls = [op for op in trace if op[0] != "frames"]
    assert all(b[0] == "frames" and b[1] in (1, 2) for a, b in zip(trace, trace[1:]) if a[0] != "frames")
    m = S.Session(oracle, LG, S.ORIGIN, gi=False)
    if anchored:
        m.texture_origin_set(*S.ORIGIN)
        m.texture_follow_scroll(1)
    for op in trace:
        m.apply(op)
    names = [op[0] for op in calls]
    assert {"edit", "scroll", "relight"} <= set(names) and len(calls) >= 5, names
    assert (m.tex == (0, 0)) != anchored
    assert m.captured >= 1
    # a call that only reads or only touches the host falls between two frames
    assert {"bodies", "flush", "store_put"} & set(names), names


def test_rank_session_holds_what_it_is_for(oracle):
    seed, n = S.RANK_SESSION
    trace = S.ops(seed, LG, n, S.FRAME_MIX, oracle=oracle, frames=True, purpose=0.5)
    m = S.replay(oracle, LG, trace, gi=False)
    names = [op[0] for op in trace]
    assert m.captured >= 1 and m.restored >= 1 and "store_put" in names
    assert "relight" in names[names.index("scroll"):]              # a relight after a scroll
