"""The texture origin on the GPU (rv_texture_origin_set, rv_texture_follow_scroll,
rv_texture_tiles): sampleTexture's lattice points shifted by an integer origin
that can follow rv_world_scroll, so that block textures stay anchored to the
terrain.  The yardsticks are rv_texture_tile_at (the kernels' function on the
CPU, itself pinned by tests/test_tex_anchor.py against numpy), whole frames and
GI updates of tests/np_shade.py with the anchored tile of tests/np_tex_anchor.py
patched in (ray cast: the oracle's), and twin contexts created at the scrolled
seed that compute nothing ahead.  Every comparison is bit-exact."""
import numpy as np
import pytest

from gpu_world import ctx128, dims, draw, gi, images, run_ranks, rv, same_frames, shifted
import np_shade as S
import np_tex_anchor as A

pytestmark = pytest.mark.gpu

W, H = 96, 64
ORIGIN = (40, -16)


def _table_positions(r):
    """Every voxel centre of the table's rows and of the 8 rows above them (clipped to the world)."""
    active, nbytes = r.tex_table_info()
    X, Y, Z = r.dims
    ny = nbytes // (4 * X * Z) if active else 0
    return A.voxel_centres(r.dims, min(Y, ny + 8)), ny


def _outside(dims, n, seed):
    """Positions outside the world, on every side of it (and above and below)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 2.0, (4 * n, 3)) * np.array(dims)
    out = ((p < 0) | (p >= np.array(dims))).any(axis=1)
    return p[out][:n].astype(np.float32)


# ---------------------------------------------------------------- 1. tiles, both paths
@pytest.mark.parametrize("table", [1, -1])
def test_tiles_table_and_noise(rv, table):
    lg = (7, 7, 7)
    r = rv.StateRender(lg, 64, 64, tex_table=table)
    # solid rows 0..40: sky exit 42, so the table covers rows 0..47 and the rows above it take the noise
    vox = np.zeros((128, 128, 128), bool)                  # (z, y, x)
    vox[:, :41, :] = True
    r.world_import(rv.RV_WORLD_BITS, np.packbits(vox.ravel(), bitorder="little").view(np.uint32))
    info = r.tex_table_info()
    assert info == ((True, 128 * 48 * 128 * 4) if table == 1 else (False, 0))
    pos = np.concatenate([A.voxel_centres(r.dims, 48 + 8), _outside(r.dims, 2000, 3)])
    assert r.texture_origin() == ((0, 0), False)
    base = None
    for origin in [(0, 0), (40, -16), (123464, -98760)]:
        r.texture_origin_set(*origin)
        assert r.texture_origin() == (origin, False)
        got = r.texture_tiles(pos)
        want = rv.texture_tile_at(origin[0], origin[1], pos)
        assert np.array_equal(got, want), (table, origin, int((got != want).sum()))
        assert r.tex_table_info() == info
        if base is None:
            base = got
        else:
            assert (got != base).mean() > 0.3             # another origin, other tiles
    r.close()


# ---------------------------------------------------------------- 2. frames and GI against numpy
def _np_world(ow):
    return {"dims": (ow.X, ow.Y, ow.Z), "csdf": ow.csdf, "gi": ow.gi.reshape(-1, 4), "solid": ow.voxels()}


def _np_trace(ow):
    return lambda org, d, dist: ow.trace_batch(np.ascontiguousarray(org, np.float32),
                                               np.ascontiguousarray(d, np.float32),
                                               np.ascontiguousarray(dist, np.float32))


_EXPECTED = {}


def _world128(oracle, atlas):
    """The 128^3 world after one GI sweep, this module's own (the session's shared one is updated in place by
    tests/test_gpu_parity.py) and never modified."""
    if "world" not in _EXPECTED:
        _EXPECTED["world"] = oracle.OracleWorld(7, 7, 7, atlas=atlas).build(gi_sweeps=1)
    return _EXPECTED["world"]


def _expected_frame(rv, oracle, atlas, pose):
    """np_shade's frame of the 128^3 world (one GI sweep at origin (0, 0)) at texture origin ORIGIN."""
    if pose not in _EXPECTED:
        from rvgrt_amd.configs import TEST_POSES_128
        ow = _world128(oracle, atlas)
        pos, yaw, pitch = TEST_POSES_128[pose]
        cam, vp = rv.camera_from_pose(pos, yaw, pitch, W, H)
        _, pvp = rv.camera_from_pose((pos[0] + 1.5, pos[1], pos[2] - 1.0), yaw + 0.03, pitch, W, H)
        with A.anchored(ORIGIN):
            want = S.render(_np_trace(ow), _np_world(ow), dict(rv.camera_dict(cam, vp), pvp=pvp), W, H,
                            S.F_PREPASS | S.F_WATER | S.F_GI, time=0.37, atlas=atlas)
        _EXPECTED[pose] = (cam, vp, pvp, want)
    return _EXPECTED[pose]


@pytest.mark.parametrize("table", [1, -1])
@pytest.mark.parametrize("pose", ["P0", "P1"])
def test_frames_equal_numpy(rv, oracle, atlas, pose, table):
    cam, vp, pvp, want = _expected_frame(rv, oracle, atlas, pose)
    flags = rv.RV_FLAGS_REFERENCE
    r = rv.StateRender((7, 7, 7), W, H, flags=flags, atlas=atlas, tex_table=table)
    r.world_build()
    r.gi_update(0)
    r.frame(cam, vp, prev_vp=pvp, time=0.37, flags=flags)
    color0, mv0, depth0 = images(rv, r)
    r.texture_origin_set(*ORIGIN)
    r.frame(cam, vp, prev_vp=pvp, time=0.37, flags=flags)
    color, mv, depth = images(rv, r)
    bad = np.any(color != want["rgba"], axis=-1)
    assert not bad.any(), f"{bad.sum()} pixels differ, first at {np.argwhere(bad)[:5].tolist()}"
    assert np.array_equal(mv, want["mv"]) and (mv != 0).any()
    assert np.array_equal(depth, want["depth"])
    assert np.array_equal(mv, mv0) and np.array_equal(depth, depth0)
    changed = np.any(color != color0, axis=-1).mean()
    print(f"{pose}: {changed:.1%} of pixels differ from the origin-(0, 0) frame")
    assert changed >= 0.10
    r.close()


def test_gi_update_equals_numpy(rv, oracle, atlas):
    ow = _world128(oracle, atlas)
    n = 32 ** 3
    with A.anchored(ORIGIN):
        want = S.gi_update(_np_trace(ow), _np_world(ow), 3, 0, n, atlas)
    got = {}
    for origin in [(0, 0), ORIGIN]:
        r = rv.StateRender((7, 7, 7), 64, 64, atlas=atlas)
        r.world_build()
        r.gi_update(0)
        assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ow.gi)
        r.texture_origin_set(*origin)
        r.gi_update(3)
        got[origin] = r.world_export(rv.RV_WORLD_GI).reshape(-1, 4)
        r.close()
    bad = np.any(got[ORIGIN] != want, axis=1)
    assert not bad.any(), f"{bad.sum()} cells differ, first {np.flatnonzero(bad)[:5]}"
    differ = int(np.any(got[ORIGIN] != got[(0, 0)], axis=1).sum())
    print(f"{differ} cells differ from the origin-(0, 0) update")
    assert differ >= 1


# ---------------------------------------------------------------- 3. the table scrolled equals the table rebuilt
SEED = (1000, -2000)
MOVES = {0: [(8, 0), (-24, 0), (64, 0), (8, -8), (256, 0)], 2: [(0, 8), (0, -24), (0, 64), (8, -8), (0, -256)]}


def _pose(lg):
    X, Y, Z = dims(lg)
    return ((X / 2 + 3.3, 62.0, Z / 2 + 1.7), 2.44, -3.6)


def _scroll_ctx(rv, atlas, lg, seed, table=1):
    c = rv.StateRender(lg, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, seed=seed, tex_table=table,
                       gi_rays_per_frame=2048)
    c.world_build()
    return c


def _plain(c):
    """Nothing computed ahead: no flow frames, no pipelined loop."""
    c.set_flow(0)
    c.set_gi_async(0)
    c.set_pipeline(0)
    return c


def _frames_three_ways(rv, r, t, descs, what):
    """r: flow frames, two-launch frames and the pipelined loop; t makes the same calls with nothing computed
    ahead.  Both advance alike, so one pair of contexts serves all three."""
    flags = rv.RV_FLAGS_REFERENCE
    launches = r.flow_info()[1]
    r.set_flow(1)
    for d in descs[:2]:
        draw(r, d, update_gi=True)
        draw(t, d, update_gi=True)
    same_frames(rv, r, t, (what, "flow"))
    assert r.flow_info()[1] == launches + 2 and r.flow_info()[2] == 0
    r.set_flow(0)
    for d in descs[2:4]:
        draw(r, d, update_gi=True)
        draw(t, d, update_gi=True)
    same_frames(rv, r, t, (what, "two-launch"))
    for c in (r, t):
        c.render_frame_seq(descs[4:7], next_desc=descs[7], flags=flags, gi_per_frame=True)
    same_frames(rv, r, t, (what, "seq"))


@pytest.mark.parametrize("lg,axis", [((8, 6, 6), 0), ((6, 6, 8), 2)])
def test_table_scrolled_equals_table_rebuilt(rv, atlas, lg, axis):
    from rvgrt_amd.configs import camera_path
    r = _scroll_ctx(rv, atlas, lg, SEED)
    n = _scroll_ctx(rv, atlas, lg, SEED, table=-1)        # follow on without a table: only the origin moves
    for c in (r, n):
        c.texture_origin_set(*SEED)
        c.texture_follow_scroll(1)
        assert c.texture_origin() == (SEED, True)
    info = r.tex_table_info()
    assert info[0] and not n.tex_table_info()[0]
    pos, ny = _table_positions(r)
    assert ny >= 8 and len(pos) == 256 * 64 * min(64, ny + 8)
    seq = camera_path(_pose(lg), W, H, 8, pan=0.01, ref_compat=True)
    origin = list(SEED)
    for dx, dz in MOVES[axis]:
        for c in (r, n):
            c.world_scroll(dx, dz)
        origin[0] += dx
        origin[1] += dz
        what = (lg, dx, dz)
        for c in (r, n):
            assert c.texture_origin() == (tuple(origin), True), what
            assert c.world_scroll_info()[3] == tuple(origin), what
        assert r.tex_table_info() == info
        want = rv.texture_tile_at(origin[0], origin[1], pos)
        got = r.texture_tiles(pos)
        assert np.array_equal(got, want), (what, int((got != want).sum()))
        assert np.array_equal(n.texture_tiles(pos), want), what
        # frames: a fresh context at the new seed with the same origin set.  rv_gi_init gives the scrolled
        # context the fresh one's grid and restarts its update sequence, so both make the same calls from here
        t = _plain(_scroll_ctx(rv, atlas, lg, tuple(origin)))
        t.texture_origin_set(*origin)
        assert np.array_equal(t.texture_tiles(pos), want), what
        r.gi_init()
        assert np.array_equal(gi(rv, r), gi(rv, t)), what
        # the camera path re-expressed in the moved grid (rv_scroll_view) while that keeps it inside the window
        sx, sz = (dx, dz) if max(abs(dx), abs(dz)) <= 64 else (0, 0)
        _frames_three_ways(rv, r, t, [shifted(rv, d, sx, sz) for d in seq], what)
        t.close()
    r.close()
    n.close()


def test_scrolled_frames_without_a_table_equal_the_table_context(rv, atlas):
    """Follow on and tex_table = -1: only the origin moves, and the frames are those of the table context."""
    from rvgrt_amd.configs import camera_path
    lg = (8, 6, 6)
    a, b = _scroll_ctx(rv, atlas, lg, SEED, table=1), _scroll_ctx(rv, atlas, lg, SEED, table=-1)
    seq = camera_path(_pose(lg), W, H, 3, pan=0.01, ref_compat=True)
    moved = [0, 0]
    for c in (a, b):
        c.texture_origin_set(*SEED)
        c.texture_follow_scroll(1)
    for dx, dz in [(8, 0), (-24, 8)]:
        for c in (a, b):
            c.world_scroll(dx, dz)
        moved = [moved[0] + dx, moved[1] + dz]
        for d in seq:
            for c in (a, b):
                draw(c, shifted(rv, d, moved[0], moved[1]), update_gi=True)
        same_frames(rv, a, b, (dx, dz))
    col = a.readback(rv.RV_IMAGE_COLOR)
    assert len(np.unique(col.reshape(-1, 4), axis=0)) > 50     # a frame of textured terrain
    a.close()
    b.close()


@pytest.mark.parametrize("lg,axis", [((8, 6, 6), 0), ((6, 6, 8), 2)])
def test_there_and_back_and_follow_off(rv, lg, axis):
    step = (8, 0) if axis == 0 else (0, 8)
    r = rv.StateRender(lg, 64, 64, seed=SEED, tex_table=1)
    r.world_build()
    pos, _ = _table_positions(r)
    # follow off (the default): the same scrolls leave every tile a function of grid coordinates
    grid = rv.texture_tile_at(0, 0, pos)
    for dx, dz in MOVES[axis][:4]:
        r.world_scroll(dx, dz)
        assert r.texture_origin() == ((0, 0), False)
        assert np.array_equal(r.texture_tiles(pos), grid), (dx, dz)
    # follow on: +8 then -8 restores every tile
    r.texture_origin_set(*SEED)
    r.texture_follow_scroll(1)
    before = r.texture_tiles(pos)
    r.world_scroll(*step)
    between = r.texture_tiles(pos)
    assert (between != before).mean() > 0.3
    r.world_scroll(-step[0], -step[1])
    assert r.texture_origin() == (SEED, True)
    assert np.array_equal(r.texture_tiles(pos), before)
    r.close()


# ---------------------------------------------------------------- 4. work computed ahead is discarded
@pytest.mark.parametrize("mode", ["draw", "seq"])
def test_origin_set_discards_work_computed_ahead(rv, atlas, mode):
    """Every update covers the whole grid (32,768 cells), so that each one reads enough textures to depend on
    the origin: a whole-grid update at ORIGIN differs from the one at (0, 0) in about ten cells."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    flags = rv.RV_FLAGS_REFERENCE
    seq = camera_path(TEST_POSES_128["P0"], W, H, 5, pan=0.01, ref_compat=True)
    r, t, u = (ctx128(rv, atlas, W, H, 32768), _plain(ctx128(rv, atlas, W, H, 32768)),
               _plain(ctx128(rv, atlas, W, H, 32768)))

    def run(ctxs, k0, k1):
        for c in ctxs:
            if mode == "draw":
                for d in seq[k0:k1]:
                    draw(c, d, update_gi=True)
            else:
                c.render_frame_seq(seq[k0:k1], next_desc=seq[k1], flags=flags, gi_per_frame=True)

    run((r, t, u), 0, 2)
    same_frames(rv, r, t, "before the set")
    for c in (r, t):
        c.texture_origin_set(*ORIGIN)
    run((r, t), 2, 3)
    same_frames(rv, r, t, "frame 3")
    # u never sets the origin: its grid differs, so the frames' updates do read the textures that changed
    run((u,), 2, 3)
    assert not np.array_equal(gi(rv, u), gi(rv, t))
    run((r, t), 3, 4)
    same_frames(rv, r, t, "frame 4")
    if mode == "draw":
        assert r.flow_info()[0] and r.flow_info()[1] == 4 and r.flow_info()[2] == 0 and not t.flow_info()[0]
    for c in (r, t, u):
        c.close()


@pytest.mark.parametrize("mode", ["draw", "seq"])
def test_setting_the_current_origin_keeps_the_work_computed_ahead(rv, atlas, mode):
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    flags = rv.RV_FLAGS_REFERENCE
    seq = camera_path(TEST_POSES_128["P0"], W, H, 5, pan=0.01, ref_compat=True)
    a, b = ctx128(rv, atlas, W, H, 4096), ctx128(rv, atlas, W, H, 4096)
    for c in (a, b):
        c.texture_origin_set(*ORIGIN)

    def run(k0, k1):
        for c in (a, b):
            if mode == "draw":
                for d in seq[k0:k1]:
                    draw(c, d, update_gi=True)
            else:
                c.render_frame_seq(seq[k0:k1], next_desc=seq[k1], flags=flags, gi_per_frame=True)

    run(0, 2)
    a.texture_origin_set(*ORIGIN)
    run(2, 4)
    same_frames(rv, a, b, "after setting the origin it has")
    assert a.stats() == b.stats()              # a discarded update or pre-pass would have been traced again
    assert a.flow_info() == b.flow_info()
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. two-rank loopback
def test_two_rank_loop_with_a_following_scroll_equals_one_rank(rv, atlas):
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    N, (dx, dz) = 2, (-8, 16)
    flags = rv.RV_FLAGS_REFERENCE
    seq = camera_path(TEST_POSES_128["P0"], W, H, 8, pan=0.02, ref_compat=True)
    seq = seq[:4] + [shifted(rv, d, dx, dz) for d in seq[4:]]
    ref = ctx128(rv, atlas, W, H, 4096)
    ref.set_pipeline(0)
    group = rv.LoopbackGroup(N, timeout_ms=60000)
    rs = [ctx128(rv, atlas, W, H, 4096) for _ in range(N)]
    comms = []
    for q, c in enumerate(rs):
        c.set_tile_shard(32, q, N)
        comms.append(rv.Comm.loopback(c, group, q))
    for c in rs + [ref]:
        c.texture_origin_set(*ORIGIN)
        c.texture_follow_scroll(1)
    for a, b in ((0, 4), (4, 8)):
        if a:
            for c in rs + [ref]:
                c.world_scroll(dx, dz)
                assert c.texture_origin() == ((ORIGIN[0] + dx, ORIGIN[1] + dz), True)
        run_ranks([lambda q=q: rs[q].render_frame_seq(seq[a:b], next_desc=seq[b] if b < 8 else None, flags=flags,
                                                      gi_per_frame=True, comm=comms[q]) for q in range(N)])
        for m in comms:
            m.wait(60000)
        for k in range(a, b):
            ref.update_gi_data()
            d = seq[k]
            ref.frame(d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp), time=d.time,
                      jx=d.jitter_x, jy=d.jitter_y, flags=flags)
        assert np.array_equal(rs[0].readback(rv.RV_IMAGE_COLOR), ref.readback(rv.RV_IMAGE_COLOR)), (a, b)
        want = ref.world_export(rv.RV_WORLD_GI)
        for q, c in enumerate(rs):
            assert np.array_equal(c.world_export(rv.RV_WORLD_GI), want), (q, a, b)
    for m in comms:
        m.close()
    for c in rs:
        c.close()
    group.close()
    ref.close()


# ---------------------------------------------------------------- 6. status codes
def test_status_codes(rv):
    lg = (7, 6, 7)
    r = rv.StateRender(lg, 64, 64, seed=(16, -8), tex_table=1)
    p = np.full((4, 3), 3.5, np.float32)
    with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
        r.texture_tiles(p)
    big = 2 ** 31 - 1
    for bad in ((big - 128 - 1321, 0), (0, big - 128 - 721), (big, big)):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.texture_origin_set(*bad)
    assert r.texture_origin() == ((0, 0), False)
    # an origin recorded before the table exists is the one it is built at
    top = (big - 128 - 1322 - 8, -2 ** 31)
    r.texture_origin_set(*top)
    r.world_build()
    pos, _ = _table_positions(r)
    tiles = r.texture_tiles(pos)
    assert np.array_equal(tiles, rv.texture_tile_at(top[0], top[1], pos))
    # a scroll that would overflow the texture origin only: refused before anything is written
    r.texture_follow_scroll(1)
    bits = r.world_export(rv.RV_WORLD_BITS)
    r.world_scroll(8, 0)
    r.world_scroll(-8, 0)
    for bad in ((16, 0), (0, -8), (8, -8)):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_scroll(*bad)
    assert r.texture_origin() == (top, True) and r.world_scroll_info()[3] == (16, -8)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), bits)
    assert np.array_equal(r.texture_tiles(pos), tiles)
    r.texture_follow_scroll(0)
    r.world_scroll(16, -8)                                  # not following: the same scroll is valid
    assert r.texture_origin() == (top, False)
    assert np.array_equal(r.texture_tiles(pos), tiles)
    r.close()
