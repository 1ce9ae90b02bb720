"""rv_world_scroll: the world window moved over the generated terrain in place.
Retained bits, CSDF bytes and GI cells move to their new index, the entering
slab is generated at the new origin, the CSDF slabs a step can change and the
exits are rebuilt, entering GI cells take gi_init's value.  The yardsticks are
the oracle (OracleWorld at the new origin; build_csdf of the expected bits;
gi_init / gi_update), the numpy exit tables of tests/np_exits.py and twin
contexts (built at the new seed, or fed the expected world through
world_import).  Every comparison is bit-exact."""
import numpy as np
import pytest

from gpu_world import (ctx128, dims, draw, generated, gi, run_ranks, rv, same_frames, same_tables, shifted, sparse_bits,
                       step, sun, tables, voxels, world)
import np_exits as E
import np_world as R

pytestmark = pytest.mark.gpu

W, H = 320, 192


def _entering(lg, axis, d, arr, cell):
    """The part of a [z, y, x] array (cell voxels per entry) that entered with a step of d along axis."""
    n = arr.shape[2 - axis]
    k = abs(d) // cell
    sl = [slice(None)] * 3
    sl[2 - axis] = slice(n - k, n) if d > 0 else slice(0, k)
    return arr[tuple(sl)]


def _box(arr, b):
    return arr[b[4]:b[5], b[2]:b[3], b[0]:b[1]]


# ---------------------------------------------------------------- 1. generated terrain
@pytest.mark.parametrize("lg,axis", [((9, 7, 7), 0), ((7, 7, 9), 2)])
def test_generated_terrain(rv, oracle, sun, lg, axis):
    S = tuple(d // 2 for d in dims(lg))
    origin = [16, -40]
    r = rv.StateRender(lg, 64, 64, seed=tuple(origin))
    r.world_build()
    assert r.world_scroll_info() == (0, 0, False, tuple(origin))
    for n, d in enumerate((8, -24, 64), 1):
        r.world_scroll(*step(axis, d))
        origin[0 if axis == 0 else 1] += d
        bits, csdf = world(rv, r)
        want_bits, want_csdf = generated(oracle, lg, tuple(origin), csdf=True)
        assert np.array_equal(bits, want_bits), (lg, d)
        assert np.array_equal(csdf, want_csdf), (lg, d)
        tr, ld, cells, full = rv.scroll_region(lg, axis, d)
        assert not full and r.world_scroll_info() == (n, cells, False, tuple(origin))
        # a fresh context at the new seed: the same world and the same exit tables
        t = rv.StateRender(lg, 64, 64, seed=tuple(origin))
        t.world_build()
        tb, tc = world(rv, t)
        assert np.array_equal(bits, tb) and np.array_equal(csdf, tc), (lg, d)
        tabs = tables(rv, r)
        same_tables(tabs, tables(rv, t), (lg, d))
        t.close()
        vox = voxels(bits, lg)
        E.check_tables(E.reference(vox, sun), *tabs, f"{lg} scrolled by {d}")
        # the case itself: the slab that entered is neither all solid nor all empty, and both rebuilt
        # boxes hold a spread of distances (a wrong stride or clip cannot pass by luck)
        slab = _entering(lg, axis, d, vox, 1)
        assert slab.any() and not slab.all()
        c3 = csdf.reshape(S[2], S[1], S[0])
        for b in (tr, ld):
            assert len(np.unique(_box(c3, b))) >= 16, (lg, d, b)
    r.close()


# ---------------------------------------------------------------- 2. imported sparse worlds
@pytest.mark.parametrize("lg,axis", [((10, 6, 6), 0), ((6, 6, 10), 2)])
def test_imported_sparse_worlds(rv, oracle, lg, axis):
    """Random bits of density 2e-5 (84 voxels), moved by +8, -8 and +40 one after the other: the retained
    imported voxels move, the slab is generated, the CSDF equals the oracle's build of the expected bits.
    At this density the voxels stand about 6 cells apart along the long axis, so the expectation differs
    from the shifted old CSDF no further than 20 cells from the trailing face (x: 17, 20, 9; z: none, 15,
    3) or before the entering planes (x: 20, 19, 20; z: 15, 18, 15) -- the oracle's figures for these seeds,
    printed below; no seed can give the 48 cells asked for (the cell would need a gap of 100 empty cells
    around it).  test_imported_sparse_worlds_far_reach makes that assertion, in worlds of 4 voxels."""
    S = tuple(d // 2 for d in dims(lg))
    origin = list(R.ORIGIN)
    r = rv.StateRender(lg, 64, 64, seed=R.ORIGIN)
    r.world_import(rv.RV_WORLD_BITS, sparse_bits(lg, 2e-5, 31 + axis))
    r.csdf_build()
    for d in (8, -8, 40):
        old_bits = r.world_export(rv.RV_WORLD_BITS)
        want_bits, old_csdf, want_csdf = R.scrolled(oracle, lg, axis, d, old_bits, tuple(origin))
        r.world_scroll(*step(axis, d))
        origin[0 if axis == 0 else 1] += d
        bits, csdf = world(rv, r)
        assert np.array_equal(bits, want_bits), (lg, d)
        assert np.array_equal(csdf, want_csdf.ravel()), (lg, d)
        assert r.world_scroll_info()[1:] == (rv.scroll_region(lg, axis, d)[2], False, tuple(origin))
        reach = R.reaches(axis, d, S, want_csdf != old_csdf)
        print(f"{lg} d {d}: trailing / leading reach {reach}")
        assert (want_csdf != old_csdf).any() and max(reach) <= 63
    r.close()


@pytest.mark.parametrize("d", [8, -8, 40])
@pytest.mark.parametrize("lg,axis", [((10, 6, 6), 0), ((6, 6, 10), 2)])
def test_imported_sparse_worlds_far_reach(rv, oracle, lg, axis, d):
    """The 4-voxel worlds of tests/test_world_scroll_region.py, whose seeds were picked on the oracle alone:
    the expectation differs from the shifted old CSDF >= 48 cells from the trailing face and >= 48 cells
    before the entering planes, so a rebuild of narrower slabs would leave stale bytes."""
    S = tuple(v // 2 for v in dims(lg))
    old_bits = sparse_bits(lg, 1e-6, R.SPARSE_SEEDS[(lg, axis, d)])
    want_bits, old_csdf, want_csdf = R.scrolled(oracle, lg, axis, d, old_bits)
    reach = R.reaches(axis, d, S, want_csdf != old_csdf)
    assert min(reach) >= 48, (lg, d, reach)
    r = rv.StateRender(lg, 64, 64, seed=R.ORIGIN)
    r.world_import(rv.RV_WORLD_BITS, old_bits)
    r.csdf_build()
    r.world_scroll(*step(axis, d))
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, want_bits), (lg, d)
    assert np.array_equal(csdf, want_csdf.ravel()), (lg, d)
    assert not r.world_scroll_info()[2]
    r.close()


# ---------------------------------------------------------------- 3. both axes in one call
def test_both_axes_in_one_call(rv, oracle, atlas):
    lg, dx, dz = (9, 6, 9), 8, -16
    r, t = (rv.StateRender(lg, 64, 64, atlas=atlas, seed=(-8, 24)) for _ in range(2))
    for c in (r, t):
        c.world_build()
    r.world_scroll(dx, dz)
    t.world_scroll(dx, 0)
    cells = t.world_scroll_info()[1]
    t.world_scroll(0, dz)
    cells += t.world_scroll_info()[1]
    assert cells == rv.scroll_region(lg, 0, dx)[2] + rv.scroll_region(lg, 2, dz)[2]
    assert r.world_scroll_info() == (1, cells, False, (0, 8)) and t.world_scroll_info()[0] == 2
    bits, csdf = world(rv, r)
    tb, tc = world(rv, t)
    assert np.array_equal(bits, tb) and np.array_equal(csdf, tc)
    assert np.array_equal(gi(rv, r), gi(rv, t))
    same_tables(tables(rv, r), tables(rv, t), "x then z")
    want_bits, want_csdf = generated(oracle, lg, (0, 8), csdf=True)
    assert np.array_equal(bits, want_bits) and np.array_equal(csdf, want_csdf)
    r.close()
    t.close()


# ---------------------------------------------------------------- 4. the whole-grid fallback
def test_fallback_and_every_voxel_entering(rv, oracle, sun):
    lg = (7, 7, 7)
    r = rv.StateRender(lg, 64, 64)
    r.world_build()
    origin = (0, 0)
    for n, (dx, dz) in enumerate([(8, 0), (0, -16), (128, 0), (-136, 256), (0, -1024)], 1):
        r.world_scroll(dx, dz)
        origin = (origin[0] + dx, origin[1] + dz)
        assert r.world_scroll_info() == (n, (1 + (dx != 0 and dz != 0)) * 64 ** 3, True, origin)
        bits, csdf = world(rv, r)
        want_bits, want_csdf = generated(oracle, lg, origin, csdf=True)
        assert np.array_equal(bits, want_bits) and np.array_equal(csdf, want_csdf), (dx, dz)
    t = rv.StateRender(lg, 64, 64, seed=origin)
    t.world_build()
    tabs = tables(rv, r)
    same_tables(tabs, tables(rv, t), "fallback")
    E.check_tables(E.reference(voxels(bits, lg), sun), *tabs, "fallback")
    # every voxel entered with the last step: the GI grid is a fresh init's
    assert np.array_equal(gi(rv, r), gi(rv, t))
    r.close()
    t.close()


# ---------------------------------------------------------------- 5. composition
def test_composition_and_edits(rv, oracle):
    lg = (9, 6, 6)
    X, Y, Z = dims(lg)
    r, t = (rv.StateRender(lg, 64, 64, seed=(64, 64)) for _ in range(2))
    for c in (r, t):
        c.world_build()
    bits0, csdf0 = world(rv, r)
    tabs0 = tables(rv, r)
    # +8, +16 against +24
    r.world_scroll(8, 0)
    r.world_scroll(16, 0)
    t.world_scroll(24, 0)
    bits, csdf = world(rv, r)
    tb, tc = world(rv, t)
    assert np.array_equal(bits, tb) and np.array_equal(csdf, tc)
    assert not np.array_equal(bits, bits0)
    same_tables(tables(rv, r), tables(rv, t), "+8 +16 / +24")
    # ... and back: bits, CSDF and exits of the unedited world
    r.world_scroll(-24, 0)
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, bits0) and np.array_equal(csdf, csdf0)
    same_tables(tables(rv, r), tabs0, "+24 -24")
    assert r.world_scroll_info()[3] == (64, 64)
    # an edit inside the part a scroll retains arrives shifted (and one in the part that leaves is gone)
    boxes = [(200, 36, 20, 209, 47, 29, 1), (203, 38, 22, 206, 44, 26, 0), (3, 50, 3, 6, 53, 6, 1)]
    r.world_edit(boxes)
    edited = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
    assert edited[25, 40, 201] and not edited[24, 40, 204] and edited[4, 51, 4]
    r.world_scroll(40, 0)
    bits, csdf = world(rv, r)
    vox = voxels(bits, lg)
    assert np.array_equal(vox[:, :, :X - 40], edited[:, :, 40:])
    gen = voxels(generated(oracle, lg, (104, 64), csdf=True)[0], lg)
    assert np.array_equal(vox[:, :, X - 40:], gen[:, :, X - 40:])
    assert vox[25, 40, 161] and not vox[24, 40, 164]
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = bits
    ow.build_csdf()
    assert np.array_equal(csdf, ow.csdf)
    assert not r.world_scroll_info()[2]
    r.close()
    t.close()


# ---------------------------------------------------------------- 6. the GI grid
@pytest.mark.parametrize("saturate", [False, True])
@pytest.mark.parametrize("lg,axis,d,seed", [((9, 6, 6), 0, 16, (40, -24)), ((6, 6, 9), 2, -24, (300, -500))])
def test_gi_grid(rv, oracle, atlas, lg, axis, d, seed, saturate):
    G = tuple(v // 4 for v in dims(lg))
    rays = 3000
    r = rv.StateRender(lg, 64, 64, atlas=atlas, seed=seed, gi_rays_per_frame=rays, gi_init_saturate=saturate)
    r.world_build()
    r.update_gi_data()
    r.update_gi_data()
    g0 = gi(rv, r).reshape(G[2], G[1], G[0])
    traces0, relight0 = r.stats()["gi_traces"], r.gi_relight_info()
    r.world_scroll(*step(axis, d))
    origin = (seed[0] + step(axis, d)[0], seed[1] + step(axis, d)[1])
    g1 = gi(rv, r).reshape(G[2], G[1], G[0])
    # retained cells: the old grid at the new index
    g = d // 4
    ax = 2 - axis
    keep_new = [slice(None)] * 3
    keep_old = [slice(None)] * 3
    keep_new[ax] = slice(0, G[axis] - g) if g > 0 else slice(-g, G[axis])
    keep_old[ax] = slice(g, G[axis]) if g > 0 else slice(0, G[axis] + g)
    assert np.array_equal(g1[tuple(keep_new)], g0[tuple(keep_old)])
    # entering cells: the oracle's gi_init in the new world
    ow = oracle.OracleWorld(*lg, atlas=atlas, ox=origin[0], oz=origin[1]).fill().build_csdf()
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
    ow.gi_init(saturate=saturate)
    init = ow.gi.view(np.uint32).reshape(G[2], G[1], G[0])
    got, want = _entering(lg, axis, d, g1, 4), _entering(lg, axis, d, init, 4)
    assert np.array_equal(got, want)
    lit = 0xFFFFFFFF if saturate else 0xFFFEF7F6
    assert (want == lit).any() and (want == 0xFF000000).any()   # both outcomes of the sun trace entered
    assert r.stats()["gi_traces"] - traces0 == want.size
    assert r.gi_relight_info() == relight0
    # the rolling update goes on: frame 2 at offset 2 * rays, on the scrolled grid
    ow.gi[:] = g1.ravel().view(np.uint8)
    ow.gi_update(2, first=2 * rays, count=rays)
    r.update_gi_data()
    assert np.array_equal(gi(rv, r), ow.gi.view(np.uint32))
    r.close()


# ---------------------------------------------------------------- 7. frames across a scroll
def _modes(mode, in_flight, ahead, plain):
    """ahead: the defaults of the mode (work computed ahead); plain: nothing computed ahead."""
    if mode == "draw":
        plain.set_flow(0)
        plain.set_gi_async(0)
    else:
        plain.set_pipeline(0)
    if in_flight > 1:
        for c in ahead + [plain]:
            c.set_frames_in_flight(in_flight)
    if mode == "group":
        for c in ahead:
            c.set_frame_group(2)
            assert c.frame_group_effective() == 2


def _run(rv, ctxs, mode, descs, nxt, flags):
    for c in ctxs:
        if mode == "draw":
            for d in descs:
                c.update_gi_data()
                draw(c, d)
        else:
            c.render_frame_seq(descs, next_desc=nxt, flags=flags, gi_per_frame=True)


@pytest.mark.parametrize("mode,in_flight", [("draw", 1), ("two", 1), ("seq", 1), ("group", 1), ("draw", 2), ("seq", 2)])
def test_frames_across_a_scroll(rv, oracle, atlas, mode, in_flight):
    """renderLoop's frames before and after a scroll, the camera re-expressed by rv_scroll_view.  r: the
    mode's defaults -- flow frames whose launch computes the next update ahead (draw), two-launch frames with
    the asynchronous update (two), the pipelined loop with its kept pre-pass and update (seq), grouped frames
    (group).  t: nothing computed ahead, and the scrolled world handed over through world_import."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, (dx, dz) = (7, 7, 7), (8, -16)
    flags = rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2 * n, pan=0.01, ref_compat=True)
    r, t = ctx128(rv, atlas, W, H, 4096), ctx128(rv, atlas, W, H, 4096)
    if mode == "two":
        r.set_flow(0)
    _modes("draw" if mode == "two" else mode, in_flight, [r], t)
    m = "draw" if mode == "two" else mode
    _run(rv, (r, t), m, seq[:n], seq[n], flags)
    same_frames(rv, r, t, "before")
    r.world_scroll(dx, dz)
    want_bits, want_csdf = generated(oracle, lg, (dx, dz), csdf=True)
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, want_bits) and np.array_equal(csdf, want_csdf)
    t.world_import(rv.RV_WORLD_BITS, want_bits)
    t.world_import(rv.RV_WORLD_CSDF, want_csdf)
    t.world_import(rv.RV_WORLD_GI, r.world_export(rv.RV_WORLD_GI))
    after = [shifted(rv, d, dx, dz) for d in seq[n:]]
    _run(rv, (r, t), m, after[:n], after[n], flags)
    same_frames(rv, r, t, "after")
    assert r.flow_info()[2] == 0
    if mode == "draw" and in_flight == 1:
        assert r.flow_info()[0] and r.flow_info()[1] == 2 * n and not t.flow_info()[0]
    # the step counters of one more frame (a stats frame computes nothing ahead in either context)
    d = after[n]
    for c in (r, t):
        c.stats_reset()
        c.frame(d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp), time=d.time,
                jx=d.jitter_x, jy=d.jitter_y, flags=flags | rv.RV_F_STATS)
    same_frames(rv, r, t, "stats frame")
    for stage in (0, 2):   # pre-pass and render: the blocks a flow frame and a two-launch frame both fill
        assert r.stats(stage) == t.stats(stage), stage
    assert r.stats(2)["primary"] == W * H
    r.close()
    t.close()


@pytest.mark.parametrize("mode", ["draw", "seq"])
def test_null_scroll_keeps_the_work_computed_ahead(rv, atlas, mode):
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    flags = rv.RV_FLAGS_REFERENCE
    n = 3
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2 * n, pan=0.01, ref_compat=True)
    a, b = ctx128(rv, atlas, W, H, 4096), ctx128(rv, atlas, W, H, 4096)
    _run(rv, (a, b), mode, seq[:n], seq[n], flags)
    info = a.world_scroll_info()
    a.world_scroll(0, 0)
    assert a.world_scroll_info() == info == (0, 0, False, (0, 0))
    _run(rv, (a, b), mode, seq[n:2 * n], seq[2 * n], flags)
    same_frames(rv, a, b, "after the null scroll")
    # a discarded update or pre-pass would have been traced a second time
    assert a.stats() == b.stats()
    assert a.flow_info() == b.flow_info()
    a.close()
    b.close()


# ---------------------------------------------------------------- 8. status codes, origin, seed
def test_status_origin_and_seed(rv, oracle):
    lg = (7, 6, 7)
    r = rv.StateRender(lg, 64, 64, seed=(-24, -8))
    with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
        r.world_scroll(8, 0)
    r.world_build()
    bits, csdf = world(rv, r)
    gi0 = gi(rv, r)
    for bad in ((4, 0), (0, -12), (7, 8), (8, 1)):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_scroll(*bad)
    big = 2 ** 31 - 8
    for bad in ((big, 0), (0, big - 112), (-2 ** 31, 0), (0, -2 ** 31)):   # origin + d (+ dim) leaves int32
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_scroll(*bad)
    r.world_scroll(0, 0)
    assert r.world_scroll_info() == (0, 0, False, (-24, -8))
    nb, nc = world(rv, r)
    assert np.array_equal(nb, bits) and np.array_equal(nc, csdf) and np.array_equal(gi(rv, r), gi0)
    # a later world_build regenerates the scrolled window
    r.world_scroll(-16, 40)
    assert r.world_scroll_info() == (1, 2 * 64 * 32 * 64, True, (-40, 32))
    nb, nc = world(rv, r)
    r.world_build()
    bb, bc = world(rv, r)
    assert np.array_equal(bb, nb) and np.array_equal(bc, nc) and not np.array_equal(nb, bits)
    want_bits, want_csdf = generated(oracle, lg, (-40, 32), csdf=True)
    assert np.array_equal(bb, want_bits) and np.array_equal(bc, want_csdf)
    assert r.world_scroll_info()[3] == (-40, 32)
    # the largest origins are reachable
    r.world_scroll(2 ** 31 - 1 - 128 - 7 + 40, 0)
    assert r.world_scroll_info()[3] == (2 ** 31 - 1 - 128 - 7, 32)
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        r.world_scroll(8, 0)
    r.close()


# ---------------------------------------------------------------- 9. two-rank loopback
def test_two_rank_loop_with_a_scroll_equals_one_rank(rv, atlas):
    """Both ranks of a tile-sharded loop scroll between two calls: the gathered frame and every rank's GI
    grid equal one context rendering whole frames one at a time with the same scroll."""
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
    for a, b in ((0, 4), (4, 8)):
        if a:
            for c in rs + [ref]:
                c.world_scroll(dx, dz)
        run_ranks([lambda q=q: rs[q].render_frame_seq(seq[a:b], next_desc=seq[b], flags=flags, gi_per_frame=True,
                                                      comm=comms[q]) for q in range(N)])
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
