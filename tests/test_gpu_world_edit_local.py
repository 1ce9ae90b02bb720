"""rv_world_edit's local CSDF rebuild (launch_csdf_box over the four clipped cell
boxes of an edit) in worlds whose CSDF has structure, at every clipping case of
the region, with the longest edit list, and read afterwards by rays, frames, GI
updates, relights and a two-rank loop.  test_gpu_world_edit.py runs the same
calls mostly on 128^3 worlds, which always take the whole-grid fallback; every
edit here that means to be local asserts world_edit_info() == (n,
edit_region's cell count, False), so a test that silently fell back fails.

The yardsticks are the CPU oracle (build_csdf, trace_batch, gi_update, render:
no exits, no local path) and a twin context that receives world_import(BITS,
host-edited bits) + csdf_build().  Every comparison is bit-exact.

Base worlds: T, the generated terrain at log2 dims (9, 7, 7); S, 2e-5-dense
random bits in (8, 8, 8), (7, 9, 7) and (7, 7, 9)."""
import numpy as np
import pytest

from conftest import random_rays
from gpu_world import (block_in_view, cells, draw, edited, oracle_of, pack, run_ranks, rv, same_frames, same_world,
                       sparse_bits, twin_edit, voxels)
from np_world import expect_relight

pytestmark = pytest.mark.gpu

T_LG = (9, 7, 7)
S_SEED = {(8, 8, 8): 31, (7, 9, 7): 32, (7, 7, 9): 33}
W, H = 160, 96


@pytest.fixture(scope="module")
def terrain(oracle_world):
    """T on the CPU: (bits, csdf), built once, never changed."""
    w = oracle_world(*T_LG, gi_sweeps=0)
    return w.bits.copy(), w.csdf.copy()


_SPARSE = {}


@pytest.fixture(scope="module")
def sparse(oracle):
    """Factory: S at these log2 dims on the CPU, (bits, csdf), built once per module, never changed."""
    def make(lg):
        if lg not in _SPARSE:
            ow = oracle.OracleWorld(*lg)
            ow.bits[:] = sparse_bits(lg, 2e-5, S_SEED[lg])
            ow.build_csdf()
            _SPARSE[lg] = (ow.bits.copy(), ow.csdf.copy())
        return _SPARSE[lg]
    return make


# ---------------------------------------------------------------- helpers
def _pair(rv, lg, bits=None, w=64, h=64, **kw):
    """A context and its twin holding the same world: the generated one, or these bits."""
    r, t = (rv.StateRender(lg, w, h, **kw) for _ in range(2))
    for c in (r, t):
        if bits is None:
            c.world_build()
        else:
            c.world_import(rv.RV_WORLD_BITS, bits)
            c.csdf_build()
    return r, t


def _assert_local(rv, r, lg, boxes, n):
    region, ncells = rv.edit_region(lg, boxes)
    SX, SY, SZ = cells(lg)
    assert 0 < ncells < SX * SY * SZ
    assert r.world_edit_info() == (n, ncells, False), (n, ncells, r.world_edit_info())
    return region


def _halo_matters(oracle, ow, lg, region):
    """CPU only.  The CSDF inside the region F of a world that keeps only F's own voxels differs from the
    real one inside F, and F holds many distinct values: the bytes a local rebuild writes depend on what
    its halo boxes (solid, dx, dy beyond F) hold, so a wrong stride, clip or halo there shows."""
    SX, SY, SZ = cells(lg)
    x0, x1, y0, y1, z0, z1 = region
    vox = ow.voxels()
    cut = np.zeros_like(vox)
    cut[2 * z0:2 * z1, 2 * y0:2 * y1, 2 * x0:2 * x1] = vox[2 * z0:2 * z1, 2 * y0:2 * y1, 2 * x0:2 * x1]
    alone = oracle_of(oracle, lg, pack(cut))
    F = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    whole = ow.csdf.reshape(SZ, SY, SX)[F]
    differing = int((alone.csdf.reshape(SZ, SY, SX)[F] != whole).sum())
    distinct = len(np.unique(whole))
    print(f"{lg} F={region}: {differing} cells of F depend on voxels outside F, {distinct} distinct values in F")
    assert differing > 0
    assert distinct >= 16


def _edit_steps(rv, oracle, r, t, ow, lg, steps, full=(), want_region=None):
    """Each step's boxes through world_edit on r, the host edit + csdf_build on t and the oracle; bits and
    CSDF of the three compared over the whole grid.  `full` lists the steps (from 1) that must report the
    whole-grid build; every other step must report the local one.  Returns the CSDF bytes each step changed."""
    SX, SY, SZ = cells(lg)
    out = []
    checked = False
    for n, boxes in enumerate(steps, 1):
        prev = ow.csdf.copy()
        r.world_edit(boxes)
        twin_edit(rv, t, lg, boxes)
        ow.bits[:] = edited(ow.bits, lg, boxes)
        ow.build_csdf()
        if n in full:
            assert r.world_edit_info() == (n, SX * SY * SZ, True), (n, r.world_edit_info())
        else:
            region = _assert_local(rv, r, lg, boxes, n)
            if n == 1 and want_region is not None:
                assert region == want_region, (region, want_region)
        bits, csdf = same_world(rv, r, t, (lg, n))
        assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf), (lg, n)
        changed = int((ow.csdf != prev).sum())
        what = boxes if len(boxes) < 4 else f"{len(boxes)} boxes"
        print(f"{lg} {what}: {'full' if n in full else 'local'}, {changed} CSDF bytes change")
        assert changed > 0   # a rebuild that does nothing cannot pass
        if n not in full and not checked:
            _halo_matters(oracle, ow, lg, region)
            checked = True
        out.append(changed)
    return out


def _set_then_clear(x, y, z):
    """A 3 x 3 x 3 set with its low corner at the voxel, then a 2 x 3 x 1 clear inside it.  The clear takes
    the z plane of the set that is alone in its coarse cell, and x + 1 .. x + 2 is a whole cell or ends in a
    cell the set holds one column of: the clear empties coarse cells again, so the CSDF changes twice."""
    zc = z if z & 1 else z + 2
    return [[(x, y, z, x + 3, y + 3, z + 3, 1)], [(x + 1, y, zc, x + 3, y + 3, zc + 1, 0)]]


# ---------------------------------------------------------------- 1. every clipping case
# The set's first voxel on the long axis (512 voxels, 256 cells) and the cells the local rebuild must
# recompute along it: E grown by 64, clipped.
LONG_CASES = [(0, (0, 66)),        # clipped at the low face
              (128, (0, 130)),     # E - 64 == 0 exactly
              (129, (0, 130)),
              (130, (1, 131)),     # one cell off that
              (255, (63, 193)),    # unclipped, straddling two cells
              (379, (125, 255)),   # last voxel 381: one cell off the high face
              (380, (126, 256)),   # last voxel 382: E + 64 == S exactly
              (381, (126, 256)),   # last voxel 383
              (509, (190, 256))]   # last voxel 511: clipped at the high face


@pytest.mark.parametrize("p,span", LONG_CASES)
def test_local_rebuild_in_the_terrain(rv, oracle, terrain, p, span):
    lg = T_LG
    r, t = _pair(rv, lg)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), terrain[0])
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), terrain[1])
    ow = oracle_of(oracle, lg, *terrain)
    z = 61
    col = ow.voxels()[z + 1, :, p + 1]
    y = min(int(np.nonzero(col)[0].max()) + 1, 124)   # on the ground of the middle column
    _edit_steps(rv, oracle, r, t, ow, lg, _set_then_clear(p, y, z), want_region=span + (0, 64, 0, 64))
    r.close()
    t.close()


@pytest.mark.parametrize("p,span", LONG_CASES)
@pytest.mark.parametrize("lg", [(7, 9, 7), (7, 7, 9)])
def test_local_rebuild_along_y_and_z(rv, oracle, sparse, lg, p, span):
    bits0, csdf0 = sparse(lg)
    r, t = _pair(rv, lg, bits0)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), csdf0)
    ow = oracle_of(oracle, lg, bits0, csdf0)
    at = (61, p, 70) if lg[1] == 9 else (61, 70, p)
    want = (0, 64) + span + (0, 64) if lg[1] == 9 else (0, 64, 0, 64) + span
    _edit_steps(rv, oracle, r, t, ow, lg, _set_then_clear(*at), want_region=want)
    r.close()
    t.close()


# local on all three axes at once: the set's low corner, the region of the set (E grown by 64, clipped)
CUBE_CASES = [((0, 0, 0), (0, 66, 0, 66, 0, 66)),
              ((253, 253, 253), (62, 128, 62, 128, 62, 128)),    # the corner voxel (255, 255, 255)
              ((0, 253, 0), (0, 66, 62, 128, 0, 66)),            # the mixed corner (0, 255, 0)
              ((100, 100, 100), (0, 116, 0, 116, 0, 116)),
              ((60, 200, 128), (0, 96, 36, 128, 0, 128)),
              ((128, 128, 128), None)]                           # the centre: the whole-grid fallback, see below


@pytest.mark.parametrize("at,region", CUBE_CASES)
def test_local_rebuild_on_three_axes(rv, oracle, sparse, at, region):
    """(8, 8, 8): 128 cells per axis, so an edit is local only where its region is clipped enough.  The set at
    the centre is not: cells 64..65 grown by 64 cover the grid, its four passes would visit exactly the
    whole-grid build's 4 * 128^3 = 8.39 M cells, and at equality the call must report the whole-grid build.
    The clear inside it (coarse cells 64..65 x 64..65 x 65, a region of 128 x 128 x 127 cells) visits 8.37 M
    and must be local: the crossover pinned from both sides."""
    lg = (8, 8, 8)
    bits0, csdf0 = sparse(lg)
    r, t = _pair(rv, lg, bits0)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), csdf0)
    ow = oracle_of(oracle, lg, bits0, csdf0)
    _edit_steps(rv, oracle, r, t, ow, lg, _set_then_clear(*at), full=(1,) if region is None else (),
                want_region=region)
    r.close()
    t.close()


# ---------------------------------------------------------------- 2. the longest edit list
def test_longest_edit_list_in_order(rv, oracle, terrain):
    lg = T_LG
    n = rv._lib.RV_EDIT_MAX_BOXES
    assert n == 1024
    rng = np.random.default_rng(11)
    boxes = []
    for _ in range(n):   # box by box: the origin, the sides of 1 to 11 voxels, solid or not
        o, s, k = rng.integers((200, 60, 50), (240, 100, 90)), rng.integers(1, 12, 3), rng.integers(0, 2)
        boxes.append(tuple(int(v) for v in (*o, *(o + s), k)))
    want = edited(terrain[0], lg, boxes)
    changed = int((voxels(want, lg) != voxels(terrain[0], lg)).sum())
    reverse = edited(terrain[0], lg, boxes[::-1])
    by_kind = edited(terrain[0], lg, [b for b in boxes if not b[6]] + [b for b in boxes if b[6]])
    d_rev = int((voxels(reverse, lg) != voxels(want, lg)).sum())
    d_kind = int((voxels(by_kind, lg) != voxels(want, lg)).sum())
    print(f"{n} boxes change {changed} voxels; {d_rev} differ in reverse order, {d_kind} with the clears first")
    assert changed > 0 and d_rev > 0 and d_kind > 0   # the order of the list matters
    r, t = _pair(rv, lg)
    ow = oracle_of(oracle, lg, *terrain)
    _edit_steps(rv, oracle, r, t, ow, lg, [boxes])
    assert np.array_equal(ow.bits, want)
    # the same list again changes no voxel: no rebuild, not an edit
    r.world_edit(boxes)
    assert r.world_edit_info() == (1, 0, False)
    same_world(rv, r, t, "repeat")
    r.close()
    t.close()


# ---------------------------------------------------------------- 3. rays, frames and GI after a local edit
def _frame_pair(rv, atlas, lg, bits=None, **kw):
    r, t = _pair(rv, lg, bits, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, **kw)
    if bits is not None:
        for c in (r, t):
            c.gi_init()
    return r, t


def _oracle_frame(rv, oracle, ow, cam, vp, flags):
    return oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)), want_stats=False)["rgba"]


def test_exits_follow_a_local_edit(rv, atlas, oracle, terrain):
    """The sky exit, the column tops and the sun horizon are re-derived after a local rebuild as after a
    whole-grid one: rays against the oracle (which has no exits), frames and step counts against the twin."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg = T_LG
    X, Y, Z = (1 << l for l in lg)
    flags = rv.RV_FLAGS_REFERENCE
    vox = voxels(terrain[0], lg)
    vox[:, 90:, :] = False            # the terrain reaches row 127: cut it, so the sky exit has room to move
    assert vox[:, 89, :].any()
    ow = oracle_of(oracle, lg, pack(vox), atlas=atlas)
    r, t = _frame_pair(rv, atlas, lg, ow.bits)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
    ow.gi[:] = r.world_export(rv.RV_WORLD_GI)
    tops = np.where(vox.any(axis=1), Y - 1 - np.argmax(vox[:, ::-1, :], axis=1), -1)   # [z, x]
    lz, lx = (int(v) for v in np.unravel_index(np.argmin(tops), tops.shape))            # the lowest column
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    # the 2 x 2-voxel column (the unit the column tops and the sun horizon are kept in) that stands highest
    # over its 8 neighbours, below the cut and among the first 128 columns along x, where the camera is
    c2 = tops.reshape(Z // 2, 2, X // 2, 2).max(axis=(1, 3))                            # [cz, cx]
    pad = np.pad(c2, 1, constant_values=-1)
    around = np.max([pad[1 + j:1 + j + Z // 2, 1 + i:1 + i + X // 2] for j in (-1, 0, 1) for i in (-1, 0, 1)
                     if (i, j) != (0, 0)], axis=0)
    peak = np.where(c2 < 89, c2 - around, -1)[:, :64]
    dz, dx = (2 * int(v) for v in np.unravel_index(np.argmax(peak), peak.shape))
    dtop = int(c2[dz // 2, dx // 2])
    assert peak.max() > 0 and dtop >= 3
    steps = [[(lx, 120, lz, lx + 1, 121, lz + 1, 1)],            # high over the lowest column: the sky exit rises
             [(lx, 120, lz, lx + 1, 121, lz + 1, 0)],            # ... and drops again
             [(dx, dtop - 2, dz, dx + 2, dtop + 1, dz + 2, 0)]]  # the top 3 rows of the peak dug out: its column
    #                                                              top and the sun horizon behind it lower
    org, d, dist = random_rays(np.random.default_rng(4321), 20000, (X, Y, Z))
    for n, boxes in enumerate(steps, 1):
        prev = ow.csdf.copy()
        r.world_edit(boxes)
        twin_edit(rv, t, lg, boxes)
        ow.bits[:] = edited(ow.bits, lg, boxes)
        ow.build_csdf()
        _assert_local(rv, r, lg, boxes, n)
        bits, csdf = same_world(rv, r, t, boxes)
        assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf)
        print(f"{boxes}: local, {int((csdf != prev).sum())} CSDF bytes change")
        assert (csdf != prev).any()
        g, h = r.trace_rays(org, d, dist), t.trace_rays(org, d, dist)
        for f in g.dtype.names:
            assert np.array_equal(g[f].view(np.uint32), h[f].view(np.uint32)), (boxes, f)
        o = ow.trace_batch(org, d, dist)
        assert np.array_equal(g["hit"], o["hit"]) and np.array_equal(g["undef"], o["undef"])
        for f in ("pos", "normal", "u", "v"):
            assert np.array_equal(g[f].view(np.uint32), o[f].view(np.uint32)), (boxes, f)
        for c in (r, t):
            c.stats_reset()
            c.frame(cam, vp, flags=flags | rv.RV_F_STATS)
        for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_DEPTH, rv.RV_IMAGE_HALF_DIST, rv.RV_IMAGE_HALF_SHADOW):
            assert np.array_equal(r.readback(k), t.readback(k)), (boxes, k)
        assert r.stats() == t.stats(), boxes
        assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), _oracle_frame(rv, oracle, ow, cam, vp, flags)), boxes
    r.close()
    t.close()


@pytest.mark.parametrize("mode,in_flight", [("draw", 1), ("seq", 2), ("group", 1)])
def test_frames_across_a_local_edit(rv, atlas, mode, in_flight):
    """test_frames_across_an_edit of test_gpu_world_edit.py on T, where the edit rebuilds locally."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg = T_LG
    flags = rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2 * n, pan=0.01, ref_compat=True)
    r, t = _pair(rv, lg, None, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=4096)
    for c in (r, t):
        c.gi_update(0)
        if in_flight > 1:
            c.set_frames_in_flight(in_flight)
        if mode == "group":
            c.set_frame_group(4)
            assert c.frame_group_effective() == 4
    boxes, ray = block_in_view(r, seq[n], np.array([1 << l for l in lg]))
    hit0 = r.trace_rays(*ray)[0]["pos"].copy()

    def run(k0):
        if mode == "draw":
            for k in range(k0, k0 + n):
                for c in (r, t):
                    c.update_gi_data()
                    draw(c, seq[k])
                same_frames(rv, r, t, k)
        else:
            for c in (r, t):
                c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
            same_frames(rv, r, t, k0)
    run(0)
    gi = r.world_export(rv.RV_WORLD_GI)
    r.world_edit(boxes)
    twin_edit(rv, t, lg, boxes)
    _assert_local(rv, r, lg, boxes, 1)
    same_world(rv, r, t, "edit")
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), gi)   # the edit leaves the GI grid alone
    assert not np.array_equal(r.trace_rays(*ray)[0]["pos"], hit0)   # the placed block is on the ray
    run(n)
    assert r.flow_info()[2] == 0 and t.flow_info()[2] == 0
    if mode == "draw" and in_flight == 1:
        assert r.flow_info()[0] and r.flow_info()[1] == 2 * n
    r.close()
    t.close()


def _edited_terrain(rv, oracle, atlas, terrain, r):
    """world_edit(the blocks in view of pose P0) on r, a context holding T; the oracle world of the result
    with r's GI grid.  Returns (boxes, oracle world)."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg = T_LG
    seq = camera_path(TEST_POSES_128["P0"], W, H, 1, pan=0.01, ref_compat=True)
    boxes, _ = block_in_view(r, seq[0], np.array([1 << l for l in lg]))
    r.world_edit(boxes)
    _assert_local(rv, r, lg, boxes, 1)
    ow = oracle_of(oracle, lg, edited(terrain[0], lg, boxes), atlas=atlas)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), ow.bits)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
    assert not np.array_equal(ow.csdf, terrain[1])
    ow.gi[:] = r.world_export(rv.RV_WORLD_GI)
    return boxes, ow


def test_relight_after_a_local_edit(rv, oracle, atlas, terrain):
    from rvgrt_amd.configs import TEST_POSES_128
    lg = T_LG
    flags = rv.RV_FLAGS_REFERENCE
    r = rv.StateRender(lg, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=4096)
    r.world_build()
    r.gi_update(0)
    boxes, ow = _edited_terrain(rv, oracle, atlas, terrain, r)
    g0 = ow.gi.view(np.uint32).copy()
    box = rv.relight_box(lg, boxes, margin=4)
    want = expect_relight(ow, box, 700, 3, init=True)
    r.gi_relight(box, 700, 3, init=True)
    print(f"relight box {box}: {int((want != g0).sum())} cells change")
    assert (want != g0).any()
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI).view(np.uint32), want)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    r.frame(cam, vp, flags=flags)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), _oracle_frame(rv, oracle, ow, cam, vp, flags))
    r.close()


def test_gi_update_after_a_local_edit(rv, oracle, atlas, terrain):
    lg = T_LG
    r = rv.StateRender(lg, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas)
    r.world_build()
    boxes, ow = _edited_terrain(rv, oracle, atlas, terrain, r)
    g0 = ow.gi.view(np.uint32).copy()
    r.gi_update(5)
    ow.gi_update(5)
    want = ow.gi.view(np.uint32)
    assert (want != g0).any()
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI).view(np.uint32), want)
    r.close()


# ---------------------------------------------------------------- 4. two ranks: a local edit and a relight
def test_two_rank_loop_with_a_local_edit_and_a_relight(rv, atlas):
    """test_two_rank_loop_with_an_edit_equals_one_rank of test_gpu_world_edit.py on T: between two calls of
    the tile-sharded loop every rank, and the single context it is compared with, applies the same edit
    (rebuilt locally) and then the same relight of the edit's GI box."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, N = T_LG, 2
    flags = rv.RV_FLAGS_REFERENCE
    seq = camera_path(TEST_POSES_128["P0"], W, H, 8, pan=0.02, ref_compat=True)

    def make():
        c = rv.StateRender(lg, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=5000)
        c.world_build()
        c.gi_update(0)
        return c
    ref = make()
    ref.set_pipeline(0)
    group = rv.LoopbackGroup(N, timeout_ms=60000)
    rs = [make() for _ in range(N)]
    comms = []
    for q, c in enumerate(rs):
        c.set_tile_shard(32, q, N)
        comms.append(rv.Comm.loopback(c, group, q))
    boxes, _ = block_in_view(ref, seq[4], np.array([1 << l for l in lg]))
    box = rv.relight_box(lg, boxes, margin=4)
    for a, b in ((0, 4), (4, 8)):
        if a:
            before = ref.world_export(rv.RV_WORLD_GI)
            for c in rs + [ref]:
                c.world_edit(boxes)
                _assert_local(rv, c, lg, boxes, 1)
                c.gi_relight(box, 700, 3, init=True)
            relit = ref.world_export(rv.RV_WORLD_GI)
            assert not np.array_equal(relit, before)
            for q, c in enumerate(rs):
                assert np.array_equal(c.world_export(rv.RV_WORLD_GI), relit), q
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
            assert c.world_edit_info()[2] is False
    for m in comms:
        m.close()
    for c in rs:
        c.close()
    group.close()
    ref.close()


# ---------------------------------------------------------------- 5. scratch above 64 MiB
def _edit_packed(bits, lg, box):
    """The box written into the canonical bit words in place, without unpacking the world: whole planes
    at once where the box spans x and y, else one x run at a time."""
    X, Y, _ = (1 << l for l in lg)
    x0, y0, z0, x1, y1, z1, s = box
    if (x0, y0, x1, y1) == (0, 0, X, Y):
        bits[z0 * (X * Y // 32):z1 * (X * Y // 32)] = 0xFFFFFFFF if s else 0
        return
    for z in range(z0, z1):
        for y in range(y0, y1):
            for x in range(x0, x1):
                i = x | (y << lg[0]) | (z << (lg[0] + lg[1]))
                m = np.uint32(1 << (i & 31))
                bits[i >> 5] = (bits[i >> 5] | m) if s else (bits[i >> 5] & ~m)


def test_scratch_above_the_kept_size_is_freed_and_reserved_again(rv):
    """(10, 10, 9) is the smallest world in which an edit is local while the solid and dx boxes together
    (2 x 512 x 512 x 132 cells) exceed the 64 MiB of scratch a context keeps between edits: the first call
    frees its scratch, the second reserves it again from nothing, the third fits in what the second kept."""
    lg = (10, 10, 9)
    X, Y, Z = (1 << l for l in lg)
    r, t = _pair(rv, lg)
    bits = r.world_export(rv.RV_WORLD_BITS)
    assert np.array_equal(bits, t.world_export(rv.RV_WORLD_BITS))
    # the centre column's top: the generated terrain is far below y = Y / 2, where a clear would change nothing
    i = (X // 2) | (np.arange(Y, dtype=np.int64) << lg[0]) | ((Z // 2) << (lg[0] + lg[1]))
    col = (bits[i >> 5] >> (i & 31).astype(np.uint32)) & 1
    top = int(np.nonzero(col)[0].max())
    assert 2 <= top < Y - 2
    steps = [(0, 0, 0, X, Y, 8, 1),                                                # 512 x 512 x 4 cells
             (X // 2 - 1, top - 1, Z // 2 - 1, X // 2 + 2, top + 2, Z // 2 + 2, 0),  # 3 x 3 x 3 around that top
             (1, 1, 1, 2, 2, 2, 0)]                                                # one voxel of the first slab
    assert 2 * 512 * 512 * 132 > 64 << 20
    csdf = r.world_export(rv.RV_WORLD_CSDF)
    for n, box in enumerate(steps, 1):
        prev, prev_csdf = bits.copy(), csdf
        _edit_packed(bits, lg, box)
        assert not np.array_equal(bits, prev)
        r.world_edit([box])
        _assert_local(rv, r, lg, [box], n)
        t.world_import(rv.RV_WORLD_BITS, bits)
        t.csdf_build()
        got, csdf = same_world(rv, r, t, box)
        assert np.array_equal(got, bits)
        changed = int((csdf != prev_csdf).sum())
        print(f"{box}: local, {changed} CSDF bytes change")
        assert changed > 0 or n == 3   # one voxel of a solid slab: its coarse cell stays solid
    r.close()
    t.close()
