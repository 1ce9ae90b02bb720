"""rv_world_edit: voxel boxes set / cleared in place on the device, the CSDF
rebuilt only where the edit can reach, the early exits re-derived.  The yardstick
is a twin -- a second context driven through the same calls that receives
world_import(BITS, numpy-edited export) + csdf_build() where the first receives
world_edit -- and the oracle's set_solid + build_csdf.  Every comparison is
bit-exact."""
import numpy as np
import pytest

from conftest import random_rays
from gpu_world import (block_in_view, draw, edited, pack, run_ranks, rv, same_frames, same_world, sparse_bits,
                       twin_edit, voxels)
import np_shapes as S

pytestmark = pytest.mark.gpu

LONG_WORLDS = [(10, 6, 6), (6, 10, 6), (6, 6, 10)]


# ---------------------------------------------------------------- 1. locality and equality
@pytest.mark.parametrize("lg", LONG_WORLDS)
def test_local_rebuild_equals_full_rebuild(rv, oracle, lg):
    X, Y, Z = (1 << l for l in lg)
    ncells = X * Y * Z // 8
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = sparse_bits(lg, 1e-6, 77 + LONG_WORLDS.index(lg))
    ow.build_csdf()
    r, t = (rv.StateRender(lg, 64, 64) for _ in range(2))
    for c in (r, t):
        c.world_import(rv.RV_WORLD_BITS, ow.bits)
        c.csdf_build()
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
    cx, cy, cz = X // 2, Y // 2, Z // 2
    assert not ow.solid(cx, cy, cz)
    assert r.world_edit_info() == (0, 0, False)
    for step, solid in enumerate((1, 0)):
        box = [(cx, cy, cz, cx + 1, cy + 1, cz + 1, solid)]
        r.world_edit(box)
        twin_edit(rv, t, lg, box)
        ow.set_solid(cx, cy, cz, bool(solid))
        ow.build_csdf()
        bits, csdf = same_world(rv, r, t, (lg, solid))
        assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf), (lg, solid)
        region, cells = rv.edit_region(lg, box)
        assert r.world_edit_info() == (step + 1, cells, False)
        assert 0 < cells < ncells
    # boxes that straddle words, half-bricks and bricks, rebuilt locally around a several-cell extent
    boxes = [(cx - 3, cy - 5, cz - 1, cx + 6, cy + 2, cz + 8, 1), (cx - 1, cy - 4, cz, cx + 3, cy + 1, cz + 7, 0),
             (cx + 5, cy - 5, cz + 7, cx + 9, cy - 4, cz + 9, 1)]
    r.world_edit(boxes)
    twin_edit(rv, t, lg, boxes)
    ow.bits[:] = edited(ow.bits, lg, boxes)
    ow.build_csdf()
    bits, csdf = same_world(rv, r, t, (lg, "boxes"))
    assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf)
    assert r.world_edit_info() == (3, rv.edit_region(lg, boxes)[1], False)
    # setting what is already set changes nothing and counts as no edit
    r.world_edit(boxes[2:])
    assert r.world_edit_info() == (3, 0, False)
    same_world(rv, r, t, (lg, "repeat"))
    r.close()
    t.close()


# ---------------------------------------------------------------- 2. unaligned and overlapping boxes
def test_unaligned_overlapping_boxes_and_full_fallback(rv, oracle, oracle_world):
    lg = (7, 7, 7)
    N = 128
    r, t = (rv.StateRender(lg, 64, 64) for _ in range(2))
    for c in (r, t):
        c.world_build()
    bits0 = r.world_export(rv.RV_WORLD_BITS)
    base = oracle_world(7, 7, 7, gi_sweeps=0)
    assert np.array_equal(bits0, base.bits)
    # a coarse cell with all 8 voxels solid: clearing one of them leaves the cell solid
    full = voxels(bits0, lg).reshape(N // 2, 2, N // 2, 2, N // 2, 2).all(axis=(1, 3, 5))
    fz, fy, fx = (int(v[len(v) // 2]) for v in np.nonzero(full))
    boxes = [(5, 3, 7, 13, 9, 10, 1), (7, 4, 8, 11, 7, 9, 0)]
    for q in range(8):   # a one-voxel box at each world corner: bottom corners cleared, top corners set
        x, y, z = ((N - 1) * (q & 1), (N - 1) * ((q >> 1) & 1), (N - 1) * (q >> 2))
        boxes.append((x, y, z, x + 1, y + 1, z + 1, (q >> 1) & 1))
    boxes.append((2 * fx + 1, 2 * fy, 2 * fz + 1, 2 * fx + 2, 2 * fy + 1, 2 * fz + 2, 0))
    r.world_edit(boxes)
    assert r.world_edit_info()[2] is True   # 64^3 cells: every region covers the grid
    twin_edit(rv, t, lg, boxes)
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = edited(bits0, lg, boxes)
    ow.build_csdf()
    bits, csdf = same_world(rv, r, t, "boxes")
    assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf)
    assert r.world_edit_info()[0] == 1
    # a whole-world clear: the whole-grid build, an empty world
    clear = [(0, 0, 0, N, N, N, 0)]
    r.world_edit(clear)
    twin_edit(rv, t, lg, clear)
    bits, csdf = same_world(rv, r, t, "clear")
    assert not bits.any() and (csdf == 64).all()
    assert r.world_edit_info() == (2, N ** 3 // 8, True)
    r.close()
    t.close()


# ---------------------------------------------------------------- 3. exits follow the edit
def test_exits_follow_the_edit(rv, atlas, oracle, oracle_world):
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = (7, 7, 7), 160, 96
    N = 128
    flags = rv.RV_FLAGS_REFERENCE
    r, t = (rv.StateRender(lg, W, H, flags=flags, atlas=atlas) for _ in range(2))
    for c in (r, t):
        c.world_build()
    ow = oracle.OracleWorld(*lg, atlas=atlas)
    ow.bits[:] = oracle_world(7, 7, 7, gi_sweeps=0).bits
    vox = ow.voxels()
    top = int(np.nonzero(vox.any(axis=(0, 2)))[0].max())          # the highest solid row (the terrain is cut at 127)
    assert top > 90 and vox[:, 89, :].any()
    tops = np.where(vox.any(axis=1), N - 1 - np.argmax(vox[:, ::-1, :], axis=1), -1)   # [z, x]
    lz, lx = (int(v) for v in np.unravel_index(np.argmin(tops), tops.shape))            # the lowest column
    org, d, dist = random_rays(np.random.default_rng(4321), 20000, (N, N, N))
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    steps = [[(0, 90, 0, N, top + 1, N, 0)],                      # rows 90 .. the highest cleared: the sky exit must drop
             [(lx, N - 3, lz, lx + 1, N - 2, lz + 1, 1)]]         # ... and rise again, over the lowest column
    for boxes in steps:
        r.world_edit(boxes)
        twin_edit(rv, t, lg, boxes)
        ow.bits[:] = edited(ow.bits, lg, boxes)
        ow.build_csdf()
        bits, csdf = same_world(rv, r, t, boxes)
        assert np.array_equal(bits, ow.bits) and np.array_equal(csdf, ow.csdf)
        g, h = r.trace_rays(org, d, dist), t.trace_rays(org, d, dist)
        for f in g.dtype.names:
            assert np.array_equal(g[f].view(np.uint32), h[f].view(np.uint32)), (boxes, f)
        o = ow.trace_batch(org, d, dist)
        assert np.array_equal(g["hit"], o["hit"]) and np.array_equal(g["undef"], o["undef"])
        for f in ("pos", "normal", "u", "v"):
            assert np.array_equal(g[f].view(np.uint32), o[f].view(np.uint32)), (boxes, f)
        # the frame traversal takes the exits (sky exit, column skip, sun horizon): frames and step counts
        for c in (r, t):
            c.stats_reset()
            c.frame(cam, vp, flags=flags | rv.RV_F_STATS)
        for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_DEPTH, rv.RV_IMAGE_HALF_DIST, rv.RV_IMAGE_HALF_SHADOW):
            assert np.array_equal(r.readback(k), t.readback(k)), (boxes, k)
        assert r.stats() == t.stats(), boxes
    r.close()
    t.close()


# ---------------------------------------------------------------- 4. frames across an edit
@pytest.mark.parametrize("mode,in_flight", [("draw", 1), ("seq", 1), ("group", 1), ("draw", 2), ("seq", 2)])
def test_frames_across_an_edit(rv, atlas, mode, in_flight):
    """renderLoop's frames before and after an edit of a block in view: flow frames with the GI update
    computed ahead (draw), the pipelined loop with its kept pre-pass and GI update (seq), grouped frames
    (group); the work kept for the frame after the edit is discarded, as after any world write."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H = (7, 7, 7), 320, 192
    flags = rv.RV_FLAGS_REFERENCE
    n = 4 if mode == "group" else 3
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2 * n, pan=0.01, ref_compat=True)
    r, t = (rv.StateRender(lg, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=4096) for _ in range(2))
    for c in (r, t):
        c.world_build()
        c.gi_update(0)
        if in_flight > 1:
            c.set_frames_in_flight(in_flight)
        if mode == "group":
            c.set_frame_group(4)
            assert c.frame_group_effective() == 4
    boxes, ray = block_in_view(r, seq[n], 128)
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
    assert r.world_edit_info()[0] == 1
    same_world(rv, r, t, "edit")
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), gi)   # the edit leaves the GI grid alone
    assert not np.array_equal(r.trace_rays(*ray)[0]["pos"], hit0)   # the placed block is on the ray
    run(n)
    assert r.flow_info()[2] == 0 and t.flow_info()[2] == 0
    if mode == "draw" and in_flight == 1:
        assert r.flow_info()[0] and r.flow_info()[1] == 2 * n
    r.close()
    t.close()


# ---------------------------------------------------------------- 5. the word grid's edges
def _edge_spans(n, m):
    """(first, last) voxel pairs of an axis of n voxels whose ends take the residues that matter mod m (8 along
    x: 0, 1, 7; 4 along y: 0, 3) in the first and the last word of the axis."""
    return [(0, 0), (1, m - 1), (m - 1, m), (0, n - 1), (n - m, n - m + 1), (n - m + 1, n - 1), (n - 1, n - 1),
            (1, n - m), (m - 1, m - 1), (m, n - 2)]


@pytest.mark.parametrize("lg", [(5, 4, 4), (6, 5, 4)])
def test_word_grid_edges_of_the_three_writers(rv, lg):
    """The three kernels that run one lane per brick word of a voxel box (box edit, shape edit, detached clear)
    in the smallest windows where a wrong row or slice stride of the word grid, or a wrong half-brick (wy >> 1),
    shows: 32 x 16 x 16 and 64 x 32 x 16 voxels -- a 16-voxel axis is two bricks and four word rows.  Boxes and
    shapes start and end on every residue of a word along x and y at both window faces; each result is compared
    exactly with the host: edited(), np_shapes.apply, and rv_world_detached_at plus a clear of its mask."""
    X, Y, Z = (1 << l for l in lg)
    E = S.ELLIPSOID
    r, t = (rv.StateRender(lg, 64, 64) for _ in range(2))
    vox = np.random.default_rng(5 + lg[0]).random((Z, Y, X)) < 0.5
    r.world_import(rv.RV_WORLD_BITS, pack(vox))
    r.csdf_build()
    # 1. boxes: every x span with every y span, over one slice, a brick seam or all of z; later ones win
    xs, ys = _edge_spans(X, 8), _edge_spans(Y, 4)
    zs = [(0, 0), (Z - 1, Z - 1), (7, 8), (0, Z - 1)]
    boxes = [(xa, ya, zs[(i + j) % 4][0], xb + 1, yb + 1, zs[(i + j) % 4][1] + 1, (i + j) & 1)
             for i, (xa, xb) in enumerate(xs) for j, (ya, yb) in enumerate(ys)]
    boxes += [(7, Y - 1, Z - 1, 9, Y, Z, 0), (X - 1, Y - 1, Z - 1, X, Y, Z, int(not vox[Z - 1, Y - 1, X - 1]))]
    assert all(0 <= b[0] < b[3] <= X and 0 <= b[1] < b[4] <= Y for b in boxes)
    r.world_edit(boxes)
    bits = edited(pack(vox), lg, boxes)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), bits), "boxes"
    assert r.world_edit_info()[0] == 1
    # 2. shapes: a one-voxel and a radius-2 ellipsoid around both ends of every span, alternately set and cleared
    vox = voxels(bits, lg)
    at = [(x, y, z) for (xa, xb), (ya, yb), (za, zb) in zip(xs, ys, zs * 3) for x, y, z in ((xa, ya, za), (xb, yb, zb))]
    at += [(X - 1, Y - 1, Z - 1), (7, Y - 1, Z - 1), (8, 0, 0)]
    shapes = [(E, (i + k) & 1, (2 * x + 1, 2 * y + 1, 2 * z + 1), (r2,) * 3)
              for i, (x, y, z) in enumerate(at) for k, r2 in enumerate((4, 1))]
    want = S.apply(vox, shapes)
    assert r.world_edit_shapes(shapes) == want[1:] and want[1] > 0 and want[2] > 0
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(want[0])), "shapes"
    # 3. the clear: a floor, and above it voxel pairs that nothing holds -- across the word seam x = 7 | 8 in the
    # top corner of the window, across the word-row seam y = 3 | 4, across the brick seam z = 7 | 8
    vox = np.zeros((Z, Y, X), bool)
    vox[:, 0, :] = True
    vox[Z - 2, Y - 1, 7:9] = True
    vox[5, 3:5, 1] = True
    vox[7:9, Y - 4, X - 2] = True
    box = (0, 1, 0, X, Y, Z)
    r.world_import(rv.RV_WORLD_BITS, pack(vox))
    r.csdf_build()
    comps, n, v, mask = rv.detached_at(lg, pack(vox), box)
    assert (n, v) == (3, 6)
    got = r.world_detached(box, 1)
    assert got[1:3] == (n, v) and np.array_equal(got[3], mask)
    for f in ("seed", "lo", "hi", "voxels"):
        assert np.array_equal(got[0][f], comps[f]), f
    det = np.unpackbits(mask.view(np.uint8), bitorder="little")[:X * (Y - 1) * Z].reshape(Z, Y - 1, X).astype(bool)
    assert det.sum() == 6
    vox[:, 1:, :] &= ~det
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), pack(vox)), "clear"
    t.world_import(rv.RV_WORLD_BITS, pack(vox))
    t.csdf_build()
    same_world(rv, r, t, "after the clear")
    r.close()
    t.close()


# ---------------------------------------------------------------- 6. status behaviour
def test_edit_status_behaviour(rv):
    lg = (7, 6, 7)
    X, Y, Z = 128, 64, 128
    r = rv.StateRender(lg, 64, 64)
    with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
        r.world_edit([(0, 0, 0, 1, 1, 1, 1)])
    r.world_build()
    for solid in (1, 0):   # whatever the terrain holds there, one of the two changes it
        r.world_edit([(10, 50, 10, 14, 52, 13, solid)])
    assert r.world_edit_info()[0] >= 1
    bits, csdf = r.world_export(rv.RV_WORLD_BITS), r.world_export(rv.RV_WORLD_CSDF)
    info = r.world_edit_info()
    r.world_edit([])
    assert r.world_edit_info() == info
    good = (20, 40, 20, 24, 44, 24, 1)
    bad = [(4, 4, 4, 4, 5, 5, 1), (4, 4, 4, 5, 3, 5, 1), (4, 4, 4, 5, 5, 4, 1), (-1, 0, 0, 1, 1, 1, 1),
           (0, 0, 0, X + 1, 1, 1, 0), (0, 0, 0, 1, Y + 1, 1, 0), (0, 0, Z, 1, 1, Z + 1, 1), (0, 0, 0, 1, 1, 1, 2)]
    for b in bad:
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_edit([good, b])   # validated before anything is written: the good box is not applied
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        r.world_edit([good] * (rv._lib.RV_EDIT_MAX_BOXES + 1))
    assert r.world_edit_info() == info
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), bits)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), csdf)
    r.close()


# ---------------------------------------------------------------- 7. two-rank loopback
def test_two_rank_loop_with_an_edit_equals_one_rank(rv, atlas):
    """Both ranks of a tile-sharded loop apply the same edit between two calls: the gathered frame and
    every rank's GI grid equal one context rendering whole frames one at a time with the same edit."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H, N = (7, 7, 7), 320, 192, 2
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
    boxes, _ = block_in_view(ref, seq[4], 128)
    for a, b in ((0, 4), (4, 8)):
        if a:
            for c in rs + [ref]:
                c.world_edit(boxes)
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
