"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Bar: bit-exact for the integer/byte world data (bits, CSDF, GI) and for the
traversal (hit flag, voxel, position, normal, uv, step counts) -- both sides
use separately rounded IEEE float ops.  Frames: RGBA8, MV and depth
bit-exact as well (ocml's powf has matched glibc's on every pixel so far).
The SURVEY.md s8c tolerance (|d| <= 2 LSB on >= 99.5 % of pixels) is kept
for the reference's own compiled arithmetic -- FMA contraction, CUDA's
tanf/powf -- and priced in tests/test_r9_numerics.py.
"""
import numpy as np
import pytest

from conftest import Hip as _Hip, random_rays
from gpu_world import ZERO_SEED_CELL, ZERO_SEED_FRAME, rv

pytestmark = pytest.mark.gpu


def _gpu_world(rv, atlas, lx, ly, lz, W=64, H=64, flags=None, seed=(0, 0), gi_sweeps=1):
    r = rv.StateRender((lx, ly, lz), W, H, flags=rv.RV_FLAGS_REFERENCE if flags is None else flags,
                       atlas=atlas, seed=seed)
    r.world_build()
    for s in range(max(gi_sweeps, 0)):
        r.gi_update(s)
    return r


@pytest.mark.parametrize("dims,seed", [((6, 6, 6), (0, 0)), ((7, 6, 7), (0, 0)), ((7, 7, 7), (0, 0)),
                                       ((6, 7, 5), (1000, -300))])
def test_world_build_bit_exact(rv, atlas, oracle_world, dims, seed):
    lx, ly, lz = dims
    ow = oracle_world(lx, ly, lz, gi_sweeps=0, seed=seed)
    r = _gpu_world(rv, atlas, lx, ly, lz, seed=seed, gi_sweeps=0)
    bits = r.world_export(rv.RV_WORLD_BITS)
    assert np.array_equal(bits, ow.bits), "voxel bits differ"
    csdf = r.world_export(rv.RV_WORLD_CSDF)
    assert np.array_equal(csdf, ow.csdf), f"CSDF differs at {np.flatnonzero(csdf != ow.csdf)[:10]}"
    gi = r.world_export(rv.RV_WORLD_GI)
    assert np.array_equal(gi, ow.gi), "GI init differs"
    r.close()


def test_gi_sweeps_bit_exact(rv, atlas, oracle_world, oracle):
    ow = oracle_world(7, 7, 7, gi_sweeps=2)
    r = _gpu_world(rv, atlas, 7, 7, 7, gi_sweeps=2)
    gi = r.world_export(rv.RV_WORLD_GI)
    assert np.array_equal(gi, ow.gi)
    # partial (rolling-window) update, UpdateGIData style
    w2 = oracle.OracleWorld(7, 7, 7, atlas=atlas)
    w2.bits[:] = ow.bits; w2.csdf[:] = ow.csdf; w2.gi[:] = ow.gi
    w2.gi_update(5, first=1000, count=3000)
    r.gi_update(5, first=1000, count=3000)
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), w2.gi)
    r.close()


def test_gi_update_zero_rng_state(rv, atlas, oracle_world, oracle):
    """The cell whose xorshift state idx + frame * 198491317 wraps to 0
    (tests/gpu_world.py ZERO_SEED_*): the update terminates and agrees
    with the oracle (a zero state once hung the GPU, 476 frames into a C4 run)."""
    ow = oracle_world(6, 6, 6, gi_sweeps=1)
    r = _gpu_world(rv, atlas, 6, 6, 6, gi_sweeps=1)
    w2 = oracle.OracleWorld(6, 6, 6, atlas=atlas)
    w2.bits[:] = ow.bits; w2.csdf[:] = ow.csdf; w2.gi[:] = ow.gi
    w2.gi_update(ZERO_SEED_FRAME, first=ZERO_SEED_CELL - 40, count=80)
    r.gi_update(ZERO_SEED_FRAME, first=ZERO_SEED_CELL - 40, count=80)
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), w2.gi)
    r.close()


def test_import_export_roundtrip(rv, atlas, oracle_world):
    ow = oracle_world(6, 6, 6, gi_sweeps=1)
    r = rv.StateRender((6, 6, 6), 64, 64, atlas=atlas)
    r.world_import(rv.RV_WORLD_BITS, ow.bits)
    r.csdf_build()
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), ow.bits)
    assert np.array_equal(r.world_export(rv.RV_WORLD_CSDF), ow.csdf)
    r.world_import(rv.RV_WORLD_CSDF, ow.csdf)
    r.world_import(rv.RV_WORLD_GI, ow.gi)
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ow.gi)
    r.close()


@pytest.mark.parametrize("dims", [(7, 7, 7), (8, 6, 7)])
def test_trace_bit_exact(rv, atlas, oracle_world, dims):
    ow = oracle_world(*dims, gi_sweeps=0)
    r = rv.StateRender(dims, 64, 64, atlas=atlas)
    r.world_import(rv.RV_WORLD_BITS, ow.bits)
    r.world_import(rv.RV_WORLD_CSDF, ow.csdf)
    rng = np.random.default_rng(1234)
    org, d, dist = random_rays(rng, 20000, (ow.X, ow.Y, ow.Z))
    g = r.trace_rays(org, d, dist)
    o = ow.trace_batch(org, d, dist)
    assert (g["hit"] == o["hit"]).all()
    assert (g["undef"] == o["undef"]).all()
    assert np.array_equal(g["pos"].view(np.uint32), o["pos"].view(np.uint32))
    assert np.array_equal(g["normal"], o["normal"])
    assert np.array_equal(g["u"].view(np.uint32), o["u"].view(np.uint32))
    assert np.array_equal(g["v"].view(np.uint32), o["v"].view(np.uint32))
    assert np.array_equal(g["sphere_steps"], o["n_sphere"])
    assert np.array_equal(g["dda_steps"], o["n_dda"])
    assert np.array_equal(g["csdf_checks"], o["n_check"])
    assert g["hit"].mean() > 0.2
    r.close()


FRAME_CASES = [("c1", 0), ("c2", 8), ("ref", 7)]


@pytest.mark.parametrize("name,flags", FRAME_CASES)
@pytest.mark.parametrize("pose", ["P0", "P1"])
def test_frame_parity(rv, atlas, oracle_world, oracle, name, flags, pose):
    lg = 7
    W, H = 256, 144
    ow = oracle_world(lg, lg, lg, gi_sweeps=1)
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    from rvgrt_amd.configs import TEST_POSES_128
    pos, yaw, pitch = TEST_POSES_128[pose]
    cam, vp = rv.camera_from_pose(pos, yaw, pitch, W, H)
    ocam = oracle.camera_from_pose(pos, yaw, pitch, W, H)
    for k in ("pos", "fo", "ri", "up", "vp"):   # host camera math agrees bit for bit
        assert np.array_equal(rv.camera_dict(cam, vp)[k], ocam[k]), k
    r.stats_reset()
    r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
    gpu = r.readback(rv.RV_IMAGE_COLOR)
    gmv = r.readback(rv.RV_IMAGE_MOTION)
    gdep = r.readback(rv.RV_IMAGE_DEPTH)
    st = r.stats()
    ref = oracle.render(ow, oracle.make_frame(W, H, flags, ocam))
    diff = np.abs(gpu.astype(np.int32) - ref["rgba"].astype(np.int32)).max(axis=2)
    assert diff.max() == 0, f"{int((diff > 0).sum())} pixels differ, max |d| = {diff.max()}"
    assert np.array_equal(gdep, ref["depth"])
    assert np.array_equal(gmv, ref["mv"])
    if flags & 1:
        hd = r.readback(rv.RV_IMAGE_HALF_DIST)
        assert np.array_equal(hd.view(np.uint32), ref["halfdist"].view(np.uint32))
    os_ = ref["stats"]
    for k in ("traces", "primary", "shadow", "refl", "refl_shadow", "prepass_primary", "prepass_shadow",
              "cones", "cone_steps", "undef_hits"):
        assert st[k] == os_[k], (k, st[k], os_[k])
    for k in ("sphere_steps", "dda_steps", "csdf_checks"):   # <=: the sky exit (test_sky_exit_frames_and_gi)
        assert st[k] <= os_[k], (k, st[k], os_[k])
    r.close()


@pytest.mark.parametrize("flags", [8, 7])
def test_frame_tiles_match_full_frame(rv, atlas, flags):
    lg = 7
    W, H = 256, 160
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    from rvgrt_amd.configs import TEST_POSES_128
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    r.frame(cam, vp)
    full = r.readback(rv.RV_IMAGE_COLOR).copy()
    T = 32
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    ids_all = np.arange(tiles_x * tiles_y, dtype=np.int32)
    # three "ranks" (fresh contexts: no half-res data from the full frame)
    # render interleaved tiles; each rank's packed tile buffer is scattered
    # into a fourth context's image (the rank-0 gather side)
    sink = rv.StateRender((lg, lg, lg), W, H, flags=flags, atlas=atlas)
    for rank in range(3):
        rr = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
        ids = ids_all[rank::3]
        rr.frame_tiles(cam, vp, ids, tile_px=T)
        rr.sync()
        p, nbytes = rr.tile_buffer()
        assert nbytes >= len(ids) * T * T * 4
        sink.untile(p, ids, tile_px=T)
        sink.sync()
        rr.close()
    out = sink.readback(rv.RV_IMAGE_COLOR)
    assert np.array_equal(out, full)
    sink.close()
    r.close()


@pytest.mark.parametrize("flags", [8, 7])
def test_cost_ordering_keeps_frames_identical(rv, atlas, flags):
    """SCHED_COST re-deals chunks/tiles every 4th frame from measured wave
    lifetimes; the order changes, the pixels must not.  Also: untile skips
    padding slots (id -1) of a gathered buffer."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H, T = 7, 320, 192, 64
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P1"], W, H)
    imgs = []
    for _ in range(9):
        r.frame(cam, vp)
        imgs.append(r.readback(rv.RV_IMAGE_COLOR).copy())
    for im in imgs[1:]:
        assert np.array_equal(im, imgs[0])
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    ids = np.arange(tiles_x * tiles_y, dtype=np.int32)[1::2]
    sink = rv.StateRender((lg, lg, lg), W, H, flags=flags, atlas=atlas)
    for k in range(9):
        r.frame_tiles(cam, vp, ids, tile_px=T)
        r.sync()
        p, _ = r.tile_buffer()
        sink.untile(p, np.concatenate([ids, np.full(3, -1, np.int32)]), tile_px=T)
        sink.sync()
        out = sink.readback(rv.RV_IMAGE_COLOR)
        for t in ids:
            ty, tx = divmod(int(t), tiles_x)
            ys, xs = slice(ty * T, min(H, ty * T + T)), slice(tx * T, min(W, tx * T + T))
            assert np.array_equal(out[ys, xs], imgs[0][ys, xs]), (k, t)
    sink.close()
    r.close()


def test_draw_cuda_ref_compat(rv, atlas):
    """drawCUDA signature: with ref_compat, time<-jitterY, jitter<-(0, oob)."""
    lg = 6
    W, H = 64, 48
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=7)
    cam, vp = rv.camera_from_pose((60.0, 50.0, 60.0), 2.44, -3.4415927, W, H)
    d = rv.camera_dict(cam, vp)
    r.draw_cuda(d["pos"], d["fo"], d["up"], d["ri"], vp, vp, 0.3, 0.0)
    a = r.readback(rv.RV_IMAGE_COLOR).copy()
    r.frame(cam, vp, time=0.0, jx=0.0, jy=0.0, flags=7)
    b = r.readback(rv.RV_IMAGE_COLOR)
    assert np.array_equal(a, b)   # jitterX ignored, time = jitterY = 0
    r.close()


def test_golden_fixtures(rv, atlas):
    """World hashes and 256 traced rays from tests/golden (oracle-made), bit-exact."""
    import hashlib
    import json
    import os
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    g = json.load(open(os.path.join(gdir, "golden.json")))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for lg in (6, 7):
        r = rv.StateRender((lg, lg, lg), 64, 64, atlas=atlas)
        r.world_build()
        ref = g["worlds"][f"{1 << lg}^3"]
        assert sha(r.world_export(rv.RV_WORLD_BITS)) == ref["bits"]
        assert sha(r.world_export(rv.RV_WORLD_CSDF)) == ref["csdf"]
        assert sha(r.world_export(rv.RV_WORLD_GI)) == ref["gi_init"]
        r.gi_update(0)
        assert sha(r.world_export(rv.RV_WORLD_GI)) == ref["gi_after_1_sweep"]
        if lg == 7:
            t = np.load(os.path.join(gdir, "traces_128.npz"))
            h = r.trace_rays(t["org"], t["dir"], t["dist"])
            assert np.array_equal(h["hit"], t["hit"]) and np.array_equal(h["undef"], t["undef"])
            assert np.array_equal(h["pos"].view(np.uint32), t["pos"].view(np.uint32))
            assert np.array_equal(h["normal"], t["normal"])
            assert np.array_equal(h["u"], t["u"]) and np.array_equal(h["v"], t["v"])
            assert np.array_equal(h["dda_steps"], t["n_dda"])
        r.close()


def test_golden_frames(rv, atlas):
    """The six golden frames of tests/golden (160x96 on the 128^3 world, C1 /
    C2 / reference flags, poses P0 / P1): MV and depth hashes and the work
    counters equal the fixture exactly; RGBA8 hashes equal the fixture's (the
    decoded PNG is compared first for a readable failure)."""
    import hashlib
    import json
    import os
    from rvgrt_amd.atlas import decode_png
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    g = json.load(open(os.path.join(gdir, "golden.json")))
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    r = None
    exact = 0
    for key, fr in sorted(g["frames"].items()):
        W, H = (int(v) for v in key.split("_")[1].split("x"))
        if r is None:
            r = _gpu_world(rv, atlas, 7, 7, 7, W, H, gi_sweeps=1)
        pos, yaw, pitch = fr["pose"]
        cam, vp = rv.camera_from_pose(pos, yaw, pitch, W, H)
        r.stats_reset()
        r.frame(cam, vp, flags=fr["flags"] | rv.RV_F_STATS)
        img = r.readback(rv.RV_IMAGE_COLOR)
        assert sha(r.readback(rv.RV_IMAGE_MOTION)) == fr["mv"], key
        assert sha(r.readback(rv.RV_IMAGE_DEPTH)) == fr["depth"], key
        st = r.stats()
        for k, v in fr["stats"].items():   # the step counts of the full march, or fewer (the sky / sun exits)
            assert (st[k] <= v) if k in ("sphere_steps", "dda_steps", "csdf_checks") else (st[k] == v), (key, k, st[k], v)
        with open(os.path.join(gdir, f"{key}.png"), "rb") as f:
            want = decode_png(f.read())
        d = np.abs(img.astype(np.int32) - want.astype(np.int32)).max(axis=2)
        assert d.max() == 0, (key, int((d > 0).sum()), int(d.max()))
        assert sha(img) == fr["rgba"], key
        exact += 1
    assert exact == len(g["frames"]) == 6
    r.close()


@pytest.mark.parametrize("flags", [0, 8, 7])
def test_wavefront_equals_per_pixel_path(rv, atlas, flags):
    """The wavefront stages and the per-pixel (megakernel) path are two
    schedules of the same arithmetic: images and counters are identical."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = 7, 320, 192
    out = {}
    for mk in ("0", "1"):
        r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
        r.set_frame_path("fused" if mk == "1" else "wavefront")
        for pose in ("P0", "P1"):
            cam, vp = rv.camera_from_pose(*TEST_POSES_128[pose], W, H)
            r.stats_reset()
            r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
            out[(mk, pose)] = (r.readback(rv.RV_IMAGE_COLOR).copy(), r.readback(rv.RV_IMAGE_MOTION).copy(),
                               r.readback(rv.RV_IMAGE_DEPTH).copy(), r.stats())
        r.close()
    for pose in ("P0", "P1"):
        a, b = out[("0", pose)], out[("1", pose)]
        for k in range(3):
            assert np.array_equal(a[k], b[k]), (pose, k)
        assert a[3] == b[3]


def test_gi_async_update_matches_serial_and_oracle(rv, atlas, oracle_world):
    """rv_update_gi_data on the side stream (overlapping the previous frame's
    render) gives the same grid and images as the serial order, and the grid
    matches the oracle's partial updates (RAYPS-style rolling offset)."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H, rays = 7, 320, 192, 5000
    ow = oracle_world(lg, lg, lg, gi_sweeps=1)
    n = len(ow.gi) // 4
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    res = {}
    for on in (0, 1):
        r = rv.StateRender((lg,) * 3, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, gi_rays_per_frame=rays)
        r.world_build()
        r.gi_update(0)
        r.set_gi_async(on)
        imgs = []
        for k in range(9):          # wraps the rolling offset once (32768 cells)
            r.update_gi_data()
            r.frame(cam, vp)
            # read back every 4th frame only, so most updates are queued
            # behind a still-running render
            imgs.append(r.readback(rv.RV_IMAGE_COLOR).copy() if k % 4 == 0 else None)
        r.sync()
        res[on] = (r.world_export(rv.RV_WORLD_GI), imgs)
        r.close()
    assert np.array_equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert (a is None and b is None) or np.array_equal(a, b)
    off = 0
    for k in range(9):              # oracle: the same rolling partial updates
        ow.gi_update(k, first=off, count=min(rays, n - off))
        off = 0 if off + rays >= n else off + rays
    assert np.array_equal(res[1][0], ow.gi)


@pytest.mark.parametrize("flags", [8, 7])
def test_frames_in_flight_identical(rv, atlas, flags):
    """rv_set_frames_in_flight: frames submitted on alternating streams, each
    in its own frame slot (images, half-res images, scheduling state), render
    concurrently and equal the one-at-a-time frame in colour, MV and depth;
    per-frame GI updates (flags 7) wait for the frames in flight.  Also the
    tile path with one tile buffer per slot."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H, T = 7, 320, 192, 64
    hip = _Hip()
    ref = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    r.set_frames_in_flight(3)
    streams = [hip.stream() for _ in range(3)]
    gi = bool(flags & rv.RV_F_GI)
    kinds = (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH)
    for k in range(7):
        if gi:
            ref.update_gi_data()
        ref.frame(cam, vp)
        want = [ref.readback(kind).copy() for kind in kinds]
        r.set_stream(streams[k % 3])
        if gi:
            r.update_gi_data()
        r.frame(cam, vp)
        if k % 2 == 0:   # read back some frames while others are in flight
            for kind, b in zip(kinds, want):
                assert np.array_equal(r.readback(kind), b), (k, kind)
    r.sync()
    if not gi:   # tiles: three slots, three tile buffers, untiled into a sink
        tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
        ids = np.arange(tiles_x * tiles_y, dtype=np.int32)
        nbytes = len(ids) * T * T * 4
        bufs = [hip.malloc(nbytes) for _ in range(3)]
        sink = rv.StateRender((lg, lg, lg), W, H, flags=flags, atlas=atlas)
        for k in range(6):
            r.set_stream(streams[k % 3])
            r.bind_tile_buffer(bufs[k % 3], nbytes)
            r.frame_tiles(cam, vp, ids, tile_px=T)
        r.sync()
        for k in range(3):
            sink.untile(bufs[k], ids, tile_px=T)
            sink.sync()
            assert np.array_equal(sink.readback(rv.RV_IMAGE_COLOR), want[0]), k
        sink.close()
    with pytest.raises(rv.RvError):
        r.set_frame_path("wavefront")   # one frame at a time only
    r.set_frames_in_flight(1)
    r.set_stream(0)
    r.close()
    ref.close()
    hip.close()


@pytest.mark.parametrize("flags,T", [(8, 16), (8, 64), (7, 32), (7, 16)])
def test_render_frames_native_loop(rv, atlas, flags, T):
    """rv_render_frames: the native loop over 3 frame slots equals frames
    rendered one at a time -- whole frames, a one-rank tile shard assembled
    locally, and the same shard gathered through a one-rank RCCL
    communicator (the multi-GPU code path with no peers)."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = 7, 320, 192
    gi = bool(flags & rv.RV_F_GI)
    ref = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P1"], W, H)
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    r.set_frames_in_flight(3)

    def ref_frames(n):
        for _ in range(n):
            if gi:
                ref.update_gi_data()
            ref.frame(cam, vp)
        return ref.readback(rv.RV_IMAGE_COLOR).copy()

    r.render_frames(5, cam, vp, gi_per_frame=gi)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref_frames(5))
    r.set_tile_shard(T, 0, 1)
    r.render_frames(4, cam, vp, gi_per_frame=gi)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref_frames(4))
    comm = rv.Comm(r, rv.Comm.unique_id(), 1, 0)
    r.render_frames(7, cam, vp, gi_per_frame=gi, comm=comm)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref_frames(7))
    with pytest.raises(rv.RvError):   # shard / communicator mismatch
        r.set_tile_shard(T, 0, 2)
        r.render_frames(1, cam, vp, comm=comm)
    comm.close()
    r.close()
    ref.close()


@pytest.mark.parametrize("order,rays,pairs", [("012", 5000, 0), ("210", 5000, 0), ("102", 5000, 0), ("102", 4096, 0),
                                              ("012", 2048, 0), ("102", 5000, 1), ("102", 4096, 1)])
def test_pipelined_reference_frames(rv, atlas, oracle, monkeypatch, order, rays, pairs):
    """rv_set_pipeline: render k | GI update k+1 | pre-pass k+1 in one launch.
    The frames and the GI grid equal UpdateGIData + drawCUDA one frame at a
    time, for every dispatch order of the parts, over a rolling GI window
    that wraps (5000-cell windows of a 32^3 grid: linear cell order, a partial
    last block; 4096 / 2048: whole planes, blocked cell order) -- and the
    oracle agrees on the grid (bit-exact) and the last frame.  pairs: the latency variant's GI cells on
    lane pairs (RV_OPT_GI_PAIRS; this small frame's launches are latency-variant ones)."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = 7, 320, 192
    flags = rv.RV_FLAGS_REFERENCE
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)

    def make():
        r = rv.StateRender((lg, lg, lg), W, H, flags=flags, atlas=atlas, gi_rays_per_frame=rays)
        r.set_option(rv.RV_OPT_PIPE_ORDER, int(order, 16))
        r.set_option(rv.RV_OPT_GI_PAIRS, pairs)
        r.world_build()
        r.gi_update(0)
        return r
    ref, r = make(), make()
    ref.set_pipeline(0)
    for n in (1, 2, 5, 3):   # 11 frames: 2 wraps of the 32768-cell grid at 5000 cells per frame
        r.render_frames(n, cam, vp, gi_per_frame=True)
        for _ in range(n):
            ref.update_gi_data()
            ref.frame(cam, vp)
        assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref.readback(rv.RV_IMAGE_COLOR)), n
        assert np.array_equal(r.readback(rv.RV_IMAGE_DEPTH), ref.readback(rv.RV_IMAGE_DEPTH)), n
        assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ref.world_export(rv.RV_WORLD_GI)), n
    # the oracle: same updates (frame numbers 0.., rolling window), same last frame
    ow = oracle.OracleWorld(lg, lg, lg, atlas=atlas).build(gi_sweeps=1)
    ngi, off = (1 << (lg - 2)) ** 3, 0
    for fno in range(11):
        ow.gi_update(fno, first=off, count=min(rays, ngi - off))
        off = 0 if off + rays >= ngi else off + rays
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ow.gi)
    ref_img = oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)))["rgba"]
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref_img)
    assert np.array_equal(r.readback(rv.RV_IMAGE_HALF_DIST), ref.readback(rv.RV_IMAGE_HALF_DIST))
    r.close()
    ref.close()


def test_pipelined_frames_stats(rv, atlas):
    """A pipelined launch with RV_F_STATS counts its three parts into their
    own stage blocks: the render's traces equal a one-at-a-time frame's."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = 7, 160, 96
    flags = rv.RV_FLAGS_REFERENCE | rv.RV_F_STATS
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H)
    r.stats_reset()
    r.frame(cam, vp, flags=flags)
    one = {k: r.stats(k) for k in range(8)}
    r.stats_reset()
    r.render_frames(3, cam, vp, flags=flags, gi_per_frame=True)
    three = {k: r.stats(k) for k in range(8)}
    assert three[2]["traces"] == 3 * one[2]["traces"]          # render: 3 frames
    # pre-pass: frame 0, frames 1 and 2 pipelined, and frame 3's, kept for the next call
    assert three[0]["traces"] == 4 * one[0]["traces"]
    assert three[7]["gi_traces"] > 0
    r.close()


def test_render_frames_two_streams(rv, atlas, monkeypatch):
    """RV_OPT_BATCH_STREAMS = 2 (what bench.py uses with N > 1): groups alternate over
    two streams so one group's tail overlaps the next; frames must not change --
    whole frames, a one-rank shard and the one-rank RCCL gather path."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H, T = 7, 320, 192, 16
    ref = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=8, gi_sweeps=1)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P1"], W, H)
    ref.frame(cam, vp)
    want = ref.readback(rv.RV_IMAGE_COLOR).copy()
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=8, gi_sweeps=1)
    r.set_option(rv.RV_OPT_BATCH_STREAMS, 2)
    r.set_frames_in_flight(4)
    r.render_frames(11, cam, vp)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), want)
    r.set_tile_shard(T, 0, 1)
    r.render_frames(9, cam, vp)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), want)
    comm = rv.Comm(r, rv.Comm.unique_id(), 1, 0)
    r.render_frames(13, cam, vp, comm=comm)
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), want)
    comm.close()
    r.close()
    ref.close()


def _frame_one(ref, rv, d, flags, gi):
    """One frame of a sequence the reference's way: UpdateGIData, then the frame."""
    if gi:
        ref.update_gi_data()
    ref.frame(d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp), time=d.time, jx=d.jitter_x,
              jy=d.jitter_y, flags=flags)


def _images(r, rv):
    return [r.readback(k).copy() for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH)]


@pytest.mark.parametrize("jitter", ["ref_compat", "rays"])
def test_frame_seq_pipelined_moving_camera(rv, atlas, oracle, jitter):
    """rv_render_frame_seq on the pipelined reference loop with a moving
    camera (yaw pan, the jitter sequence as time or as ray jitter, previous
    VP = the previous frame's): frames, motion vectors and the GI grid equal
    one-at-a-time frames after every call.  The next frame's update and
    pre-pass kept between calls are used when the next call starts where the
    last ended, dropped when it does not (a different camera) or when a GI
    write came in between."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H, rays = 7, 320, 192, 5000
    flags = rv.RV_FLAGS_REFERENCE
    seq = camera_path(TEST_POSES_128["P0"], W, H, 14, pan=0.02, ref_compat=jitter == "ref_compat")

    def make():
        r = rv.StateRender((lg,) * 3, W, H, flags=flags, atlas=atlas, gi_rays_per_frame=rays)
        r.world_build()
        r.gi_update(0)
        return r
    ref, r = make(), make()
    ref.set_pipeline(0)
    # (first, end, next index): kept work used (calls 1, 2), pre-pass kept for seq[8] but the next call
    # starts at seq[9] (call 3: update used, pre-pass recomputed), a GI write before call 4 (update
    # recomputed, pre-pass used)
    calls = [(0, 3, 3), (3, 7, 7), (7, 9, None), (9, 11, 11), (11, 14, None)]
    for i, (a, b, nxt) in enumerate(calls):
        if i == 4:   # a GI write between calls: the kept update is stale
            r.gi_update(9, first=100, count=300)
            ref.gi_update(9, first=100, count=300)
        r.render_frame_seq(seq[a:b], next_desc=seq[nxt] if nxt is not None else None, gi_per_frame=True)
        for k in range(a, b):
            _frame_one(ref, rv, seq[k], flags, True)
        for x, y in zip(_images(r, rv), _images(ref, rv)):
            assert np.array_equal(x, y), (a, b)
        assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ref.world_export(rv.RV_WORLD_GI)), (a, b)
    assert np.abs(r.readback(rv.RV_IMAGE_MOTION).view(np.float16).astype(np.float32)).max() > 0   # camera moved
    r.close()
    ref.close()


@pytest.mark.parametrize("flags", [0, 8])
def test_frame_seq_batched_moving_camera(rv, atlas, flags):
    """Batched groups (no per-frame GI update) with a camera per frame: the
    group launch reads each frame's camera from the device table; the last
    frame of sequences of several lengths (whole groups, a partial group,
    equal split groups) equals that frame rendered alone -- whole frames, a
    one-rank tile shard and the one-rank RCCL gather path."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H = 7, 320, 192
    seq = camera_path(TEST_POSES_128["P1"], W, H, 21, pan=0.03, ref_compat=False)
    ref = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    r = _gpu_world(rv, atlas, lg, lg, lg, W, H, flags=flags, gi_sweeps=1)
    r.set_frames_in_flight(4)
    for shard in ("none", "one_rank", "rccl"):
        comm = None
        if shard == "one_rank":
            r.set_tile_shard(16, 0, 1)
        elif shard == "rccl":
            comm = rv.Comm(r, rv.Comm.unique_id(), 1, 0)
        for n in (4, 7, 21):
            r.render_frame_seq(seq[:n], flags=flags, comm=comm)
            _frame_one(ref, rv, seq[n - 1], flags, False)
            assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref.readback(rv.RV_IMAGE_COLOR)), (shard, n)
            if shard == "none":
                assert np.array_equal(r.readback(rv.RV_IMAGE_MOTION), ref.readback(rv.RV_IMAGE_MOTION)), n
                assert np.array_equal(r.readback(rv.RV_IMAGE_DEPTH), ref.readback(rv.RV_IMAGE_DEPTH)), n
        if comm is not None:
            comm.close()
    r.close()
    ref.close()


@pytest.mark.parametrize("pose", ["P0", "P1"])
def test_sky_exit_frames_and_gi(rv, atlas, oracle, pose):
    """The frame traversal's sky exit (World::ytop = highest solid row + 2,
    recomputed on every bits write): on a 128^3 world with open sky above
    y = 90 (rows cleared, CSDF rebuilt, imported through rv_world_import), the
    reference frame (RGBA8, motion, depth, half-res distance) and a GI update
    equal the oracle's full march bit for bit, with the same trace and cone
    counts and fewer sphere steps; rv_trace_rays keeps the reference's step
    counts exactly."""
    from rvgrt_amd.configs import TEST_POSES_128
    lg, W, H = 7, 256, 144
    flags = rv.RV_FLAGS_REFERENCE
    ow = oracle.OracleWorld(lg, lg, lg, atlas=atlas).build(gi_sweeps=1)
    vox = ow.voxels()
    vox[:, 90:, :] = False
    ow.bits[:] = np.packbits(vox.ravel(), bitorder="little").view(np.uint32)
    ow.build_csdf()
    r = rv.StateRender((lg,) * 3, W, H, flags=flags, atlas=atlas)
    r.world_import(rv.RV_WORLD_BITS, ow.bits)
    r.world_import(rv.RV_WORLD_CSDF, ow.csdf)
    r.world_import(rv.RV_WORLD_GI, ow.gi)
    cam, vp = rv.camera_from_pose(*TEST_POSES_128[pose], W, H)
    r.stats_reset()
    r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
    st = r.stats()
    ref = oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)))
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref["rgba"])
    assert np.array_equal(r.readback(rv.RV_IMAGE_MOTION), ref["mv"])
    assert np.array_equal(r.readback(rv.RV_IMAGE_DEPTH), ref["depth"])
    assert np.array_equal(r.readback(rv.RV_IMAGE_HALF_DIST).view(np.uint32), ref["halfdist"].view(np.uint32))
    os_ = ref["stats"]
    for k in ("traces", "primary", "refl", "refl_shadow", "prepass_primary", "prepass_shadow", "cones", "cone_steps",
              "undef_hits"):
        assert st[k] == os_[k], (k, st[k], os_[k])
    assert st["sphere_steps"] < os_["sphere_steps"] and st["dda_steps"] <= os_["dda_steps"]
    # a GI update window: shadow and bounce rays through the same exit
    r.gi_update(3, first=1000, count=6000)
    ow.gi_update(3, first=1000, count=6000)
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), ow.gi)
    # the trace API: the reference's counts
    rng = np.random.default_rng(5)
    org, dirs, dist = random_rays(rng, 4000, (ow.X, ow.Y, ow.Z))
    g = r.trace_rays(org, dirs, dist)
    o = ow.trace_batch(org, dirs, dist)
    assert np.array_equal(g["sphere_steps"], o["n_sphere"]) and np.array_equal(g["dda_steps"], o["n_dda"])
    r.close()
