"""The land pixel's cone lighting on the GPU (rv_shade.h cone_lighting, rv_device.h trace_cones6: first-sample
offsets from the per-normal table, the interior fast path with its all-opaque case, one cold loop for the cones
that go past step 0) against the oracle: frames (RGBA8, motion, depth) bit for bit and the frame's cone and
cone-step counts, through rv_frame (k_render), the pipelined native loop (k_ref_pipe) and the flow launch
(k_ref_flow: rv_frame on a flow context, and rv_draw_cuda).

The world is made for the paths of that code: a 64^3 world of pillars carrying plates, so that -y faces are
seen from below and +-x / +-z faces from the side, pillars and plates next to the world's faces (the slow
path) and far from them (the fast path) in one frame, and an imported GI grid of random texels whose alpha is
drawn from {0, 1, 128, 254, 255}: most cones that are not blocked go past step 0.  Before anything is
rendered the oracle's own hits must show that the frames hold what the test is about."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import oracle_of, pack, rv  # noqa: F401 -- rv is a fixture

pytestmark = pytest.mark.gpu

LG, N, W, H = (6, 6, 6), 64, 160, 96
RAYS = 512          # GI cells the pipelined loop updates per frame
ALPHAS = np.array([0, 1, 128, 254, 255], np.uint32)
# (position, yaw, pitch): low in one corner looking up and across, high in the opposite corner looking down
# and back, and inside the solid floor (every primary ray starts in a solid voxel)
POSES = {"low": ((5.5, 37.5, 6.5), -0.7, -np.pi + 0.35),
         "high": ((61.5, 60.5, 61.5), 2.35, -np.pi - 0.5),
         "in_solid": ((30.5, 33.5, 30.5), -0.7, -np.pi - 0.3)}
# close under a plate at the world's corner: primary rays that start inside it (test_undefined_hits_reach_the_cones)
EDGE_POSE = ((2.5, 36.5, 2.5), -0.8, -np.pi + 0.5)


def pillar_world():
    """[z, y, x] occupancy: a floor up to y = 34 (above the water level 31), 2 x 2 pillars every 8 voxels from
    it to a random height in [44, 63), each carrying a 6 x 6 plate one voxel thick at its top."""
    rng = np.random.default_rng(5)
    v = np.zeros((N, N, N), bool)
    v[:, :34, :] = True
    for k in range(1, N - 2, 8):
        for i in range(1, N - 2, 8):
            h = int(rng.integers(44, 63))
            v[k + 2:k + 4, 34:h, i + 2:i + 4] = True
            v[k:k + 6, h - 1:h, i:i + 6] = True
    return v


def mixed_gi():
    rng = np.random.default_rng(11)
    g = rng.integers(0, 1 << 24, (N // 4) ** 3, dtype=np.uint32)
    return g | (ALPHAS[rng.integers(0, 5, g.shape)] << 24)


@pytest.fixture(scope="module")
def scene(oracle, atlas):
    """The oracle's world, the same after the GI updates of the pipelined loop's frames 0 and 1, and per pose
    the oracle's frames; computed once for every test of the module."""
    bits = pack(pillar_world())
    ow = oracle_of(oracle, LG, bits, atlas=atlas)
    ow.gi[:] = mixed_gi().view(np.uint8)
    upd = []
    o2 = oracle_of(oracle, LG, bits, csdf=ow.csdf, atlas=atlas)
    o2.gi[:] = ow.gi
    for k in range(2):
        o2.gi_update(k, first=k * RAYS, count=RAYS)
        o3 = oracle_of(oracle, LG, bits, csdf=ow.csdf, atlas=atlas)
        o3.gi[:] = o2.gi
        upd.append(o3)
    return ow, upd


def _land(h):
    """Land pixels of the oracle's primary hits at the reference flags (water takes a hit below 31.001)."""
    return (h["hit"] != 0) & ~(h["pos"][..., 1] < np.float32(31.001))


def _continuing(oracle, ow, pos, nrm, enough):
    """Cones of these axis-normal hits with more than one step, by the oracle's traceCone (stops at `enough`)."""
    L, w, n = oracle.lib(), ow.c, 0
    c = np.float32(0.577)
    for p, up in zip(pos, nrm):
        up = up.astype(np.float32)
        right = np.cross(up, np.array([c, c, c], np.float32)).astype(np.float32)
        right /= np.float32(np.linalg.norm(right))
        fwd = np.cross(up, right).astype(np.float32)
        fwd /= np.float32(np.linalg.norm(fwd))
        half = np.float32(0.5)
        for d in (up, up + (right - up) * half, up + (-right - up) * half, up + (fwd - up) * half,
                  up + (-fwd - up) * half, up + ((right + (fwd - right) * half) - up) * half):
            st = C.c_int(0)
            L.or_trace_cone(C.byref(w), oracle.F3(*p), oracle.F3(*d), C.byref(st))
            n += st.value > 1
        if n >= enough:
            break
    return n


def _same(rv, r, ref, what):
    assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), ref["rgba"]), what
    assert np.array_equal(r.readback(rv.RV_IMAGE_MOTION), ref["mv"]), what
    assert np.array_equal(r.readback(rv.RV_IMAGE_DEPTH), ref["depth"]), what


def _ctx(rv, atlas, ow, flow):
    r = rv.StateRender(LG, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, gi_rays_per_frame=RAYS)
    r.world_import(rv.RV_WORLD_BITS, ow.bits)
    r.csdf_build()
    r.world_import(rv.RV_WORLD_GI, ow.gi)
    r.set_flow(flow)
    return r


def test_frames_hold_the_cases(rv, oracle, scene):
    """From the oracle's hits alone: the three frames together hold at least 1,000 land pixels of each of the
    six normals, 1,000 within 4 voxels of a world face and 1,000 farther inside, and 1,000 cones that go past
    step 0."""
    ow, _ = scene
    flags = rv.RV_FLAGS_REFERENCE
    codes, near, far, more = np.zeros(6, int), 0, 0, 0
    for name, pose in POSES.items():
        cam, vp = rv.camera_from_pose(*pose, W, H)
        fr = oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp))
        ref = oracle.render(ow, fr)
        h = oracle.primary_hits(ow, fr, halfdist=ref["halfdist"]).ravel()
        h = h[_land(h)]
        n, p = h["normal"], h["pos"]
        axis = (n != 0).any(axis=1)
        n, p = n[axis], p[axis]
        code = 2 * np.argmax(n != 0, axis=1) + (n.sum(axis=1) < 0)
        codes += np.bincount(code, minlength=6)
        margin = np.minimum(p, N - p).min(axis=1)
        near += int((margin < 4).sum())
        far += int((margin >= 4).sum())
        if more < 1000:
            more += _continuing(oracle, ow, p, n, 1000 - more)
    assert (codes >= 1000).all(), codes
    assert near >= 1000 and far >= 1000, (near, far)
    assert more >= 1000, more


@pytest.mark.parametrize("pose", list(POSES))
def test_cone_frames_equal_oracle(rv, atlas, oracle, scene, pose):
    from rvgrt_amd.configs import camera_path
    ow, upd = scene
    flags = rv.RV_FLAGS_REFERENCE
    cam, vp = rv.camera_from_pose(*POSES[pose], W, H)
    ref = oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)))
    ctx = []
    try:
        # rv_frame, two launches (k_prepass, k_render), and as one flow launch (k_ref_flow)
        for flow in (0, 1):
            r = _ctx(rv, atlas, ow, flow)
            ctx.append(r)
            r.stats_reset()
            r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
            _same(rv, r, ref, ("rv_frame", flow))
            st = r.stats(2)
            assert (st["cones"], st["cone_steps"]) == (ref["stats"]["cones"], ref["stats"]["cone_steps"]), flow
            r.frame(cam, vp, flags=flags)          # the instantiations without counters
            _same(rv, r, ref, ("rv_frame", flow, "plain"))
        # rv_draw_cuda on the flow context: the drop-in frame (time and texel fetch as drawCUDA's)
        d = camera_path(POSES[pose], W, H, 2, pan=0.01, ref_compat=True)[1]
        dvp, dpvp = np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp)
        r.draw_cuda(d.cam.pos[:], d.cam.forward[:], d.cam.up[:], d.cam.right[:], dvp, dpvp, 0.0, d.time)
        dref = oracle.render(ow, oracle.make_frame(W, H, flags | rv.RV_F_REF_FETCH, rv.camera_dict(d.cam, dvp),
                                                   time=d.time, pvp=dpvp), want_stats=False)
        _same(rv, r, dref, "rv_draw_cuda")
        active, launches, fallbacks = r.flow_info()
        assert active and launches >= 2 and fallbacks == 0
        # the pipelined native loop (k_ref_pipe): two frames, each after its GI update of RAYS cells
        refs = [oracle.render(o, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp))) for o in upd]
        for stats in (rv.RV_F_STATS, 0):
            p = _ctx(rv, atlas, ow, 0)
            ctx.append(p)
            p.stats_reset()
            p.render_frames(2, cam, vp, flags=flags | stats, gi_per_frame=True)
            _same(rv, p, refs[1], ("pipelined", stats))
            assert np.array_equal(p.world_export(rv.RV_WORLD_GI), upd[1].gi)
            st = p.stats(2)
            for k in ("cones", "cone_steps"):
                assert st[k] == (refs[0]["stats"][k] + refs[1]["stats"][k] if stats else 0), k
    finally:
        for r in ctx:
            r.close()


def test_undefined_hits_reach_the_cones(rv, atlas, oracle, scene):
    """Without the water branch (which takes the undefined hit's position (-500, -500, -500) at the reference
    flags) the undefined hit is a land pixel with a zero normal: the generic basis and the slow path.  A GI-only
    frame from inside the floor, where every primary ray is one, and a pre-pass + GI frame from under a plate in
    the world's corner, where they are scattered among defined hits."""
    ow, _ = scene
    r = _ctx(rv, atlas, ow, 0)
    try:
        for pose, flags, least in ((POSES["in_solid"], rv.RV_F_GI, W * H), (EDGE_POSE, rv.RV_F_PREPASS | rv.RV_F_GI, 500)):
            cam, vp = rv.camera_from_pose(*pose, W, H)
            ref = oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)))
            assert ref["stats"]["undef_hits"] >= least and ref["stats"]["cones"] >= 6 * least
            r.stats_reset()
            r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
            _same(rv, r, ref, pose)
            st = r.stats(2)
            assert (st["cones"], st["cone_steps"]) == (ref["stats"]["cones"], ref["stats"]["cone_steps"]), pose
    finally:
        r.close()


def test_all_opaque_grid(rv, atlas, oracle, oracle_world):
    """The generator's own GI grid (every alpha 255) on the 128^3 procedural world: the all-opaque case of the
    fast path, through rv_frame, the flow launch and the pipelined loop."""
    from rvgrt_amd.configs import TEST_POSES_128
    ow = oracle_world(7, 7, 7, gi_sweeps=1)
    assert (ow.gi.reshape(-1, 4)[:, 3] == 255).all()
    flags = rv.RV_FLAGS_REFERENCE
    cam, vp = rv.camera_from_pose(*TEST_POSES_128["P0"], W, H)
    ref = oracle.render(ow, oracle.make_frame(W, H, flags, rv.camera_dict(cam, vp)))
    assert ref["stats"]["cones"] >= 6 * 1000
    ctx = []
    try:
        for flow in (0, 1):
            r = rv.StateRender((7, 7, 7), W, H, flags=flags, atlas=atlas, gi_rays_per_frame=3000)
            ctx.append(r)
            r.world_build()
            r.gi_update(0)
            r.set_flow(flow)
            r.stats_reset()
            r.frame(cam, vp, flags=flags | rv.RV_F_STATS)
            _same(rv, r, ref, flow)
            st = r.stats(2)
            assert (st["cones"], st["cone_steps"]) == (ref["stats"]["cones"], ref["stats"]["cone_steps"]), flow
        one, pipe = ctx
        one.set_pipeline(0)
        for r in ctx:
            r.set_flow(0)
            r.render_frames(3, cam, vp, flags=flags, gi_per_frame=True)
        for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH):
            assert np.array_equal(pipe.readback(k), one.readback(k)), k
        assert np.array_equal(pipe.world_export(rv.RV_WORLD_GI), one.world_export(rv.RV_WORLD_GI))
    finally:
        for r in ctx:
            r.close()
