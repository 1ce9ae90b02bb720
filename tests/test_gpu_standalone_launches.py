"""The stand-alone pre-pass / render launches (k_prepass, k_render, k_prepass_tiles, k_render_tiles) in
every variant the launchers choose between, at a frame size that is no multiple of the wave block or of
the tile, against the CPU oracle."""
import numpy as np
import pytest

from gpu_world import rv

pytestmark = pytest.mark.gpu


_ODD_FRAME = {}


def _odd_frame_reference(rv, atlas, oracle, seq, W, H):
    """The oracle's image of seq[1] (rendered once, shared by the cases; a world of its own: the session's
    shared oracle worlds carry other tests' GI updates)."""
    if "img" not in _ODD_FRAME:
        d = seq[1]
        ow = oracle.OracleWorld(7, 7, 7, atlas=atlas).build(gi_sweeps=1)
        fr = oracle.make_frame(W, H, rv.RV_FLAGS_REFERENCE, rv.camera_dict(d.cam, np.ctypeslib.as_array(d.vp)),
                               time=d.time, jx=d.jitter_x, jy=d.jitter_y, pvp=np.ctypeslib.as_array(d.prev_vp))
        _ODD_FRAME["img"] = oracle.render(ow, fr, want_stats=False)["rgba"]
    return _ODD_FRAME["img"]


@pytest.mark.parametrize("stats", [False, True])
def test_standalone_launches_odd_frame(rv, atlas, oracle, stats):
    """The stand-alone pre-pass / render launches (no pipelined, flow or grouped launch) of the reference
    frame at a size that is no multiple of the 8-px wave block or of the 16-px tile: whole frames and tile
    lists, one camera for the launch and a per-frame camera table, RGBA8 and RGB24 packed tiles, with and
    without RV_F_STATS -- every image equals the oracle's, hence the whole-frame image, bit for bit."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H, T = 7, 150, 90, 16
    flags = rv.RV_FLAGS_REFERENCE | (rv.RV_F_STATS if stats else 0)
    seq = camera_path(TEST_POSES_128["P0"], W, H, 2, pan=0.03, ref_compat=False)
    want = _odd_frame_reference(rv, atlas, oracle, seq, W, H)
    d = seq[1]
    one = dict(prev_vp=np.ctypeslib.as_array(d.prev_vp), time=d.time, jx=d.jitter_x, jy=d.jitter_y, flags=flags)
    r = rv.StateRender((lg,) * 3, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas)
    r.world_build()
    r.gi_update(0)
    r.set_frames_in_flight(2)   # frame slots: rv_frame takes the two stand-alone launches, not the flow launch

    def check(what):
        assert np.array_equal(r.readback(rv.RV_IMAGE_COLOR), want), what

    r.frame(d.cam, np.ctypeslib.as_array(d.vp), **one)                 # whole frame, one camera
    check("frame")
    r.render_frame_seq(seq[:2], flags=flags)                           # whole frames, camera table
    check("seq")
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    ids = np.arange(tiles_x * tiles_y, dtype=np.int32)[::-1].copy()    # tile list, one camera, RGBA8
    sink = rv.StateRender((lg,) * 3, W, H, atlas=atlas)
    r.frame_tiles(d.cam, np.ctypeslib.as_array(d.vp), ids, tile_px=T, **one)
    r.sync()
    sink.untile(r.tile_buffer()[0], ids, tile_px=T)
    sink.sync()
    assert np.array_equal(sink.readback(rv.RV_IMAGE_COLOR), want), "frame_tiles"
    sink.close()
    r.set_tile_shard(T, 0, 1)
    for bpp in (3, 4):
        r.set_gather_bpp(bpp)
        r.render_frame_seq(seq[:2], flags=flags)                       # tile shard, camera table
        check(("shard seq", bpp))
        r.render_frames(2, d.cam, np.ctypeslib.as_array(d.vp), **one)  # tile shard, one camera
        check(("shard frames", bpp))
    r.close()
