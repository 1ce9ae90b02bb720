"""RV_OPT_PIPE_MIX on the GPU: a pipelined launch whose pre-pass, GI and render workgroups are interleaved
(include/rvgrt/rv_internal.h pipe_layout) computes what one frame at a time computes -- frames (RGBA8,
motion vectors, depth), half-res images and the GI grid bit for bit, and the same RV_F_STATS counters --
for every pattern of the A/B (profiles/r07/pipe_mix_ab.txt) with heads of 0, 1/8 and 1/4 of the pre-pass
rows, at an even and an odd frame size, with a moving camera and a GI window that wraps.  Tile-share
launches keep the contiguous order whatever the option says."""
import numpy as np
import pytest

from gpu_world import rv

pytestmark = pytest.mark.gpu

LG = 7
RAYS = 7000            # cells per GI window of the 32768-cell grid: the 5th window is partial, the 6th wraps
CALLS = (2, 1, 3)      # 6 frames in three calls: the kept update and pre-pass cross the calls
PATTERNS = ((1, 0, 4), (1, 0, 3), (1, 0, 2), (1, 1, 4))   # with heads of 0, 1/8 and 1/4 of the pre-pass rows
MORE = ((3, 2, 12), (2, 1, 8), (2, 0, 8), (5, 2, 20), (1, 1, 6))   # the default and others of the second A/B round
SIZES = ((160, 96), (161, 97))


def pack(head, pat):
    return head << 24 | pat[0] << 16 | pat[1] << 8 | pat[2]


def mixes(W, H):
    """Pattern 0 and every pattern x head of the A/B; the heads from this frame's pre-pass rows."""
    rows = (((W // 2 + 7) // 8) * ((H // 2 + 7) // 8) + 7) // 8   # 60 waves of 8x8 texels: 8 rows
    return [0] + [pack(h, p) for p in PATTERNS for h in (0, rows // 8, rows // 4)] + [pack(0, p) for p in MORE]


def make(rv, atlas, W, H, flags=None):
    r = rv.StateRender((LG, LG, LG), W, H, flags=rv.RV_FLAGS_REFERENCE if flags is None else flags, atlas=atlas,
                       gi_rays_per_frame=RAYS)
    r.world_build()
    r.gi_update(0)
    return r


def path(W, H):
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    return camera_path(TEST_POSES_128["P0"], W, H, sum(CALLS), pan=0.01)


KINDS = ("RV_IMAGE_COLOR", "RV_IMAGE_MOTION", "RV_IMAGE_DEPTH", "RV_IMAGE_HALF_DIST", "RV_IMAGE_HALF_SHADOW")


def snapshot(rv, r):
    s = {k: r.readback(getattr(rv, k)).copy() for k in KINDS}
    s["gi"] = r.world_export(rv.RV_WORLD_GI).copy()
    return s


_REF = {}


def reference(rv, atlas, W, H, flags):
    """One frame at a time (UpdateGIData, then the frame), a snapshot after each call's last frame; computed
    once per frame size and flag set, shared by every case and never modified."""
    key = (W, H, flags)
    if key not in _REF:
        r = make(rv, atlas, W, H, flags)
        r.set_pipeline(0)
        p, k, snaps = path(W, H), 0, []
        for n in CALLS:
            for d in p[k:k + n]:
                r.update_gi_data()
                r.frame(d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp), time=d.time,
                        jx=d.jitter_x, jy=d.jitter_y, flags=flags)
            k += n
            snaps.append(snapshot(rv, r))
        r.close()
        _REF[key] = snaps
    return _REF[key]


def run_pipelined(rv, atlas, W, H, flags, mix, check):
    r = make(rv, atlas, W, H, flags)
    r.set_option(rv.RV_OPT_PIPE_MIX, mix)
    assert r.get_option(rv.RV_OPT_PIPE_MIX) == mix
    p, k = path(W, H), 0
    for i, n in enumerate(CALLS):
        r.render_frame_seq(p[k:k + n], next_desc=p[k + n], flags=flags, gi_per_frame=True)
        k += n
        assert r.get_option(rv.RV_OPT_PIPE_MIX_LAST) == mix
        check(i, r)
    return r


@pytest.mark.parametrize("size,mix", [(s, m) for s in SIZES for m in mixes(*s)],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else hex(v))
def test_mixed_launches_equal_one_frame_at_a_time(rv, atlas, size, mix):
    """Every pattern and head; the plain reference frame (these small frames launch the latency variant)."""
    W, H = size
    flags = rv.RV_FLAGS_REFERENCE
    ref = reference(rv, atlas, W, H, flags)

    def check(i, r):
        got = snapshot(rv, r)
        for k, want in ref[i].items():
            assert np.array_equal(got[k], want), (hex(mix), i, k)
    run_pipelined(rv, atlas, W, H, flags, mix, check).close()


@pytest.mark.parametrize("flags_name", ["stats", "no_water"])
def test_mixed_launches_throughput_variant(rv, atlas, flags_name):
    """The throughput variant's instantiations (RV_F_STATS; a feature set other than the reference's) under a
    three-way pattern with a head and a two-way pattern: frames and grid as one frame at a time, and with
    RV_F_STATS every stage's counters equal those of the contiguous order."""
    W, H = SIZES[1]
    flags = {"stats": rv.RV_FLAGS_REFERENCE | rv.RV_F_STATS, "no_water": rv.RV_F_PREPASS | rv.RV_F_GI}[flags_name]
    ref = reference(rv, atlas, W, H, flags)
    counters = {}
    for mix in (0, pack(1, (1, 1, 4)), pack(0, (1, 0, 2))):
        def check(i, r):
            got = snapshot(rv, r)
            for k, want in ref[i].items():
                assert np.array_equal(got[k], want), (hex(mix), i, k)
        r = run_pipelined(rv, atlas, W, H, flags, mix, check)
        counters[mix] = [r.stats(k) for k in range(8)]
        r.close()
    if flags & rv.RV_F_STATS:
        assert counters[0][2]["traces"] > 0 and counters[0][7]["gi_traces"] > 0
        for mix, c in counters.items():
            assert c == counters[0], hex(mix)


def test_tile_share_keeps_the_contiguous_order(rv, atlas):
    """A tile-share launch (a one-rank shard, assembled locally) under a set pattern: the launch reports
    pattern 0, and the frame and the grid equal the whole-frame loop's."""
    W, H = 160, 96
    flags = rv.RV_FLAGS_REFERENCE
    d = path(W, H)[0]
    vp, pvp = np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp)
    a, b = make(rv, atlas, W, H), make(rv, atlas, W, H)
    mix = pack(1, (1, 1, 4))
    b.set_option(rv.RV_OPT_PIPE_MIX, mix)
    b.set_tile_shard(32, 0, 1)
    for r in (a, b):
        r.render_frames(4, d.cam, vp, prev_vp=pvp, gi_per_frame=True)
    # the default pattern is the throughput variant's: this small frame's latency-variant launches keep 0
    # until the option is set; its RV_F_STATS launches (a throughput instantiation) take the default
    default = a.get_option(rv.RV_OPT_PIPE_MIX)
    assert default == pack(0, (3, 2, 12))
    assert a.get_option(rv.RV_OPT_PIPE_MIX_LAST) == 0
    c = make(rv, atlas, W, H)
    c.render_frames(2, d.cam, vp, prev_vp=pvp, flags=flags | rv.RV_F_STATS, gi_per_frame=True)
    assert c.get_option(rv.RV_OPT_PIPE_MIX_LAST) == default
    c.close()
    assert b.get_option(rv.RV_OPT_PIPE_MIX) == mix and b.get_option(rv.RV_OPT_PIPE_MIX_LAST) == 0
    assert np.array_equal(a.readback(rv.RV_IMAGE_COLOR), b.readback(rv.RV_IMAGE_COLOR))
    assert np.array_equal(a.world_export(rv.RV_WORLD_GI), b.world_export(rv.RV_WORLD_GI))
    b.set_tile_shard(32, 0, 0)   # whole frames again: the pattern applies
    b.render_frames(2, d.cam, vp, prev_vp=pvp, gi_per_frame=True)
    assert b.get_option(rv.RV_OPT_PIPE_MIX_LAST) == mix
    a.close()
    b.close()
