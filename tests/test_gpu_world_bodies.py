"""rv_world_bodies_move on the GPU: the kernel's masked word tests over the brick records against the numpy
restatement (tests/np_bodies.py) run on the context's exported bits, bit for bit: lo as uint32 and flags.
Where the world is at least 32 wide rv_world_bodies_move_at, the same function on the host, must agree too."""
import ctypes as C

import numpy as np
import pytest

from conftest import Hip
from gpu_world import dims, draw, pack, rv, same_frames, synthetic_voxels, voxels
import np_bodies as B

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = (1, 63, 65, 1000)        # partial waves, one wave + 1, several workgroups


def _same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "lo")
    assert np.array_equal(got[1], want[1]), (what, "flags")


def _context(rv, lg, vox=None, **kw):
    r = rv.StateRender(lg, 64, 64, **kw)
    if vox is None:
        r.world_build()
    else:
        r.world_import(rv.RV_WORLD_BITS, pack(vox))
        r.csdf_build()
    return r


def _exported(rv, r, lg):
    bits = r.world_export(rv.RV_WORLD_BITS)
    return bits, voxels(bits, lg)


def _world(rv, name):
    if name == "terrain":
        return (7, 7, 7), None
    if name == "ragged":
        return (5, 7, 6), synthetic_voxels("blocks", 32, 128, 64, np.random.default_rng(21))
    return (4, 4, 4), B.random_world(seed=22, n=16, floor=2)


# ---------------------------------------------------------------- 1. worlds, counts, masks
@pytest.mark.parametrize("name", ["terrain", "ragged", "tiny"])
def test_worlds_and_counts(rv, name):
    lg, vox = _world(rv, name)
    r = _context(rv, lg, vox)
    bits, vox = _exported(rv, r, lg)
    rng = np.random.default_rng(31)
    lo, size, delta = B.random_bodies(rng, max(COUNTS), dims(lg))
    if name == "terrain":        # most of the window is air: half of the bodies down where the ground is
        lo[::2, 1] = np.minimum(lo[::2, 1], F(vox.any(axis=(0, 2)).nonzero()[0].max() + 3))
    calls = bodies = 0
    for mode in (0, B.OPEN_EDGES):
        want = B.move(vox, lo, size, delta, mode)              # bodies are independent: a prefix is a case
        assert (want[1] & 63).any() and ((want[1] & 63) == 0).any() and (want[1] & B.EDGE).any()
        for n in COUNTS:
            got = r.bodies_move(lo[:n], size[:n], delta[:n], mode)
            _same(got, (want[0][:n], want[1][:n]), (name, mode, n))
            calls, bodies = calls + 1, bodies + n
        s = B.straddling_bodies(dims(lg))
        got = r.bodies_move(*s, mode)
        calls, bodies = calls + 1, bodies + len(s[0])
        _same(got, B.move(vox, *s, mode), (name, mode, "straddling"))
        if lg[0] >= 5:
            _same(got, rv.bodies_move_at(lg, bits, *s, mode), (name, mode, "move_at"))
            _same(r.bodies_move(lo, size, delta, mode), rv.bodies_move_at(lg, bits, lo, size, delta, mode), name)
            calls, bodies = calls + 1, bodies + len(lo)
    assert r.bodies_info() == (calls, bodies)
    r.close()


# ---------------------------------------------------------------- 2. the device form
class _DeviceBodies:
    """n rv_body and n rv_body_out in device buffers of the runtime the library loaded."""
    H2D, D2H, D2D = 1, 2, 3

    def __init__(self, hip, n):
        self.hip, self.n = hip, n
        self.d_in, self.d_out = hip.malloc(36 * n), hip.malloc(16 * n)

    def upload(self, lo, size, delta):
        b = np.empty((self.n, 9), F)
        b[:, 0:3], b[:, 3:6], b[:, 6:9] = lo, size, delta
        assert self.hip.L.hipMemcpy(C.c_void_p(self.d_in), b.ctypes.data_as(C.c_void_p), C.c_size_t(b.nbytes),
                                    self.H2D) == 0

    def set_delta(self, delta):
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, F), (self.n, 3)))
        assert self.hip.L.hipMemcpy2D(C.c_void_p(self.d_in + 24), C.c_size_t(36), d.ctypes.data_as(C.c_void_p),
                                      C.c_size_t(12), C.c_size_t(12), C.c_size_t(self.n), self.H2D) == 0

    def feed_back(self):
        """out.lo -> in.lo, on the device."""
        assert self.hip.L.hipMemcpy2D(C.c_void_p(self.d_in), C.c_size_t(36), C.c_void_p(self.d_out), C.c_size_t(16),
                                      C.c_size_t(12), C.c_size_t(self.n), self.D2D) == 0

    def download(self):
        out = np.zeros((self.n, 4), np.uint32)
        assert self.hip.L.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.d_out), C.c_size_t(out.nbytes),
                                    self.D2H) == 0
        return np.ascontiguousarray(out[:, :3]).view(F), out[:, 3].copy()


def test_device_form(rv):
    lg = (7, 7, 7)
    r = _context(rv, lg)
    bits, vox = _exported(rv, r, lg)
    hip = Hip()
    try:
        # the same bodies through both forms
        lo, size, delta = B.random_bodies(np.random.default_rng(41), 1000, dims(lg))
        lo[:, 1] = np.minimum(lo[:, 1], F(vox.any(axis=(0, 2)).nonzero()[0].max() + 3))
        for n in (65, 1000):
            d = _DeviceBodies(hip, n)
            d.upload(lo[:n], size[:n], delta[:n])
            for mode in (0, B.OPEN_EDGES):
                r.bodies_move_device(d.d_in, n, d.d_out, mode)
                r.sync()
                _same(d.download(), r.bodies_move(lo[:n], size[:n], delta[:n], mode), ("device", n, mode))
        # drop and walk: 24 player-sized bodies fall from above the terrain and walk across it, 200 steps
        # chained through the device buffers, each step against the restatement
        n = 24
        rng = np.random.default_rng(42)
        lo = np.stack([rng.uniform(20, 100, n), np.full(n, 126.0), rng.uniform(20, 100, n)], 1).astype(F)
        size = np.broadcast_to(np.array([0.6, 1.8, 0.6], F), (n, 3))
        walk = rng.normal(0, 0.3, (n, 3)).astype(F)
        walk[:, 1] = F(-0.75)
        d = _DeviceBodies(hip, n)
        d.upload(lo, size, walk)
        landed = walked = 0
        for step in range(200):
            if step == 120:                               # turn round
                walk[:, [0, 2]] = -walk[:, [0, 2]]
                d.set_delta(walk)
            r.bodies_move_device(d.d_in, n, d.d_out, 0)
            r.sync()
            got = d.download()
            want = B.move(vox, lo, size, walk, 0)
            _same(got, want, ("walk", step))
            landed += int((got[1] & B.YN).astype(bool).sum())
            walked += int((got[1] & (B.XN | B.XP | B.ZN | B.ZP)).astype(bool).sum())
            lo = got[0]
            d.feed_back()
        assert landed > 50 * n and walked > 0             # they stood on the ground and ran into it
    finally:
        hip.close()
        r.close()


# ---------------------------------------------------------------- 3. after an edit
@pytest.mark.parametrize("lg,full", [((9, 7, 7), False), ((7, 7, 7), True)])
def test_after_an_edit(rv, lg, full):
    """A floor placed in the air catches a falling body; once it is cleared the same body falls through."""
    r = _context(rv, lg)
    vox = _exported(rv, r, lg)[1]
    fy = 110
    x, z = next((x, z) for z in range(16, 112, 8) for x in range(16, 112, 8)
                if not vox[z - 2:z + 6, 60:, x - 2:x + 6].any())            # open air from row 60 up
    body = ([(x + 1.25, 120.0, z + 1.25)], (0.6, 1.8, 0.6), (0.0, -58.0, 0.0))
    down = r.bodies_move(*body)
    assert down[0][0].tolist() == [x + 1.25, 62.0, z + 1.25] and down[1][0] == 0      # nothing in the way

    floor = (x, fy, z, x + 4, fy + 1, z + 4)
    r.world_edit([floor + (1,)])
    assert r.world_edit_info()[2] is full
    on = r.bodies_move(*body)
    assert on[0][0].tolist() == [x + 1.25, fy + 1.0, z + 1.25] and on[1][0] == B.YN
    _same(on, B.move(_exported(rv, r, lg)[1], *body), "placed")

    r.world_edit([floor + (0,)])
    assert r.world_edit_info()[2] is full
    _same(r.bodies_move(*body), down, "cleared")
    r.close()


# ---------------------------------------------------------------- 4. after a scroll
def test_after_a_scroll(rv):
    lg = (7, 7, 7)
    r = _context(rv, lg, seed=(24, -8))
    bits, vox = _exported(rv, r, lg)
    rng = np.random.default_rng(51)
    # bodies in the middle of the window on a 1/64 lattice with dyadic sizes and deltas: shifting them by a
    # scroll is exact in fp32, so their results shift with them bit for bit
    n = 600
    lo = (np.round(rng.uniform(24, 96, (n, 3)) * 64) / 64).astype(F)
    lo[:, 1] = (np.round(rng.uniform(0, 100, n) * 64) / 64).astype(F)
    size = rng.choice(np.array([1 / 32, 0.75, 1.0, 1.75, 2.0], F), (n, 3))
    delta = (np.round(rng.uniform(-4, 4, (n, 3)) * 64) / 64).astype(F)
    any_lo, any_size, any_delta = B.random_bodies(rng, 600, dims(lg))
    before = r.bodies_move(lo, size, delta)
    _same(before, B.move(vox, lo, size, delta), "before")
    assert (before[1] & 63).any() and ((before[1] & 63) == 0).any()
    for (dx, dz) in ((8, 0), (0, -16)):
        r.world_scroll(dx, dz)
        shift = np.array([dx, 0, dz], F)
        lo = lo - shift                                   # as rv_scroll_view moves the camera
        got = r.bodies_move(lo, size, delta)
        assert np.array_equal((got[0] + shift).view(np.uint32), before[0].view(np.uint32)), (dx, dz)
        assert np.array_equal(got[1], before[1]), (dx, dz)
        before = got
        vox = _exported(rv, r, lg)[1]
        _same(got, B.move(vox, lo, size, delta), ("retained", dx, dz))
        for mode in (0, B.OPEN_EDGES):
            _same(r.bodies_move(any_lo, any_size, any_delta, mode), B.move(vox, any_lo, any_size, any_delta, mode),
                  ("anywhere", dx, dz, mode))
    r.close()


# ---------------------------------------------------------------- 5. the frames do not notice
@pytest.mark.parametrize("mode,in_flight", [("draw", 1), ("seq", 2), ("group", 1)])
def test_frames_are_untouched(rv, atlas, mode, in_flight):
    """A twin renders the same flow, pipelined or grouped frames without the move calls in between."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, W, H = (7, 7, 7), 160, 96
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
            c.set_frame_group(2)
            assert c.frame_group_effective() == 2
    lo, size, delta = B.random_bodies(np.random.default_rng(61), 1000, dims(lg))
    hip = Hip()
    try:
        d = _DeviceBodies(hip, len(lo))
        d.upload(lo, size, delta)
        first = None
        for k0 in (0, n):
            if mode == "draw":
                for k in range(k0, k0 + n):
                    r.bodies_move_device(d.d_in, d.n, d.d_out, 0)      # enqueued next to the frame
                    for c in (r, t):
                        c.update_gi_data()
                        draw(c, seq[k])
                    got = r.bodies_move(lo, size, delta)
                    same_frames(rv, r, t, k)
            else:
                r.bodies_move_device(d.d_in, d.n, d.d_out, 0)
                for c in (r, t):
                    c.render_frame_seq(seq[k0:k0 + n], next_desc=seq[k0 + n], flags=flags, gi_per_frame=True)
                got = r.bodies_move(lo, size, delta)
                same_frames(rv, r, t, k0)
            r.sync()
            _same(d.download(), got, (mode, k0))
            first = first or got
            _same(got, first, (mode, k0, "repeatable"))
        assert r.flow_info()[2] == 0 and t.flow_info()[2] == 0
        if mode == "draw":
            assert r.flow_info()[0] and r.flow_info()[1] == 2 * n     # the flow path ran, as in the twin
        assert r.flow_info() == t.flow_info()
        assert t.bodies_info() == (0, 0) and r.bodies_info()[0] > 0
    finally:
        hip.close()
        r.close()
        t.close()


# ---------------------------------------------------------------- 6. status codes and counters
def test_status_codes_and_counters(rv):
    L, lib = rv._lib.load(), rv._lib
    r = rv.StateRender((5, 5, 5), 64, 64)
    b = np.zeros((4, 9), F)
    b[:, 3:6] = 1
    out = np.zeros((4, 4), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    hip = Hip()
    try:
        d_in, d_out = hip.malloc(36 * 4), hip.malloc(16 * 4)
        dev = lambda i, n, fl, o: L.rv_world_bodies_move_device(r._h, C.c_void_p(i), n, fl, C.c_void_p(o))   # noqa: E731
        host = lambda i, n, fl, o: L.rv_world_bodies_move(r._h, i, n, fl, o)   # noqa: E731
        # before a world: a valid call is out of order, an empty one is not
        assert host(p(b), 4, 0, p(out)) == lib.RV_ERR_STATE and dev(d_in, 4, 0, d_out) == lib.RV_ERR_STATE
        with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
            r.bodies_move(b[:, 0:3], b[:, 3:6], b[:, 6:9])
        assert host(None, 0, 0, None) == lib.RV_OK and dev(None, 0, 0, None) == lib.RV_OK
        r.world_build()
        assert r.bodies_info() == (0, 0)
        for f in (host, dev):
            i, o = (p(b), p(out)) if f is host else (d_in, d_out)
            assert f(i, 4, 0, o) == lib.RV_OK and f(i, 4, B.OPEN_EDGES, o) == lib.RV_OK
            assert f(None, 0, 0, None) == lib.RV_OK
            assert f(None, 4, 0, o) == lib.RV_ERR_INVALID and f(i, 4, 0, None) == lib.RV_ERR_INVALID
            assert f(i, -1, 0, o) == lib.RV_ERR_INVALID and f(i, (1 << 24) + 1, 0, o) == lib.RV_ERR_INVALID
            assert f(i, 4, 2, o) == lib.RV_ERR_INVALID and f(i, 4, -1, o) == lib.RV_ERR_INVALID
        assert dev(d_in, 4, 0, d_in) == lib.RV_ERR_INVALID                 # overlapping arrays
        assert dev(d_in, 4, 0, d_in + 16) == lib.RV_ERR_INVALID
        assert dev(d_in, 4, 0, d_out + 4) == lib.RV_ERR_INVALID            # dev_out is 16-byte aligned
        r.sync()
        assert r.bodies_info() == (4, 16)                                  # the calls that did work
        calls, bodies = C.c_uint64(), C.c_uint64()
        assert L.rv_world_bodies_info(r._h, None, None) == lib.RV_OK
        assert L.rv_world_bodies_info(r._h, C.byref(calls), None) == lib.RV_OK and calls.value == 4
        assert L.rv_world_bodies_info(r._h, None, C.byref(bodies)) == lib.RV_OK and bodies.value == 16
    finally:
        hip.close()
        r.close()
