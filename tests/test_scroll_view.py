"""rv_scroll_view (host only): a camera and its column-major VP matrices re-expressed
in the grid after rv_world_scroll(dx, dz) -- pos -= (dx, 0, dz), VP' = VP . T(dx, 0, dz)
-- against float64 numpy to within 1 ulp of float32, and the property it exists for:
a point's clip coordinates before the scroll equal those of the shifted point
after it."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import rv

CASES = [(8, 0), (0, -8), (64, -16), (-4096, 2048), (3, -5), (0, 0), (1 << 20, -(1 << 20))]


def views(rv):
    """A few poses' (camera, VP) from the library's own camera model, and a random matrix."""
    out = []
    for pos, yaw, pitch in (((300.5, 180.25, 411.0), 0.7, -0.3), ((17.0, 60.0, 1000.125), -2.4, 0.5),
                            ((2047.9, 33.3, 0.01), 3.0, 0.0)):
        out.append(rv.camera_from_pose(pos, yaw, pitch, 320, 192))
    cam, _ = out[0]
    out.append((cam, np.random.default_rng(5).normal(size=16).astype(np.float32) * 100))
    return out


def within_1ulp(got, want64):
    want = want64.astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    return bool(np.all((got >= lo) & (got <= hi)))


@pytest.mark.parametrize("dx,dz", CASES)
def test_matches_float64(rv, dx, dz):
    for cam, vp in views(rv):
        pvp = (vp * np.float32(1.25)).astype(np.float32)
        c2, v2, p2 = rv.scroll_view(dx, dz, cam, vp, pvp)
        T = np.eye(4)
        T[0, 3], T[2, 3] = dx, dz
        for m, m2 in ((vp, v2), (pvp, p2)):
            M = m.astype(np.float64).reshape(4, 4).T   # column-major
            want = (M @ T).T.reshape(16)
            assert within_1ulp(m2, want), (dx, dz)
            assert np.array_equal(m2[:12], m[:12])     # only the translation column moves
        pos = np.array(cam.pos[:], np.float64)
        assert within_1ulp(np.array(c2.pos[:], np.float32), pos - (dx, 0, dz))
        assert c2.pos[1] == cam.pos[1]
        for f in ("forward", "right", "up", "mul", "add"):
            assert list(getattr(c2, f)) == list(getattr(cam, f))
        # the inputs are untouched by the wrapper
        assert cam.pos[0] == np.float32(pos[0]) and cam.pos[2] == np.float32(pos[2])


@pytest.mark.parametrize("dx,dz", [(8, -24), (-512, 64), (2048, 2048)])
def test_clip_coordinates_are_kept(rv, dx, dz):
    rng = np.random.default_rng(11)
    for cam, vp in views(rv)[:3]:
        _, v2, _ = rv.scroll_view(dx, dz, None, vp, None)
        P = np.concatenate([rng.uniform(0, 2048, (64, 3)), np.ones((64, 1))], axis=1)   # points of the old grid
        Q = P - (dx, 0, dz, 0)                                                          # ... in the new grid
        M, M2 = (m.astype(np.float64).reshape(4, 4).T for m in (vp, v2))
        a, b = P @ M.T, Q @ M2.T
        # M2's column 3 was rounded to float32 once: half an ulp of its entries, which are sums of terms as
        # large as |d| * |M|
        scale = np.abs(M[:, :3]).max() * (2048 + abs(dx) + abs(dz)) + np.abs(M[:, 3]).max()
        assert np.abs(a - b).max() <= scale * 2.0 ** -23, (dx, dz)


def test_null_arguments(rv):
    L = rv._lib.load()
    assert L.rv_scroll_view(8, 8, None, None, None) == 0
    cam, vp = rv.camera_from_pose((10.0, 20.0, 30.0), 0.1, 0.2, 64, 64)
    assert rv.scroll_view(8, -8) == (None, None, None)
    c2, v2, p2 = rv.scroll_view(8, -8, cam)
    assert (v2, p2) == (None, None) and tuple(c2.pos) == (2.0, 20.0, 38.0)
    c2, v2, p2 = rv.scroll_view(8, -8, None, None, vp)
    assert c2 is None and v2 is None
    want = rv.scroll_view(8, -8, None, vp)[1]
    assert np.array_equal(p2, want) and not np.array_equal(p2, vp)
    # in place through the raw entry point, one pointer at a time
    raw = (C.c_float * 16)(*vp)
    assert L.rv_scroll_view(8, -8, None, raw, None) == 0
    assert np.array_equal(np.array(raw[:], np.float32), want)
    # (0, 0) is the identity
    c2, v2, _ = rv.scroll_view(0, 0, cam, vp)
    assert tuple(c2.pos) == tuple(cam.pos) and np.array_equal(v2, vp)
