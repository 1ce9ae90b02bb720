"""The texture origin on the CPU (rv_texture_tile_at, host only: the kernels' own
texture_tile compiled for the host): against the numpy restatement of
tests/np_tex_anchor.py, against the unpatched reference restatement at origin
(0, 0), and its translation identity.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import rv
import np_shade as S
import np_tex_anchor as A

ORIGINS = [(0, 0), (8, 0), (40, -16), (123464, -98760), (2 ** 24 + 8, -2 ** 24 - 16)]


@pytest.fixture(scope="module")
def positions():
    """20,000 random positions in [0, 64)^3, and positions at the carry thresholds of the second lattice
    point: fractional parts .69 / .71 along x and y (+ 121.3, 1321.3), .49 / .51 along z (+ 721.5)."""
    rng = np.random.default_rng(20)
    rnd = rng.uniform(0, 64, (20000, 3)).astype(np.float32)
    base = rng.integers(0, 64, (4000, 3)).astype(np.float32)
    fr = np.stack([rng.choice([0.69, 0.71], 4000), rng.choice([0.69, 0.71], 4000), rng.choice([0.49, 0.51], 4000)], 1)
    edge = (base + fr.astype(np.float32)).astype(np.float32)
    return np.concatenate([rnd, edge])


@pytest.mark.parametrize("origin", ORIGINS)
def test_tile_at_equals_the_numpy_restatement(rv, positions, origin):
    got = rv.texture_tile_at(origin[0], origin[1], positions)
    want = A.tile_bytes(positions, origin)
    assert np.array_equal(got, want), (origin, int((got != want).sum()))
    assert len(np.unique(got)) >= 4                     # several tiles occur
    # every carry combination of the second lattice point occurs among the positions
    off = np.array([121.3, 1321.3, 721.5])
    carry = (np.floor((positions.astype(np.float64) + off).astype(np.float32)) - np.floor(positions)
             - np.array([121, 1321, 721])).astype(int)
    assert len({tuple(c) for c in carry}) == 8
    if origin == (0, 0):
        assert np.array_equal(got, A.tile_byte(S.texture_tile(positions)))
    else:
        changed = (got != rv.texture_tile_at(0, 0, positions)).mean()
        assert changed > 0.3, changed                   # the issue's census: 54 % to 71 % of positions


def test_translation_identity(rv):
    """Positions that are multiples of 1/64 in [0, 64)^3 and |o| < 2^16: p + o is exact in float, and so are
    its sums with the offsets' integer parts, so the tile at origin o equals the tile of p + o at origin 0."""
    rng = np.random.default_rng(21)
    p = (rng.integers(0, 64 * 64, (20000, 3)) / 64.0).astype(np.float32)
    for o in [(8, 0), (40, -16), (-65535, 65535), (12345, -54321)]:
        q = (p + np.array([o[0], 0, o[1]], np.float32)).astype(np.float32)
        assert np.array_equal(q.astype(np.float64), p.astype(np.float64) + np.array([o[0], 0, o[1]], np.float64))
        assert np.array_equal(rv.texture_tile_at(o[0], o[1], p), rv.texture_tile_at(0, 0, q)), o


def test_exports_and_abi_version(rv):
    L = rv._lib.load()
    for name in ("rv_texture_origin_set", "rv_texture_follow_scroll", "rv_texture_origin_get", "rv_texture_tiles",
                 "rv_texture_tile_at"):
        assert hasattr(L, name), name
    assert L.rv_abi_version() == 2
    assert C.sizeof(rv._lib.rv_config) == 72


def test_status_codes_without_a_device(rv):
    L = rv._lib.load()
    inv = rv._lib.RV_ERR_INVALID
    x, z, f = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.rv_texture_origin_set(None, 0, 0) == inv
    assert L.rv_texture_follow_scroll(None, 1) == inv
    assert L.rv_texture_origin_get(None, C.byref(x), C.byref(z), C.byref(f)) == inv
    assert L.rv_texture_tiles(None, None, 0, None) == inv
    p = np.zeros((1, 3), np.float32)
    t = np.zeros(1, np.uint8)
    pp, tp = p.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    big = 2 ** 31 - 1
    assert L.rv_texture_tile_at(big - 1322, big - 722, pp, 1, tp) == 0        # the largest origin
    assert L.rv_texture_tile_at(big - 1321, 0, pp, 1, tp) == inv              # a lattice point leaves int32
    assert L.rv_texture_tile_at(0, big - 721, pp, 1, tp) == inv
    assert L.rv_texture_tile_at(-2 ** 31, -2 ** 31, pp, 1, tp) == 0
    assert L.rv_texture_tile_at(0, 0, None, 1, tp) == inv
    assert L.rv_texture_tile_at(0, 0, pp, -1, tp) == inv
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        rv.texture_tile_at(big, 0, p)
