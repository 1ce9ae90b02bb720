"""The texture origin restated in numpy (test infrastructure): sampleTexture's atlas
tile with both lattice points shifted by (ox, 0, oz) as integers before the
conversion to float that feeds the noise.  Written from include/rvgrt.h's
definition on top of tests/np_shade.py's restatement of the reference's
sampleTexture (its simplex3D, thresholds and double-precision offsets), not from
the kernels: `anchored(origin)` patches it into np_shade, so np_shade.render and
np_shade.gi_update produce whole expected frames and GI windows at any origin."""
from __future__ import annotations

import contextlib

import numpy as np

import np_shade as S
from np_ref import simplex3D

f32 = np.float32


def texture_tile(pos, origin=(0, 0)):
    """np_shade.texture_tile at a texture origin: (whichBlock.x, whichBlock.y) as k/16 for positions (N, 3)."""
    pos = np.asarray(pos, f32)
    shift = np.array([int(origin[0]), 0, int(origin[1])], np.int64)
    freq = f32(0.05)
    f = np.floor(pos).astype(np.int64) + shift                      # the integer shift ...
    off = np.array([121.3, 1321.3, 721.5], np.float64)
    g = np.floor((pos.astype(np.float64) + off).astype(f32)).astype(np.int64) + shift
    fl, p2 = f.astype(f32), g.astype(f32)                           # ... then the conversion to float
    e1 = simplex3D(fl[:, 0] * freq, fl[:, 1] * freq, fl[:, 2] * freq)
    e2 = simplex3D((p2[:, 0] * freq) * f32(0.3), (p2[:, 1] * freq) * f32(0.3), (p2[:, 2] * freq) * f32(0.3))
    ev = (e1 * f32(0.4) + e2 * f32(0.6)).astype(f32)
    tx = np.full(len(pos), 0.0, f32)
    ty = np.full(len(pos), 1.0 / 16.0, f32)
    done = np.zeros(len(pos), bool)
    for th, (a, b) in S._TILES:
        m = (~done) & (ev < f32(th))
        tx[m] = f32(a / 16.0)
        ty[m] = f32(b / 16.0)
        done |= m
    return tx, ty


def tile_byte(tiles):
    """(tx, ty) in 1/16 units -> the library's byte 0xYX."""
    tx, ty = tiles
    return (np.rint(tx * 16).astype(np.uint8) | (np.rint(ty * 16).astype(np.uint8) << 4)).astype(np.uint8)


def tile_bytes(pos, origin=(0, 0)):
    return tile_byte(texture_tile(pos, origin))


@contextlib.contextmanager
def anchored(origin):
    """np_shade with its texture_tile at `origin` (sample_texture looks the name up at call time)."""
    old = S.texture_tile
    S.texture_tile = lambda pos: texture_tile(pos, origin)
    try:
        yield S
    finally:
        S.texture_tile = old


def voxel_centres(dims, rows):
    """Centres of every voxel of rows [0, rows), (n, 3) float32."""
    X, _, Z = dims
    z, y, x = np.mgrid[0:Z, 0:rows, 0:X]
    return (np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(f32) + f32(0.5)).astype(f32)
