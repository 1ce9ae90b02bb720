"""Plain numpy references for the traversal's exit tables (rv_abi.cpp world_top: World::ytop,
the 2x2-voxel column tops, the 3x3-brick-column neighbourhood tops and the sun horizon),
computed from the canonical voxel array (OracleWorld.voxels(), [z, y, x]) and sharing no code
with the library.  tests/test_exits_ref.py proves them on the host-compiled tables,
tests/test_gpu_exits.py then holds the GPU's tables to them.

The integer tables are max-reductions, exact by definition.  The horizon is stated three ways:
  * horizon_safety:    float64, from the geometry alone -- "from here a sun ray can only miss";
  * horizon_tightness: float64, the bound of horizon_column's comment evaluated exhaustively
                       over a superset band, with no scan window and no early stop;
  * horizon_f32:       a float32 restatement of horizon_column, operation by operation (the
                       library is built with -ffp-contract=off), expected bit-equal.
All horizon arrays are [z / 2, x / 2], as rv_world_export returns them.
"""
import numpy as np

from gpu_world import synthetic_voxels

HORIZON_OFF = 0xFFFFFFFF     # the fills of a table that is switched off (rv_config.exits_off)
DTOP_OFF = 0x7F7F7F7F


# ---------------------------------------------------------------- worlds both test files use
def terrain_cut(oracle, lx, ly, lz, cut=None):
    """The procedural terrain's voxels, rows >= cut cleared (open sky above, as tests/test_host_trace.py)."""
    vox = oracle.OracleWorld(lx, ly, lz).fill().voxels()
    if cut is not None:
        vox[:, cut:, :] = False
    return vox


def synthetic(kind, X, Y, Z):
    return synthetic_voxels(kind, X, Y, Z, np.random.default_rng(sum(map(ord, kind))))


def single(X, Y, Z, where):
    v = np.zeros((Z, Y, X), bool)
    x, y, z = where
    v[z, y, x] = True
    return v


# name -> (log2 dims, maker(oracle) -> voxels); no world above 256 x 64 x 128
WORLDS = {
    "terrain128_cut90": ((7, 7, 7), lambda O: terrain_cut(O, 7, 7, 7, 90)),
    "terrain_8_6_7": ((8, 6, 7), lambda O: terrain_cut(O, 8, 6, 7)),
    "terrain_6_7_5": ((6, 7, 5), lambda O: terrain_cut(O, 6, 7, 5)),
    "terrain16": ((4, 4, 4), lambda O: terrain_cut(O, 4, 4, 4)),
    "empty": ((6, 5, 6), lambda O: synthetic("empty", 64, 32, 64)),
    "full": ((5, 5, 6), lambda O: synthetic("full", 32, 32, 64)),
    "sparse": ((6, 6, 5), lambda O: synthetic("sparse", 64, 64, 32)),
    "dense": ((5, 6, 6), lambda O: synthetic("dense", 32, 64, 64)),
    "pillars": ((7, 6, 6), lambda O: synthetic("pillars", 128, 64, 64)),
    "voxel_origin": ((5, 4, 6), lambda O: single(32, 16, 64, (0, 0, 0))),
    "voxel_far_corner": ((6, 4, 5), lambda O: single(64, 16, 32, (63, 15, 31))),
}


def bits_of(vox):
    """Canonical bit words (rv_world_import's RV_WORLD_BITS layout) of a [z, y, x] voxel array."""
    return np.packbits(np.ascontiguousarray(vox).ravel(), bitorder="little").view(np.uint32).copy()


# ---------------------------------------------------------------- rays (those of tests/test_host_trace.py)
N_RAYS = 30001   # not a multiple of the 64-lane wave: the last wave is partial


def sky_rays(dims, n=N_RAYS):
    """test_sky_exit_keeps_every_hit's rays: anywhere, half of them pointing up, some exactly level."""
    from conftest import random_rays
    rng = np.random.default_rng(77)
    org, d, dist = random_rays(rng, n, dims)
    up = rng.random(len(d)) < 0.5
    d[up, 1] = np.abs(d[up, 1])
    d[:200, 1] = 0.0
    d[200:400, 1] = -0.0
    return org, d, dist


def sun_rays(ow, sun):
    """test_sun_exit_keeps_every_shadow_hit's rays: toward the sun from the voxel surfaces (primary hits of
    random rays, offset along the normal as the kernels do) and from anywhere in the world."""
    from conftest import random_rays
    rng = np.random.default_rng(9)
    org0, d0, dist0 = random_rays(rng, 40000, (ow.X, ow.Y, ow.Z))
    h0 = ow.trace_batch(org0, d0, dist0)
    sel = (h0["hit"] != 0) & (h0["undef"] == 0)
    surf = (h0["pos"][sel] + h0["normal"][sel] * np.float32(0.1)).astype(np.float32)
    org = np.concatenate([surf, org0[:10000]])
    org = np.ascontiguousarray(org[:len(org) - (len(org) % 64 == 0)], np.float32)
    dirs = np.ascontiguousarray(np.broadcast_to(np.asarray(sun, np.float32), org.shape), np.float32)
    return org, dirs, np.zeros(len(org), np.float32)


def column_rays(vox, n=N_RAYS):
    """test_column_skip_keeps_every_hit's rays: skimming just above the terrain, ascending, level and
    descending, from above the surface tops and from the water plane.  Also returns each ray's start
    height above its own voxel column's top."""
    Z, Y, X = vox.shape
    top = tops(vox) - 1                                        # highest solid y per (z, x), -1: empty
    top = np.maximum(top, 0)
    rng = np.random.default_rng(21)
    x = rng.integers(0, X, n)
    z = rng.integers(0, Z, n)
    org = np.stack([x + rng.uniform(0, 1, n), top[z, x] + 1 + rng.uniform(0.05, 4.0, n), z + rng.uniform(0, 1, n)],
                   1).astype(np.float32)
    water = rng.uniform(size=n) < 0.3
    org[water, 1] = np.float32(31.0) + rng.uniform(0.0, 1.0, water.sum()).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 1] = rng.uniform(-0.25, 0.25, n) * np.hypot(d[:, 0], d[:, 2])
    d[rng.uniform(size=n) < 0.05, 1] = 0.0
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(org), np.ascontiguousarray(d), np.zeros(n, np.float32), org[:, 1] - (top[z, x] + 1)


def groups_walked(dda, g):
    """Look-ahead groups of g cells a ray's DDA walked (test_column_skip_keeps_every_hit's measure)."""
    return (dda.astype(np.int64) + g - 1) // g


# ---------------------------------------------------------------- integer tables
def tops(vox):
    """[z, x]: highest solid row + 1 of every voxel column, 0 = empty."""
    Y = vox.shape[1]
    return np.where(vox.any(axis=1), Y - np.argmax(vox[:, ::-1, :], axis=1), 0).astype(np.int64)


def ytop(vox):
    """World::ytop: min(Y, highest solid row + 2); the device gives 1 for a world without a solid voxel."""
    return int(min(vox.shape[1], tops(vox).max() + 1))


def coltop(vox):
    """[z / 2, x / 2] uint32: highest solid row + 1 per 2x2-voxel column."""
    t = tops(vox)
    Z, X = t.shape
    return t.reshape(Z // 2, 2, X // 2, 2).max(axis=(1, 3)).astype(np.uint32)


def dtop(vox):
    """[z / 8, x / 8] int32: max of coltop over the 3x3 brick columns around each, clipped at the edges."""
    t = tops(vox)
    Z, X = t.shape
    b = t.reshape(Z // 8, 8, X // 8, 8).max(axis=(1, 3))
    p = np.zeros((b.shape[0] + 2, b.shape[1] + 2), np.int64)
    p[1:-1, 1:-1] = b
    out = np.zeros_like(b)
    for dz in range(3):
        for dx in range(3):
            out = np.maximum(out, p[dz:dz + b.shape[0], dx:dx + b.shape[1]])
    return out.astype(np.int32)


# ---------------------------------------------------------------- the sun horizon
def _sun64(sun):
    s = np.asarray(sun, np.float32).astype(np.float64)
    hxz = np.hypot(s[0], s[2])
    return s[0] / hxz, s[2] / hxz, s[1] / hxz    # ux, uz, k_true


def _offsets(ncz, ncx):
    """Centre offsets (voxels) of column b from column c for every (bz - cz, bx - cx)."""
    dz = 2.0 * np.arange(-(ncz - 1), ncz)[:, None]
    dx = 2.0 * np.arange(-(ncx - 1), ncx)[None, :]
    return np.broadcast_arrays(dz, dx)


def _max_over_columns(ct, cost, valid):
    """[cz, cx] -> max over solid columns b with valid[b - c] of ct[b] - cost[b - c] (-inf: none)."""
    ncz, ncx = ct.shape
    solid = ct > 0
    base = np.where(solid, ct.astype(np.float64), -np.inf)
    pen = np.where(valid, cost, np.inf)
    out = np.full((ncz, ncx), -np.inf)
    # offset by offset over the valid ones (a narrow band along the sun's direction): the same differences
    # as column by column, and a max does not depend on the order of its arguments
    for j, i in np.argwhere(np.isfinite(pen)):
        dz, dx = int(j) - (ncz - 1), int(i) - (ncx - 1)      # b - c
        c = (slice(max(0, -dz), min(ncz, ncz - dz)), slice(max(0, -dx), min(ncx, ncx - dx)))
        b = (slice(max(0, dz), min(ncz, ncz + dz)), slice(max(0, dx), min(ncx, ncx + dx)))
        np.maximum(out[c], base[b] - pen[j, i], out=out[c])
    return out


def horizon_safety(ct, sun):
    """Float64 lower bound of a safe horizon, from the geometry alone.  A ray toward the sun from
    anywhere in the 2x2 column c moves that square along u = the sun's horizontal unit direction; it can
    meet a solid voxel of column b only while the moved square overlaps b's square, i.e. at a horizontal
    travel t >= 0 with |t ux - dx| <= 2 and |t uz - dz| <= 2 (d = the centre offset); hmin = the least
    such t.  By then it has risen k_true hmin, so a start height y is safe iff
    y >= max_b (top_b - k_true hmin(c, b)); pairs whose squares never overlap are skipped."""
    ux, uz, k = _sun64(sun)
    dz, dx = _offsets(*ct.shape)

    def interval(u, d):
        if u == 0.0:
            return np.where(np.abs(d) <= 2.0, -np.inf, np.inf), np.where(np.abs(d) <= 2.0, np.inf, -np.inf)
        a, b = (d - 2.0) / u, (d + 2.0) / u
        return np.minimum(a, b), np.maximum(a, b)
    lx, hx = interval(ux, dx)
    lz, hz = interval(uz, dz)
    lo = np.maximum(np.maximum(lx, lz), 0.0)
    hi = np.minimum(hx, hz)
    return _max_over_columns(ct, k * lo, lo <= hi)


def horizon_tightness(ct, sun):
    """Float64 upper bound: ceil(max over the solid columns b of the band |d.n| <= 2R + 0.02,
    d.u >= -2R - 0.02 of top_b + 2 - 0.999 k_true max(0, d.u - 2R)) + 1 -- the bound of horizon_column's
    comment over a superset band, every column tried (no scan window, no early stop); 0 when the band
    holds no solid column.  The + 1 covers float32 rounding under ceilf (operands below 2^11)."""
    ux, uz, k = _sun64(sun)
    R = abs(ux) + abs(uz)
    dz, dx = _offsets(*ct.shape)
    du, dn = dx * ux + dz * uz, dx * -uz + dz * ux
    band = (np.abs(dn) <= 2.0 * R + 0.02) & (du >= -2.0 * R - 0.02)
    v = _max_over_columns(ct, 0.999 * k * np.maximum(0.0, du - 2.0 * R) - 2.0, band)
    return np.ceil(np.maximum(v, 0.0)) + 1.0


def horizon_f32(ct, sun, topmax):
    """horizon_column (rv_device.h) restated in float32 numpy, every operation separately rounded,
    vectorised over the columns still scanning; the constants as rv_abi.cpp's world_top passes them
    (slope shaded 0.1 % low, topmax = World::ytop)."""
    f = np.float32
    s = np.asarray(sun, np.float32).astype(np.float64)
    hxz = np.sqrt(s[0] * s[0] + s[2] * s[2])
    k, ux, uz = f(s[1] / hxz * (1.0 - 1e-3)), f(s[0] / hxz), f(s[2] / hxz)
    ncz, ncx = ct.shape
    R = f(np.abs(ux) + np.abs(uz))
    nx, nz = f(-uz), ux
    R2 = f(f(2.0) * R)
    jj, ii = np.divmod(np.arange(ncz * ncx), ncx)
    cx = (f(2.0) * ii.astype(f) + f(1.0)).astype(f)
    cz = (f(2.0) * jj.astype(f) + f(1.0)).astype(f)
    wx, wz = f(2.0) * f(ncx), f(2.0) * f(ncz)
    top = ct.ravel()
    H = np.zeros(ncz * ncx, f)
    act = np.arange(ncz * ncx)                   # the columns still scanning
    sidx = int(np.floor(f(f(-2.0) * R) - f(0.5)))
    o5z, o5x = (v.reshape(25, 1) for v in np.divmod(np.arange(25), 5))
    topmax = f(topmax)
    while act.size:
        t = f(sidx)
        sidx += 1
        a = f(f(t - f(0.5)) - R2)
        if a > 0:                                  # no later sample can raise the result
            act = act[~(f(f(topmax + f(2.0)) - f(k * a)) <= H[act])]
        qx = (cx[act] + f(t * ux)).astype(f)
        qz = (cz[act] + f(t * uz)).astype(f)
        out = (qx < f(-4.0)) | (qz < f(-4.0)) | (qx > f(wx + f(4.0))) | (qz > f(wz + f(4.0)))
        if t > 0:                                  # left the world ahead: done
            act, qx, qz = act[~out], qx[~out], qz[~out]
        else:                                      # still behind the world: next sample
            qx, qz = qx[~out], qz[~out]
        cur = act if t > 0 else act[~out]
        b0x = np.floor(((qx - f(4.4)).astype(f) * f(0.5)).astype(f)).astype(np.int64)
        b0z = np.floor(((qz - f(4.4)).astype(f) * f(0.5)).astype(f)).astype(np.int64)
        # the 5 x 5 columns around the sample, all at once: [25, columns]
        bx, bz = b0x[None, :] + o5x, b0z[None, :] + o5z
        ok = (bx >= 0) & (bz >= 0) & (bx < ncx) & (bz < ncz)
        tp = np.where(ok, top[np.clip(bz, 0, ncz - 1) * ncx + np.clip(bx, 0, ncx - 1)], 0)
        ok &= tp != 0
        dx = ((f(2.0) * bx.astype(f) + f(1.0)).astype(f) - cx[cur]).astype(f)
        dz = ((f(2.0) * bz.astype(f) + f(1.0)).astype(f) - cz[cur]).astype(f)
        du = ((dx * ux).astype(f) + (dz * uz).astype(f)).astype(f)
        dn = ((dx * nx).astype(f) + (dz * nz).astype(f)).astype(f)
        ok &= ~((np.abs(dn) > f(R2 + f(0.01))) | (du < f(f(-2.0) * R - f(0.01))))
        h = (du - R2).astype(f)
        h = np.where(h > 0, h, f(0.0)).astype(f)
        v = ((tp.astype(f) + f(2.0)).astype(f) - (k * h).astype(f)).astype(f)
        H[cur] = np.maximum(H[cur], np.where(ok, v, f(0.0)).max(axis=0))   # H >= 0: a column that is not ok adds 0
    return np.ceil(H).astype(np.uint32).reshape(ncz, ncx)


_REF = {}
_HORIZON = {}


def _horizons(ct, sun, yt):
    """The three horizon statements, which read the column tops alone: once per set of tops."""
    key = (ct.shape, ct.tobytes(), np.asarray(sun, np.float32).tobytes(), yt)
    if key not in _HORIZON:
        _HORIZON[key] = {"safety": horizon_safety(ct, sun), "tightness": horizon_tightness(ct, sun),
                         "f32": horizon_f32(ct, sun, yt)}
    return _HORIZON[key]


def reference(vox, sun, key=None):
    """Every table's reference for these voxels, computed once per key (a world's name; None: not kept)."""
    if key is None or key not in _REF:
        ct, yt = coltop(vox), ytop(vox)
        ref = {"ytop": yt, "coltop": ct, "dtop": dtop(vox), **_horizons(ct, sun, yt)}
        if key is None:
            return ref
        _REF[key] = ref
    return _REF[key]


def check_tables(ref, yt, ct, hz, dt, label=""):
    """A built set of tables against `reference`: ytop, coltop and dtop equal; the horizon's three
    statements.  Returns the horizon's observed slack, (min, max) each: horizon - safety bound over the
    columns that have one (how much march the conservative 2R disc gives away; None in a world without a
    solid column) and tightness bound - horizon."""
    assert yt == ref["ytop"], (label, "ytop", yt, ref["ytop"])
    assert ct.dtype == np.uint32 and np.array_equal(ct, ref["coltop"]), (label, "coltop")
    assert dt.dtype == np.int32 and np.array_equal(dt, ref["dtop"]), (label, "dtop")
    lo, hi, h = ref["safety"], ref["tightness"], hz.astype(np.float64)
    assert hz.dtype == np.uint32 and hz.shape == lo.shape, (label, "horizon shape")
    assert (h >= lo).all(), (label, "horizon too eager: below the safety bound", float((h - lo).min()))
    assert (h <= hi).all(), (label, "horizon too timid: above the tightness bound", float((hi - h).min()))
    assert np.array_equal(hz, ref["f32"]), (label, "horizon differs from the float32 restatement")
    a = (h - lo)[np.isfinite(lo)]
    return ((float(a.min()), float(a.max())) if a.size else None, (float((hi - h).min()), float((hi - h).max())))


# ---------------------------------------------------------------- the edits both test files apply
EDIT_WORLD = ((8, 6, 7), lambda O: terrain_cut(O, 8, 6, 7, 56))   # open sky above row 55: the exits can move


def apply_boxes(vox, boxes):
    v = vox.copy()
    for x0, y0, z0, x1, y1, z1, solid in boxes:
        v[z0:z1, y0:y1, x0:x1] = bool(solid)
    return v


def edit_steps(vox):
    """(name, boxes) applied one after the other, all within the low-x half of the 256-wide world so
    that rv_world_edit takes its local rebuild: a set above the highest column (ytop and every horizon
    behind it rise), a clear of the top of the 2x2 column that stands highest over its 8 neighbours (its
    coltop, its neighbourhood's dtop and the horizons it raised drop), and a set in the corner brick (the
    clipped 3x3 neighbourhoods)."""
    t = tops(vox)
    Z, X = t.shape
    c2 = t.reshape(Z // 2, 2, X // 2, 2).max(axis=(1, 3))
    hi = int(t.max())
    pad = np.pad(c2, 1, constant_values=-1)
    around = np.max([pad[1 + j:1 + j + Z // 2, 1 + i:1 + i + X // 2] for j in (-1, 0, 1) for i in (-1, 0, 1)
                     if (i, j) != (0, 0)], axis=0)
    peak = (c2 - around)[:, :60]      # x < 120: the local rebuild's boxes still fall short of the whole grid
    pz, px = (2 * int(v) for v in np.unravel_index(np.argmax(peak), peak.shape))
    ptop = int(c2[pz // 2, px // 2])
    assert peak.max() > 0 and ptop >= 3 and hi + 6 <= vox.shape[1]
    return [("set above the highest column", [(21, hi + 3, 34, 22, hi + 5, 36, 1)]),
            ("clear the most prominent column's top", [(px, ptop - 3, pz, px + 2, ptop, pz + 2, 0)]),
            ("set in the corner brick", [(0, 5, Z - 3, 2, hi + 1, Z, 1)])]


def pillar_boxes(vox):
    """A 4 x 4 pillar up to three rows above the world's top, in the low-x quarter: into the skimming rays' path."""
    hi = int(tops(vox).max())
    return [(44, 0, 60, 48, hi + 3, 64, 1)]
