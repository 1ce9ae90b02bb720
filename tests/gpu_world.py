"""Context and frame plumbing shared by the test modules: the rv / sun fixtures, rank threads, world
arithmetic on the host (dims, voxels, pack, edited, the sparse-world generators), context exports (world,
tables, gi, images), twin comparisons and the oracle worlds the scroll tests compare with.  A test module
imports what it uses; the numpy restatements the GPU is checked against live in the np_*.py modules."""
import threading

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rv():
    import rvgrt_amd
    rvgrt_amd._lib.load()
    return rvgrt_amd


@pytest.fixture(scope="module")
def sun(oracle):
    return np.ascontiguousarray(oracle.sun_dir(), np.float32)


def run_ranks(fns, timeout=300):
    """Runs fns[q]() on N threads; re-raises the first failure."""
    errs = [None] * len(fns)

    def body(q):
        try:
            fns[q]()
        except BaseException as e:   # noqa: BLE001 -- re-raised below
            errs[q] = e
    ts = [threading.Thread(target=body, args=(q,)) for q in range(len(fns))]
    for th in ts:
        th.start()
    for th in ts:
        th.join(timeout=timeout)
        assert not th.is_alive(), "a rank thread hung"
    for e in errs:
        if e is not None:
            raise e


# ---------------------------------------------------------------- worlds on the host
def dims(lg):
    """Voxels per axis."""
    return tuple(1 << l for l in lg)


def cells(lg):
    """Coarse (CSDF) cells per axis: 2 voxels each."""
    return tuple(1 << (l - 1) for l in lg)


def gi_dims(lg):
    """GI cells per axis: 4 voxels each."""
    return tuple(1 << (l - 2) for l in lg)


def voxels(bits, lg):
    X, Y, Z = dims(lg)
    return np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(Z, Y, X).astype(bool)


def pack(vox):
    return np.packbits(vox.ravel(), bitorder="little").view(np.uint32)


def edited(bits, lg, boxes):
    """The canonical bit words after the boxes, applied in order on the host."""
    vox = voxels(bits, lg)
    for (x0, y0, z0, x1, y1, z1, s) in boxes:
        vox[z0:z1, y0:y1, x0:x1] = bool(s)
    return pack(vox)


def sparse_bits(lg, density, seed, exact=True):
    """Random bits.  exact: round(n * density) distinct voxels; else int(n * density) draws with replacement
    (fewer voxels where two draws coincide).  The two give different worlds for the same seed."""
    n = 1 << sum(lg)
    bits = np.zeros(n // 32, np.uint32)
    rng = np.random.default_rng(seed)
    idx = rng.choice(n, int(round(n * density)), replace=False) if exact else rng.choice(n, int(n * density))
    np.bitwise_or.at(bits, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return bits


def synthetic_voxels(kind, X, Y, Z, rng):
    """Dense [z, y, x] occupancy of one synthetic world."""
    if kind == "empty":
        return np.zeros((Z, Y, X), bool)
    if kind == "full":
        return np.ones((Z, Y, X), bool)
    if kind == "sparse":
        return rng.uniform(size=(Z, Y, X)) < 0.01
    if kind == "dense":
        return rng.uniform(size=(Z, Y, X)) < 0.40
    if kind == "pillars":            # a floor and 1-voxel pillars of mixed heights every 6 voxels
        v = np.zeros((Z, Y, X), bool)
        v[:, :8, :] = True
        h = rng.integers(10, Y - 10, (Z // 6 + 1, X // 6 + 1))
        for k in range(0, Z, 6):
            for i in range(0, X, 6):
                v[k, :h[k // 6, i // 6], i] = True
        return v
    if kind == "blocks":             # 4^3 blocks at 10 %, with a floor (ragged dims)
        b = rng.uniform(size=(Z // 4, Y // 4, X // 4)) < 0.10
        v = b.repeat(4, 0).repeat(4, 1).repeat(4, 2)
        v[:, :2, :] = True
        return v
    raise ValueError(kind)


# frame 4732006 seeds cell 3042 of a 64^3 world's 16^3 grid (an air cell near
# the top) with xorshift state idx + frame * 198491317 == 0 (mod 2^32): the
# fixed point that would keep the bounce-direction rejection loop drawing
# (-1, -1, -1) forever (src/CoarseArray.cu:258-268); such a state starts at
# 0x9E3779B9 instead, on both sides (rvgrt_amd/csrc/rv_kernels.hip gi_bounce_dir)
ZERO_SEED_FRAME, ZERO_SEED_CELL = 4732006, 3042


def step(axis, d):
    return (d, 0) if axis == 0 else (0, d)


def oracle_of(oracle, lg, bits, csdf=None, atlas=None):
    ow = oracle.OracleWorld(*lg, atlas=atlas)
    ow.bits[:] = bits
    if csdf is None:
        ow.build_csdf()
    else:
        ow.csdf[:] = csdf
    return ow


_GENERATED = {}


def generated(oracle, lg, origin, csdf=False):
    """The oracle's generated window at `origin`, built once per window: its bits, or (bits, csdf)."""
    key = (lg, origin, csdf)
    if key not in _GENERATED:
        ow = oracle.OracleWorld(*lg, ox=origin[0], oz=origin[1]).fill()
        _GENERATED[key] = (ow.bits.copy(), ow.build_csdf().csdf.copy()) if csdf else ow.bits.copy()
    return _GENERATED[key]


# ---------------------------------------------------------------- what a context holds
def world(rv, r):
    return r.world_export(rv.RV_WORLD_BITS), r.world_export(rv.RV_WORLD_CSDF)


def tables(rv, r):
    return (r.world_top_info(), r.world_export(rv.RV_WORLD_COLTOP), r.world_export(rv.RV_WORLD_HORIZON),
            r.world_export(rv.RV_WORLD_DTOP))


def same_tables(a, b, what):
    assert a[0] == b[0], what
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y), what


def gi(rv, r, lg=None):
    """The GI grid as uint32 cells: flat, or [z, y, x] of a world of these log2 dims."""
    g = r.world_export(rv.RV_WORLD_GI).view(np.uint32)
    return g if lg is None else g.reshape(gi_dims(lg)[::-1])


def images(rv, r):
    return [r.readback(k) for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH)]


def same_frames(rv, r, t, what):
    for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH):
        assert np.array_equal(r.readback(k), t.readback(k)), (what, k)
    assert np.array_equal(gi(rv, r), gi(rv, t)), what


def same_world(rv, r, t, what):
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, t.world_export(rv.RV_WORLD_BITS)), what
    assert np.array_equal(csdf, t.world_export(rv.RV_WORLD_CSDF)), what
    return bits, csdf


def twin_edit(rv, t, lg, boxes):
    t.world_import(rv.RV_WORLD_BITS, edited(t.world_export(rv.RV_WORLD_BITS), lg, boxes))
    t.csdf_build()


# ---------------------------------------------------------------- contexts and frames
def ctx128(rv, atlas, W, H, rays=None, edit=(), **kw):
    """A reference-flags context of the generated 128^3 world after one GI sweep, then these edit boxes."""
    if rays is not None:
        kw["gi_rays_per_frame"] = rays
    c = rv.StateRender((7, 7, 7), W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, **kw)
    c.world_build()
    c.gi_update(0)
    if edit:
        c.world_edit(edit)
    return c


def draw(r, d, update_gi=False):
    """drawCUDA with ref_compat: the jitterY argument is the frame time (Appendix R1)."""
    c = d.cam
    if update_gi:
        r.update_gi_data()
    r.draw_cuda(c.pos[:], c.forward[:], c.up[:], c.right[:], np.ctypeslib.as_array(d.vp),
                np.ctypeslib.as_array(d.prev_vp), 0.0, d.time)


def shifted(rv, d, dx, dz):
    cam, vp, pvp = rv.scroll_view(dx, dz, d.cam, np.ctypeslib.as_array(d.vp), np.ctypeslib.as_array(d.prev_vp))
    return rv.frame_desc(cam, vp, pvp, d.time, d.jitter_x, d.jitter_y)


def block_in_view(r, d, N):
    """Boxes on a ray through the frame (the centre ray, or tilted down until it hits ground): the hit
    block dug out, a block placed in the air 8 voxels before it.  Returns the boxes and the ray."""
    c = d.cam
    fo = np.asarray(c.forward[:], np.float64)
    for tilt in (0.0, 0.15, 0.3, 0.45):
        v = fo + tilt * np.array([0.0, -1.0, 0.0])
        v /= np.linalg.norm(v)
        ray = ([c.pos[:]], [v.astype(np.float32)], [0.0])
        h = r.trace_rays(*ray)[0]
        if h["hit"] and np.linalg.norm(np.asarray(h["pos"], np.float64) - np.asarray(c.pos[:])) > 16:
            break
    else:
        raise AssertionError("no ground in view")
    p = np.asarray(h["pos"], np.float64)
    a = np.clip(np.floor(p).astype(int) - 1, 0, N - 3)
    b = np.clip(np.floor(p - 8.0 * v).astype(int) - 1, 0, N - 3)
    return [(int(a[0]), int(a[1]), int(a[2]), int(a[0]) + 3, int(a[1]) + 3, int(a[2]) + 3, 0),
            (int(b[0]), int(b[1]), int(b[2]), int(b[0]) + 3, int(b[1]) + 3, int(b[2]) + 3, 1)], ray
