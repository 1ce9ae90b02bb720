"""rv_world_edit_shapes on the CPU: rv_world_edit_shapes_at -- the row function the kernel calls, evaluated on
the host over RV_WORLD_BITS words -- and rv_world_edit_shapes_box against the numpy restatement of the
definition (tests/np_shapes.py), exactly: every word of the world after the call, both counts, every box.
The scenes defined here are the ones tests/test_gpu_world_shapes.py runs on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gpu_world import pack, rv, voxels   # noqa: F401 -- rv is the fixture
import np_shapes as S
from test_world_detached import random32

E, CX, CY, CZ = S.ELLIPSOID, S.CYLINDER_X, S.CYLINDER_Y, S.CYLINDER_Z


def lg_of(vox):
    return tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])


def sphere(c2, r2, solid=1):
    return (E, solid, tuple(c2), (r2, r2, r2))


def check(rv, vox, shapes, what=None):
    """The host form against the restatement on this world; returns the restatement's (vox', n_set, n_cleared)."""
    lg = lg_of(vox)
    want = S.apply(vox, shapes)
    bits, n_set, n_cleared = rv.edit_shapes_at(lg, pack(vox), shapes)
    assert (n_set, n_cleared) == want[1:], (what, n_set, n_cleared, want[1:])
    assert np.array_equal(bits, pack(want[0])), (what, "bits")
    assert rv.edit_shapes_box(lg, shapes) == S.boxes(lg, shapes), (what, "boxes")
    return want


# ---------------------------------------------------------------- scenes (shared with the GPU tests)
# (shape, voxels set in an empty 32^3 world), counted from the definition in include/rvgrt.h (DESIGN s5.13)
KNOWN = [
    (sphere((33, 33, 33), 2), 7),
    (sphere((33, 33, 33), 6), 123),
    (sphere((33, 33, 33), 1), 1),
    (sphere((32, 32, 32), 2), 8),
    (sphere((32, 32, 32), 1), 0),          # box non-empty
    ((E, 1, (33, 33, 33), (7, 3, 5)), 61),
    ((CY, 1, (33, 33, 33), (6, 4, 6)), 145),   # 29 * 5
    (sphere((1, 33, 33), 6), 76),          # clipped at x = 0
]


def random_shapes(rng, lg, n, rmax=24, margin=12):
    """n random shapes of all kinds, centres up to `margin` half-voxels beyond the window's faces."""
    D = [2 << l for l in lg]   # the window in half-voxels
    out = []
    for _ in range(n):
        c2 = tuple(int(rng.integers(-margin, d + margin + 1)) for d in D)
        r2 = tuple(int(v) for v in rng.integers(1, rmax + 1, 3))
        out.append((int(rng.integers(0, 4)), int(rng.integers(0, 2)), c2, r2))
    return out


def scenes(lg):
    """Named shape lists for a window of these log2 dims (every axis >= 32 voxels)."""
    X, Y, Z = (1 << l for l in lg)
    rng = np.random.default_rng(sum(lg) * 977)
    sc = {
        # centred on a corner shared by eight bricks: straddles x = 0 (mod 8), y = 0 (mod 4) and the brick
        # boundaries of all three axes; both words of a brick row pair (y >> 2 & 1) on either side
        "brick_corner": [sphere((32, 32, 32), 11)],
        # centre on a voxel next to the boundaries, odd radii, an ellipsoid longer than a word along x
        "ellipsoid_x": [(E, 1, (2 * 15 + 1, 2 * 12 + 1, 2 * 23 + 1), (19, 5, 9)), (E, 0, (32, 24, 48), (7, 3, 4))],
        # one shape through each face of the window, centres inside, on and beyond it
        "faces": [sphere((1, Y, Z), 9), sphere((2 * X - 1, Y, Z), 9, 0), sphere((X, 0, Z), 8), sphere((X, 2 * Y, Z), 8, 0),
                  sphere((X, Y, -3), 10), sphere((X, Y, 2 * Z + 3), 10, 0)],
        # the three cylinders through the whole window and beyond
        "cylinders": [(CX, 1, (X, Y + 1, Z - 1), (512, 7, 5)), (CY, 0, (X + 1, Y, Z), (6, 512, 9)),
                      (CZ, 1, (X - 3, Y + 2, Z), (9, 4, 512))],
        # a shell, then a shaft drilled through it, then a boulder in the middle
        "shell": [sphere((X + 1, Y + 1, Z + 1), 26), sphere((X + 1, Y + 1, Z + 1), 20, 0),
                  (CY, 0, (X + 1, Y + 1, Z + 1), (6, 40, 6)), sphere((X + 1, Y + 1, Z + 1), 8)],
        "corner_and_outside": [sphere((0, 0, 0), 13), sphere((2 * X, 2 * Y, 2 * Z), 13, 0), sphere((-40, Y, Z), 20),
                               sphere((X, 2 * Y + 600, Z), 512, 0)],
        "many": random_shapes(rng, lg, S.MAX_SHAPES, rmax=10, margin=4),
        "random": random_shapes(rng, lg, 8),
    }
    sc["known"] = [s for s, _ in KNOWN]
    return sc


# ---------------------------------------------------------------- known counts
@pytest.mark.parametrize("i", range(len(KNOWN)))
def test_known_counts(rv, i):
    shape, count = KNOWN[i]
    empty = np.zeros((32, 32, 32), bool)
    want = check(rv, empty, [shape], shape)
    assert want[1:] == (count, 0)
    assert rv.edit_shapes_box((5, 5, 5), [shape])[0][0] != (0,) * 6
    # and cleared out of a solid world: the same voxels
    assert check(rv, ~empty, [(shape[0], 0) + shape[2:]], shape)[1:] == (0, count)


# ---------------------------------------------------------------- symmetry
@pytest.mark.parametrize("r2", [1, 2, 9, 13, 14, 21, 28])
def test_sphere_symmetry(rv, r2):
    """A voxel-centred sphere is invariant under the 48 permutations and reflections about its centre."""
    empty = np.zeros((32, 32, 32), bool)
    bits, n_set, _ = rv.edit_shapes_at((5, 5, 5), pack(empty), [sphere((33, 33, 33), r2)])
    v = voxels(bits, (5, 5, 5))[1:, 1:, 1:]   # 31^3 around voxel 16
    assert v.sum() == n_set and v[15, 15, 15]
    for perm in itertools.permutations(range(3)):
        t = v.transpose(perm)
        for fl in itertools.product((False, True), repeat=3):
            u = t[::-1] if fl[0] else t
            u = u[:, ::-1] if fl[1] else u
            u = u[:, :, ::-1] if fl[2] else u
            assert np.array_equal(u, v), (perm, fl)


def test_cylinders_are_transposes(rv):
    empty = np.zeros((32, 32, 32), bool)
    for c2, r2 in [((33, 31, 36), (9, 14, 5)), ((30, 33, 33), (512, 3, 8)), ((1, 70, 33), (12, 20, 7))]:
        y = voxels(rv.edit_shapes_at((5, 5, 5), pack(empty), [(CY, 1, c2, r2)])[0], (5, 5, 5))   # [z, y, x]
        swap = lambda t, i, j: tuple(t[j] if k == i else t[i] if k == j else t[k] for k in range(3))   # noqa: E731
        x = voxels(rv.edit_shapes_at((5, 5, 5), pack(empty), [(CX, 1, swap(c2, 0, 1), swap(r2, 0, 1))])[0], (5, 5, 5))
        z = voxels(rv.edit_shapes_at((5, 5, 5), pack(empty), [(CZ, 1, swap(c2, 1, 2), swap(r2, 1, 2))])[0], (5, 5, 5))
        assert y.any()
        assert np.array_equal(x, y.transpose(0, 2, 1)) and np.array_equal(z, y.transpose(1, 0, 2))


# ---------------------------------------------------------------- boxes
def test_boxes_bound_and_touch(rv):
    """Every set voxel lies inside its shape's box.  For a voxel-centred shape that the window does not clip,
    every face of the box holds an inside voxel: the voxel on the centre line, whose d is 0 on the other two
    axes.  (A corner-centred shape's face need not: the corner-centred r2 = 1 sphere of KNOWN has a box and no voxel.)"""
    lg = (6, 6, 6)
    rng = np.random.default_rng(5)
    empty = np.zeros((64, 64, 64), bool)
    for k in range(60):
        kind = k % 4
        c2 = tuple(int(2 * v + 1) for v in rng.integers(26, 38, 3))
        r2 = tuple(int(v) for v in rng.integers(1, 50, 3))
        shape = (kind, 1, c2, r2)
        (b,), u = rv.edit_shapes_box(lg, [shape])
        assert b == u == S.box(lg, shape)
        v = voxels(rv.edit_shapes_at(lg, pack(empty), [shape])[0], lg)
        out = v.copy()
        out[b[2]:b[5], b[1]:b[4], b[0]:b[3]] = False
        assert not out.any(), shape
        sub = v[b[2]:b[5], b[1]:b[4], b[0]:b[3]]
        for face in (sub[0], sub[-1], sub[:, 0], sub[:, -1], sub[:, :, 0], sub[:, :, -1]):
            assert face.any(), shape


# ---------------------------------------------------------------- order and counts
def test_shell_depends_on_order(rv):
    empty = np.zeros((32, 32, 32), bool)
    big, small = sphere((33, 33, 33), 20), sphere((33, 33, 33), 12, 0)
    shell = check(rv, empty, [big, small])
    ball = check(rv, empty, [small, big])
    assert shell[1] < ball[1] and not shell[0][16, 16, 16] and ball[0][16, 16, 16]
    assert ball[1] == S.apply(empty, [big])[1]


def test_counts_compare_before_with_after(rv):
    """A voxel set by one shape and cleared by a later one was not changed; neither was one that keeps its value."""
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :16] = True
    a, b = sphere((33, 32, 33), 10), sphere((33, 32, 33), 10, 0)
    n = int(S.inside(vox.shape, a).sum())
    assert n % 2 == 0 and n > 0
    assert check(rv, vox, [a])[1:] == (n // 2, 0)
    assert check(rv, vox, [b])[1:] == (0, n // 2)
    assert check(rv, vox, [a, b])[1:] == (0, n // 2)      # set, then cleared: only what was solid counts
    assert check(rv, vox, [b, a])[1:] == (n // 2, 0)
    assert check(rv, vox, [a, b, a, b, a])[1:] == (n // 2, 0)


@pytest.mark.parametrize("dims", [(32, 32, 32), (128, 32, 64)])   # [z, y, x]: 32^3 and 64 x 32 x 128
@pytest.mark.parametrize("seed", range(6))
def test_random_lists(rv, dims, seed):
    rng = np.random.default_rng(100 + seed)
    vox = rng.random(dims) < (0.0, 0.5, 1.0, 0.3, 0.5, 0.7)[seed]
    lg = lg_of(vox)
    for n in (1, 2, 3, 5, 8):
        check(rv, vox, random_shapes(rng, lg, n), (dims, seed, n))


@pytest.mark.parametrize("lg", [(5, 5, 5), (6, 6, 6), (7, 5, 6)])
def test_scenes(rv, lg):
    X, Y, Z = (1 << l for l in lg)
    rnd = np.random.default_rng(3).random((Z, Y, X)) < 0.5 if lg != (5, 5, 5) else random32(0.5, 3)
    for name, shapes in scenes(lg).items():
        for vox in (np.zeros((Z, Y, X), bool), np.ones((Z, Y, X), bool), rnd):
            check(rv, vox, shapes, (lg, name))


# ---------------------------------------------------------------- clipping
def test_clipping_at_the_six_faces(rv):
    lg = (5, 5, 5)
    empty = np.zeros((32, 32, 32), bool)
    whole = int(S.inside((96, 96, 96), sphere((97, 97, 97), 12)).sum())
    for a in range(3):
        for c in (1, 0, -5, 63, 64, 69):   # first / last voxel's centre, on the face, beyond it
            c2 = [33, 33, 33]
            c2[a] = c
            want = check(rv, empty, [sphere(c2, 12)], (a, c))
            assert 0 < want[1] < whole
    # wholly outside: empty boxes, unchanged bits, 0 / 0
    vox = random32(0.5, 9)
    outside = [sphere((-13, 33, 33), 12), sphere((33, 64 + 13, 33), 12, 0), sphere((33, 33, -600), 512),
               (CY, 0, (33, 33, 64 + 9), (8, 512, 8)), sphere((S.MAX_C2, 33, 33), 512, 0), sphere((33, -S.MAX_C2, 33), 512)]
    assert check(rv, vox, outside)[1:] == (0, 0)
    assert rv.edit_shapes_box(lg, outside) == ([(0,) * 6] * len(outside), (0,) * 6)
    assert rv.edit_shapes_box(lg, []) == ([], (0,) * 6)
    # touching the face from outside by exactly one voxel
    assert check(rv, empty, [sphere((-11, 33, 33), 12)])[1] == 1


# ---------------------------------------------------------------- extremes
def test_extremes(rv):
    lg = (6, 6, 6)
    empty = np.zeros((64, 64, 64), bool)
    R = S.MAX_R2
    assert check(rv, empty, [sphere((64, 64, 64), R)])[1] == 64 ** 3          # everything inside
    assert check(rv, ~empty, [sphere((64, 64, 64), R, 0)])[2] == 64 ** 3
    row = check(rv, empty, [(E, 1, (64, 65, 64), (R, 1, R))])                  # odd c2.y: the row y = 32
    assert row[1] == 64 * 64 and row[0][:, 32, :].all()
    assert check(rv, empty, [(E, 1, (64, 64, 64), (R, 1, R))])[1] == 0          # even c2.y: dy = +-1 leaves no room
    for kind in (CX, CY, CZ):
        assert check(rv, empty, [(kind, 1, (65, 65, 65), (R, R, R))])[1] == 64 ** 3
    # the far corner of the bit array, and the largest centre coordinates
    assert check(rv, empty, [sphere((127, 127, 127), 1)])[0][63, 63, 63]
    assert check(rv, empty, [sphere((128 + R - 1, 127, 127), R)])[1] >= 1
    for sgn in (1, -1):
        assert check(rv, ~empty, [(kind, 0, (sgn * S.MAX_C2,) * 3, (R, R, R)) for kind in range(4)])[1:] == (0, 0)


# ---------------------------------------------------------------- world_blast's settle boxes
def test_settle_parts(rv):
    """The parts tile the shape's box grown by one voxel and clipped, none above the cap, split along the
    longest axis; small boxes stay whole, an empty box gives none."""
    cap = rv.RV_DETACHED_MAX_VOXELS
    dims = (1024, 256, 512)
    assert rv.settle_parts((0,) * 6, dims) == []
    assert rv.settle_parts((10, 0, 500, 20, 9, 512), dims) == [(9, 0, 499, 21, 10, 512)]       # clipped at two faces
    assert rv.settle_parts((100, 100, 100, 226, 226, 226), dims) == [(99, 99, 99, 227, 227, 227)]   # 128^3: the cap itself
    assert rv.settle_parts((0, 0, 0, 4, 4, 9), dims, cap=125) == [(0, 0, 0, 5, 5, 5), (0, 0, 5, 5, 5, 10)]
    for box in [(100, 100, 100, 227, 226, 226), (300, 0, 200, 557, 256, 457), (0, 3, 0, 1024, 200, 512),
                (37, 1, 5, 166, 131, 262), (0, 20, 0, 1024, 30, 512)]:
        parts = rv.settle_parts(box, dims)
        grown = tuple(max(v - 1, 0) for v in box[:3]) + tuple(min(v + 1, d) for v, d in zip(box[3:], dims))
        vol = lambda b: (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])   # noqa: E731
        assert len(parts) >= 2 and all(0 < vol(p) <= cap for p in parts), box
        assert sum(vol(p) for p in parts) == vol(grown), box
        for i, p in enumerate(parts):
            assert all(grown[a] <= p[a] < p[3 + a] <= grown[3 + a] for a in range(3)), (box, p)
            for q in parts[:i]:      # no two parts overlap: with equal sums of volumes they tile the grown box
                assert any(p[3 + a] <= q[a] or q[3 + a] <= p[a] for a in range(3)), (box, p, q)
        # only parts above the cap were halved: the larger half of one is above half the cap
        assert max(vol(p) for p in parts) > cap // 2, box


# ---------------------------------------------------------------- status codes
def test_status_codes_leave_the_bits_alone(rv):
    from rvgrt_amd import _lib
    from rvgrt_amd.render import _edit_shapes
    L = _lib.load()
    bits = pack(random32(0.5, 4)).copy()
    keep = bits.copy()
    ptr = bits.ctypes.data_as(C.c_void_p)
    good = sphere((33, 33, 33), 40, 0)
    a, b = C.c_uint64(77), C.c_uint64(77)

    def at(shapes, n=None, lg=(5, 5, 5), p=ptr):
        arr = _edit_shapes(shapes) if shapes is not None else None
        return L.rv_world_edit_shapes_at(lg[0], lg[1], lg[2], p, arr, len(shapes) if n is None else n, C.byref(a), C.byref(b))

    def box(shapes, n=None, lg=(5, 5, 5), null_all=False):
        arr = _edit_shapes(shapes) if shapes is not None else None
        u = _lib.rv_voxel_box()
        return L.rv_world_edit_shapes_box(lg[0], lg[1], lg[2], arr, len(shapes) if n is None else n, None,
                                          None if null_all else C.byref(u))

    bad_lists = [
        ([good], -1), ([good] * (S.MAX_SHAPES + 1), None), (None, 1),
        ([good, (4, 0) + good[2:]], None), ([(-1, 0) + good[2:]], None),               # kind
        ([(E, 2) + good[2:]], None), ([(E, -1) + good[2:]], None),                     # solid
        ([(E, 1, (33, 33, 33), (0, 4, 4))], None), ([(E, 1, (33, 33, 33), (4, S.MAX_R2 + 1, 4))], None),
        ([(E, 1, (33, 33, 33), (4, 4, -3))], None),                                     # r2
        ([good, (E, 1, (S.MAX_C2 + 1, 33, 33), (4, 4, 4))], None), ([(E, 1, (33, 33, -S.MAX_C2 - 1), (4, 4, 4))], None),
    ]
    for shapes, n in bad_lists:
        assert at(shapes, n) == _lib.RV_ERR_INVALID, (shapes and shapes[-1], n)
        assert box(shapes, n) == _lib.RV_ERR_INVALID, (shapes and shapes[-1], n)
    for lg in [(4, 5, 5), (3, 5, 5), (5, 3, 5), (5, 5, 14), (12, 12, 12)]:
        assert at([good], lg=lg) == _lib.RV_ERR_INVALID, lg
        assert box([good], lg=lg) == _lib.RV_ERR_INVALID, lg
    assert at([good], p=None) == _lib.RV_ERR_INVALID
    assert box([good], null_all=True) == _lib.RV_ERR_INVALID
    assert np.array_equal(bits, keep) and (a.value, b.value) == (77, 77)
    # the valid edges
    assert at([], 0) == _lib.RV_OK and (a.value, b.value) == (0, 0) and np.array_equal(bits, keep)
    assert at(None, 0) == _lib.RV_OK and box(None, 0) == _lib.RV_OK
    assert at([good] * S.MAX_SHAPES) == _lib.RV_OK and not np.array_equal(bits, keep)
    assert L.rv_world_edit_shapes_at(5, 5, 5, ptr, _edit_shapes([good]), 1, None, None) == _lib.RV_OK
    # no context
    assert L.rv_world_edit_shapes(None, _edit_shapes([good]), 1, None, None) == _lib.RV_ERR_INVALID


def test_abi_version_and_struct_size(rv):
    from rvgrt_amd import _lib
    assert _lib.load().rv_abi_version() == 2
    assert C.sizeof(_lib.rv_edit_shape) == 32
    assert (_lib.RV_SHAPE_ELLIPSOID, _lib.RV_SHAPE_CYLINDER_X, _lib.RV_SHAPE_CYLINDER_Y, _lib.RV_SHAPE_CYLINDER_Z) == (
        E, CX, CY, CZ)
    assert (_lib.RV_EDIT_MAX_SHAPES, _lib.RV_SHAPE_MAX_R2) == (S.MAX_SHAPES, S.MAX_R2)
