"""rv_world_stamp on the CPU: rv_world_stamp_at -- the row function the kernel calls, evaluated on the host over
RV_WORLD_BITS words -- and rv_world_stamp_box against the numpy restatement of the definition
(tests/np_stamp.py), exactly: every word of the world after the call, both counts, every box.  The scenes
defined here are the ones tests/test_gpu_world_stamp.py runs on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from gpu_world import pack, rv, voxels   # noqa: F401 -- rv is the fixture
import np_stamp as N

SET, CLEAR, COPY = N.SET, N.CLEAR, N.COPY
SWAP, FX, FZ = N.SWAP_XZ, N.FLIP_X, N.FLIP_Z
LGS = [(5, 5, 5), (6, 6, 6), (7, 5, 6)]


def lg_of(vox):
    return tuple(int(n).bit_length() - 1 for n in vox.shape[::-1])


def rand_pattern(rng, nx, ny, nz, fill=0.5):
    """A random pattern [z, y, x] whose corner voxels are set, so that its extent is its dims."""
    p = rng.random((nz, ny, nx)) < fill
    p[0, 0, 0] = p[-1, -1, -1] = True
    return p


def worlds(lg):
    X, Y, Z = (1 << l for l in lg)
    return {"empty": np.zeros((Z, Y, X), bool), "solid": np.ones((Z, Y, X), bool),
            "random": np.random.default_rng(3 + sum(lg)).random((Z, Y, X)) < 0.5}


def check(rv, vox, pats, stamps, what=None):
    """The host forms against the restatement on this world; returns the restatement's (vox', n_set, n_cleared)."""
    lg = lg_of(vox)
    want = N.apply(vox, pats, stamps)
    bits, n_set, n_cleared = rv.stamp_at(lg, pack(vox), pats, stamps)
    assert (n_set, n_cleared) == want[1:], (what, n_set, n_cleared, want[1:])
    assert np.array_equal(bits, pack(want[0])), (what, "bits")
    assert rv.stamp_box(lg, pats, stamps) == N.boxes(lg, pats, stamps), (what, "boxes")
    assert rv.stamp_box(lg, [p.shape[::-1] for p in pats], stamps) == N.boxes(lg, pats, stamps), (what, "boxes from dims")
    return want


# ---------------------------------------------------------------- scenes (shared with the GPU tests)
def random_stamps(rng, lg, pats, n, margin=6):
    """n random stamps of all ops and orientations, reaching up to `margin` voxels beyond the window's faces."""
    D = [1 << l for l in lg]
    out = []
    for _ in range(n):
        i = int(rng.integers(0, len(pats)))
        at = tuple(int(rng.integers(-margin, d + margin - 2)) for d in D)
        out.append((i, int(rng.integers(0, 3)), int(rng.integers(0, 8)), at))
    return out


def scenes(lg):
    """name -> (patterns, stamps) for a window of these log2 dims (every axis >= 32 voxels)."""
    X, Y, Z = (1 << l for l in lg)
    rng = np.random.default_rng(sum(lg) * 131)
    sc = {}
    # rows of 1 .. 37 voxels at x offsets that are no multiple of 8 and y offsets that are no multiple of 4: a
    # word's run of 8 begins before the row, straddles its two words (33, 37) and ends past it; every op
    widths = [rand_pattern(rng, nx, 5, 3) for nx in (1, 8, 31, 32, 33, 37)]
    sc["widths"] = (widths, [(i, (SET, CLEAR, COPY)[(i + k) % 3], FX * k, (3 + 5 * i + 13 * k, 1 + 6 * k + i, 2 + 4 * i))
                             for i in range(6) for k in range(2)] +
                    [(4, COPY, 0, (X - 40 + 1, Y - 7, Z - 4)), (5, SET, FX, (X - 37, 9, Z - 9)), (5, CLEAR, 0, (-29, 13, 7))])
    # a single voxel, at the corners and in the middle
    one = [np.ones((1, 1, 1), bool), np.zeros((1, 1, 1), bool)]
    sc["unit"] = (one, [(0, SET, 0, (0, 0, 0)), (0, CLEAR, 7, (X - 1, Y - 1, Z - 1)), (0, COPY, 3, (13, 6, 21)),
                        (1, COPY, 0, (14, 6, 21)), (0, SET, 0, (15, 7, 9)), (0, CLEAR, 0, (16, 7, 9)), (1, SET, 0, (17, 7, 9)),
                        (0, SET, 5, (X, 3, 3)), (0, SET, 0, (-1, 3, 3))])
    # the longest patterns along each axis, in a world that clips them at both ends or at one
    long = [rand_pattern(rng, 256, 1, 1), rand_pattern(rng, 1, 256, 1), rand_pattern(rng, 1, 1, 256)]
    sc["long"] = (long, [(0, COPY, 0, (-100, 3, 5)), (0, SET, FX, (-250, 7, 9)), (0, CLEAR, 0, (X - 3, 11, 2)),
                         (1, COPY, 0, (5, -100, 6)), (1, SET, 0, (9, Y - 2, 8)), (2, COPY, FZ, (7, 2, -100)),
                         (2, CLEAR, SWAP, (-200, 5, 11)), (0, SET, SWAP | FZ, (21, 6, -131)), (2, SET, 0, (2, 9, Z - 1))])
    # negative offsets on each axis and on all, at offsets that are no multiples of the word
    blk = [rand_pattern(rng, 13, 7, 11), rand_pattern(rng, 37, 6, 9)]
    sc["negative"] = (blk, [(0, COPY, 0, (-5, 6, 9)), (0, SET, 1, (19, -3, 5)), (0, CLEAR, 2, (11, 9, -7)),
                            (1, COPY, 4, (-33, -2, -4)), (1, SET, 6, (-9, 13, 17)), (0, COPY, 3, (-12, -6, -10))])
    # one stamp through each face of the window, and stamps wholly outside it on every side
    sc["faces"] = (blk, [(0, COPY, 0, (-6, 9, 10)), (0, SET, 2, (X - 5, 10, 11)), (0, CLEAR, 0, (7, -3, 12)),
                         (1, COPY, 5, (3, Y - 2, 13)), (1, SET, 0, (5, 14, -4)), (1, CLEAR, 3, (9, 15, Z - 3)),
                         (0, COPY, 0, (-13, 5, 5)), (0, COPY, 0, (X, 5, 5)), (1, SET, 0, (5, -6, 5)), (1, SET, 0, (5, Y, 5)),
                         (0, CLEAR, 0, (5, 5, -11)), (0, CLEAR, 1, (5, 5, Z)), (0, COPY, 7, (N.MAX_AT, 0, 0)),
                         (1, COPY, 7, (0, -N.MAX_AT, 0)), (1, COPY, 1, (-N.MAX_AT, -N.MAX_AT, N.MAX_AT))])
    # the 8 orientations of a pattern with no symmetry and nx != nz, side by side and at a face
    asym = [rand_pattern(rng, 11, 4, 6), rand_pattern(rng, 35, 3, 9)]
    sc["orientations"] = (asym, [(0, COPY, o, (1 + 13 * (o % 2), 2 + 5 * (o // 4), 3 + 14 * (o // 2 % 2))) for o in range(8)] +
                          [(1, (SET, CLEAR)[o % 2], o, (X - 20 - o, 13 + o, Z - 5 - 3 * o)) for o in range(8)])
    # the three ops overlapping, in every order
    three = [rand_pattern(rng, 10, 6, 7), rand_pattern(rng, 9, 7, 8), rand_pattern(rng, 12, 5, 6)]
    sc["ops"] = (three, [(q, op, (q + k) % 8, (2 + 10 * (k % 3) + q, 3 + 14 * (k // 3) + 2 * q, 5 + q))
                         for k, perm in enumerate(itertools.permutations((SET, CLEAR, COPY))) for q, op in enumerate(perm)])
    # a masked paste: CLEAR with a hull, then SET with the object
    hull = np.ones((7, 9, 7), bool)
    obj = rand_pattern(rng, 7, 9, 7, 0.3)
    sc["masked"] = ([hull, obj], [(0, CLEAR, 0, (11, 5, 13)), (1, SET, 0, (11, 5, 13)), (0, CLEAR, 3, (-3, 20, Z - 4)),
                                  (1, SET, 3, (-3, 20, Z - 4))])
    small = [rand_pattern(rng, int(rng.integers(1, 9)), int(rng.integers(1, 7)), int(rng.integers(1, 9))) for _ in range(5)]
    sc["max"] = (small, random_stamps(rng, lg, small, N.MAX_STAMPS, margin=4))
    mixed = widths[2:] + blk + asym
    sc["random"] = (mixed, random_stamps(rng, lg, mixed, 12))
    return sc


@pytest.mark.parametrize("lg", LGS)
def test_scenes(rv, lg):
    for name, (pats, stamps) in scenes(lg).items():
        assert name != "max" or len(stamps) == rv._lib.RV_STAMP_MAX
        for wname, vox in worlds(lg).items():
            want = check(rv, vox, pats, stamps, (lg, name, wname))
            assert wname != "random" or want[1] + want[2] > 0, (lg, name)   # the scene did something


@pytest.mark.parametrize("lg", LGS)
@pytest.mark.parametrize("seed", range(4))
def test_random_lists(rv, lg, seed):
    rng = np.random.default_rng(500 + seed)
    vox = worlds(lg)["random"]
    pats = [rand_pattern(rng, int(rng.integers(1, 70)), int(rng.integers(1, 12)), int(rng.integers(1, 40))) for _ in range(4)]
    for n in (1, 2, 5, 9):
        want = check(rv, vox, pats, random_stamps(rng, lg, pats, n, margin=3), (lg, seed, n))
        assert n < 5 or want[1] + want[2] > 0, (lg, seed, n)


# ---------------------------------------------------------------- orientation
def test_orientation_by_hand(rv):
    """One voxel of a 2 x 1 x 3 pattern, at (sx, sz) = (1, 0), followed through the 8 orientations by the
    header's formulas, worked out by hand: (u, w) with oriented dims (ox, oz)."""
    pat = np.zeros((3, 1, 2), bool)
    pat[0, 0, 1] = True
    where = {0: (1, 0), FX: (0, 0), FZ: (1, 2), FX | FZ: (0, 2),
             SWAP: (0, 1), SWAP | FX: (2, 1), SWAP | FZ: (0, 0), SWAP | FX | FZ: (2, 0)}
    empty = np.zeros((32, 32, 32), bool)
    for o, (u, w) in where.items():
        want = check(rv, empty, [pat], [(0, SET, o, (9, 5, 17))], o)
        assert want[1] == 1 and want[0][17 + w, 5, 9 + u], o
        assert N.oriented(pat, o).shape == ((2, 1, 3) if o & SWAP else (3, 1, 2))


def test_eight_orientations_differ_and_a_quarter_turn_has_order_four(rv):
    rng = np.random.default_rng(8)
    pat = rand_pattern(rng, 11, 4, 6)
    lg, empty = (5, 5, 5), np.zeros((32, 32, 32), bool)
    got = []
    for o in range(8):
        want = check(rv, empty, [pat], [(0, COPY, o, (3, 5, 7))], o)
        ox, oz = (6, 11) if o & SWAP else (11, 6)
        got.append(np.pad(want[0][7:7 + oz, 5:9, 3:3 + ox], ((0, 11 - oz), (0, 0), (0, 11 - ox))))
        assert np.array_equal(voxels(rv.stamp_at(lg, pack(empty), [pat], [(0, COPY, o, (3, 5, 7))])[0], lg)[7:7 + oz, 5:9, 3:3 + ox],
                              N.oriented(pat, o))
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(got[i], got[j]), (i, j)
    # SWAP_XZ | FLIP_X is a quarter turn: four of them about a centre give the original back.  The turned
    # pattern is read out of the host form's world and stamped again.
    cur = pat
    for k in range(4):
        bits, _, _ = rv.stamp_at(lg, pack(empty), [cur], [(0, COPY, SWAP | FX, (9, 2, 9))])
        nz, ny, nx = cur.shape
        cur = voxels(bits, lg)[9:9 + nx, 2:2 + ny, 9:9 + nz].copy()
        assert (k == 3) == np.array_equal(cur, pat), k
    # and the quarter turn the other way undoes it
    turned = N.oriented(pat, SWAP | FX)
    assert np.array_equal(N.oriented(turned, SWAP | FZ), pat)


# ---------------------------------------------------------------- layout
def test_pattern_layout_and_junk_bits(rv):
    """The ABI's layout by hand, and bits at x >= nx of a row's last word ignored."""
    from rvgrt_amd import _lib
    from rvgrt_amd.render import _stamps
    L = _lib.load()
    rng = np.random.default_rng(21)
    for nx in (1, 8, 31, 32, 33, 37):
        pat = rand_pattern(rng, nx, 3, 2)
        dims, words = rv.render.pattern_bits(pat)
        nwx = (nx + 31) // 32
        assert dims == (nx, 3, 2) and words.size == nwx * 3 * 2
        for z, y, x in np.argwhere(np.ones_like(pat)):
            assert bool(words[(x >> 5) + nwx * (y + 3 * z)] >> np.uint32(x & 31) & np.uint32(1)) == pat[z, y, x]
        assert np.array_equal(rv.render.pattern_voxels(dims, words), pat)
        junk = words.copy()
        if nx % 32:
            junk[nwx - 1::nwx] |= np.uint32((0xFFFFFFFF << (nx % 32)) & 0xFFFFFFFF)
        vox = np.random.default_rng(22).random((32, 32, 32)) < 0.5
        for op in (SET, CLEAR, COPY):
            for o in (0, FX, SWAP, SWAP | FX | FZ):
                stamps = [(0, op, o, (5, 3, 7)), (0, op, o, (-3, 9, -1))]
                bits = pack(vox).copy()
                ph = (_lib.rv_pattern_host * 1)(_lib.rv_pattern_host(nx, 3, 2, junk.ctypes.data))
                a, b = C.c_uint64(), C.c_uint64()
                assert L.rv_world_stamp_at(5, 5, 5, bits.ctypes.data_as(C.c_void_p), ph, 1, _stamps(stamps), 2,
                                           C.byref(a), C.byref(b)) == 0
                want = N.apply(vox, [pat], stamps)
                assert np.array_equal(bits, pack(want[0])) and (a.value, b.value) == want[1:], (nx, op, o)


# ---------------------------------------------------------------- ops, order and counts
def test_ops_by_hand(rv):
    vox = np.zeros((32, 32, 32), bool)
    vox[:, :16] = True
    pat = np.zeros((2, 2, 2), bool)
    pat[0, :, 0] = True                      # the column x = 0, z = 0, two voxels high
    at = (8, 15, 8)                          # one voxel in rock, one in air
    assert check(rv, vox, [pat], [(0, SET, 0, at)])[1:] == (1, 0)
    assert check(rv, vox, [pat], [(0, CLEAR, 0, at)])[1:] == (0, 1)
    assert check(rv, vox, [pat], [(0, COPY, 0, at)])[1:] == (1, 3)      # the other three rock voxels of the box go
    assert check(rv, vox, [pat], [(0, SET, 0, at), (0, CLEAR, 0, at)])[1:] == (0, 1)   # set, then cleared: not changed
    assert check(rv, vox, [pat], [(0, CLEAR, 0, at), (0, SET, 0, at)])[1:] == (1, 0)
    assert check(rv, vox, [pat], [(0, COPY, 0, at), (0, COPY, FX, at)])[1:] == (1, 3)
    assert check(rv, vox, [pat], [(0, COPY, 0, at), (0, COPY, FX, at)])[0][8, 16, 9]


def test_a_later_stamp_wins(rv):
    rng = np.random.default_rng(31)
    vox = rng.random((32, 32, 32)) < 0.5
    a, b = rand_pattern(rng, 12, 9, 10), rand_pattern(rng, 10, 12, 9)
    for ops in itertools.product((SET, CLEAR, COPY), repeat=2):
        s = [(0, ops[0], 1, (7, 6, 5)), (1, ops[1], 6, (10, 3, 9))]
        first, second = check(rv, vox, [a, b], s, ops), check(rv, vox, [a, b], s[::-1], ops)
        # two SETs or two CLEARs commute; every other pair depends on its order
        assert np.array_equal(first[0], second[0]) == (ops in ((SET, SET), (CLEAR, CLEAR))), ops


# ---------------------------------------------------------------- clipping
def test_clipping_at_the_six_faces(rv):
    lg = (5, 5, 5)
    empty = np.zeros((32, 32, 32), bool)
    pat = np.ones((6, 6, 6), bool)
    for a in range(3):
        for at_a, n in ((-5, 1), (-1, 5), (0, 6), (26, 6), (27, 5), (31, 1), (32, 0), (-6, 0)):
            at = [13, 13, 13]
            at[a] = at_a
            want = check(rv, empty, [pat], [(0, SET, 0, tuple(at))], (a, at_a))
            assert want[1] == 36 * n
            assert (rv.stamp_box(lg, [pat], [(0, SET, 0, tuple(at))])[1] == N.ZERO) == (n == 0)
    vox = worlds(lg)["random"]
    outside = [(0, COPY, 0, (-6, 5, 5)), (0, COPY, 0, (5, 32, 5)), (0, CLEAR, 0, (5, 5, -N.MAX_AT)), (0, SET, 7, (N.MAX_AT,) * 3)]
    assert check(rv, vox, [pat], outside)[1:] == (0, 0)
    assert rv.stamp_box(lg, [pat], outside) == ([N.ZERO] * 4, N.ZERO)
    assert rv.stamp_box(lg, [pat], []) == ([], N.ZERO)
    assert rv.stamp_box(lg, [], []) == ([], N.ZERO)


def test_far_corners(rv):
    lg = (5, 5, 6)
    vox = np.random.default_rng(41).random((64, 32, 32)) < 0.5
    pat = rand_pattern(np.random.default_rng(42), 256, 2, 256, 0.5)
    for o in range(8):
        check(rv, vox, [pat], [(0, COPY, o, (-224, 30, -192)), (0, SET, o, (31, -1, 63)), (0, CLEAR, o, (-255, 31, -255))], o)
    full = np.ones((256, 256, 256), bool)
    assert check(rv, vox, [full], [(0, COPY, 3, (-100, -100, -100))])[0].all()
    assert not check(rv, vox, [full], [(0, CLEAR, 6, (-224, -224, -192))])[0].any()


# ---------------------------------------------------------------- status codes
def test_status_codes_leave_the_bits_alone(rv):
    from rvgrt_amd import _lib
    from rvgrt_amd.render import _patterns_host, _stamps
    L = _lib.load()
    bits = pack(worlds((5, 5, 5))["random"]).copy()
    keep = bits.copy()
    ptr = bits.ctypes.data_as(C.c_void_p)
    pat = np.ones((4, 4, 4), bool)
    pats, alive = _patterns_host([pat, pat], True)
    good = (0, COPY, 0, (3, 3, 3))
    a, b = C.c_uint64(77), C.c_uint64(77)

    def at(stamps, n=None, lg=(5, 5, 5), p=ptr, ph=pats, npats=2):
        arr = _stamps(stamps) if stamps is not None else None
        return L.rv_world_stamp_at(lg[0], lg[1], lg[2], p, ph, npats, arr, len(stamps) if n is None else n, C.byref(a), C.byref(b))

    def box(stamps, n=None, lg=(5, 5, 5), ph=pats, npats=2, null_all=False):
        arr = _stamps(stamps) if stamps is not None else None
        u = _lib.rv_voxel_box()
        return L.rv_world_stamp_box(lg[0], lg[1], lg[2], ph, npats, arr, len(stamps) if n is None else n, None,
                                    None if null_all else C.byref(u))

    bad_lists = [
        ([good], -1), ([good] * (N.MAX_STAMPS + 1), None), (None, 1),
        ([good, (2, COPY, 0, (3, 3, 3))], None), ([(-1, COPY, 0, (3, 3, 3))], None),          # pattern
        ([good, (0, 3, 0, (3, 3, 3))], None), ([(0, -1, 0, (3, 3, 3))], None),                # op
        ([good, (0, SET, 8, (3, 3, 3))], None), ([(0, SET, -1, (3, 3, 3))], None),            # orient
        ([good, (0, SET, 0, (N.MAX_AT + 1, 3, 3))], None), ([(0, SET, 0, (3, -N.MAX_AT - 1, 3))], None),
        ([(0, SET, 0, (3, 3, N.MAX_AT + 1))], None),                                           # at
    ]
    for stamps, n in bad_lists:
        assert at(stamps, n) == _lib.RV_ERR_INVALID, (stamps and stamps[-1], n)
        assert box(stamps, n) == _lib.RV_ERR_INVALID, (stamps and stamps[-1], n)
    for lg in [(4, 5, 5), (3, 5, 5), (5, 3, 5), (5, 5, 14), (12, 12, 12)]:
        assert at([good], lg=lg) == _lib.RV_ERR_INVALID, lg
        assert box([good], lg=lg) == _lib.RV_ERR_INVALID, lg
    assert at([good], p=None) == _lib.RV_ERR_INVALID
    assert box([good], null_all=True) == _lib.RV_ERR_INVALID
    # the patterns: a NULL array, a negative count, bad dims, NULL bits (the box form reads none)
    assert at([good], ph=None) == _lib.RV_ERR_INVALID and box([good], ph=None) == _lib.RV_ERR_INVALID
    assert at([good], npats=-1) == _lib.RV_ERR_INVALID and box([good], npats=-1) == _lib.RV_ERR_INVALID
    assert at([good], npats=0) == _lib.RV_ERR_INVALID and box([good], npats=0) == _lib.RV_ERR_INVALID
    for dims in [(0, 4, 4), (4, 257, 4), (4, 4, -1)]:
        bad = (_lib.rv_pattern_host * 2)(pats[0], _lib.rv_pattern_host(*dims, pats[1].bits))
        assert at([good], ph=bad) == _lib.RV_ERR_INVALID and box([good], ph=bad) == _lib.RV_ERR_INVALID, dims
    nobits = (_lib.rv_pattern_host * 2)(pats[0], _lib.rv_pattern_host(4, 4, 4, None))
    assert at([good], ph=nobits) == _lib.RV_ERR_INVALID and box([good], ph=nobits) == _lib.RV_OK
    assert np.array_equal(bits, keep) and (a.value, b.value) == (77, 77)
    # the valid edges
    assert at([], 0) == _lib.RV_OK and (a.value, b.value) == (0, 0) and np.array_equal(bits, keep)
    assert at(None, 0) == _lib.RV_OK and box(None, 0) == _lib.RV_OK and at(None, 0, ph=None, npats=0) == _lib.RV_OK
    edge = [(1, COPY, 7, (N.MAX_AT, -N.MAX_AT, N.MAX_AT)), good] * (N.MAX_STAMPS // 2)
    assert at(edge) == _lib.RV_OK and not np.array_equal(bits, keep)
    assert L.rv_world_stamp_at(5, 5, 5, ptr, pats, 2, _stamps([good]), 1, None, None) == _lib.RV_OK
    # no context
    assert L.rv_world_stamp(None, _stamps([good]), 1, None, None, None) == _lib.RV_ERR_INVALID
    assert L.rv_pattern_destroy(None, 0) == _lib.RV_ERR_INVALID
    assert L.rv_world_stamp_info(None, None, None, None, None) == _lib.RV_ERR_INVALID
    del alive


def test_abi_version_and_struct_sizes(rv):
    from rvgrt_amd import _lib
    assert _lib.load().rv_abi_version() == 2
    assert C.sizeof(_lib.rv_stamp) == 24 and C.sizeof(_lib.rv_pattern_host) == 24
    assert (_lib.RV_STAMP_SET, _lib.RV_STAMP_CLEAR, _lib.RV_STAMP_COPY) == (SET, CLEAR, COPY)
    assert (_lib.RV_ORIENT_SWAP_XZ, _lib.RV_ORIENT_FLIP_X, _lib.RV_ORIENT_FLIP_Z) == (SWAP, FX, FZ)
    assert (_lib.RV_PATTERN_MAX_DIM, _lib.RV_PATTERN_MAX, _lib.RV_STAMP_MAX) == (N.MAX_DIM, N.MAX_PATTERNS, N.MAX_STAMPS)
