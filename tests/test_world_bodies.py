"""rv_world_bodies_move on the CPU: the definition's invariants on the numpy restatement (tests/np_bodies.py),
and rv_world_bodies_move_at -- the function the kernel calls, evaluated on the host over RV_WORLD_BITS words
-- against that restatement bit for bit: lo as uint32 and flags."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import generated, pack, rv, synthetic_voxels, voxels
import np_bodies as B

F = np.float32


def _same(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "lo")
    assert np.array_equal(got[1], want[1]), (what, "flags")


@pytest.fixture(scope="module")
def world32():
    return B.random_world()


@pytest.fixture(scope="module")
def chained(world32):
    """4 chained steps of random bodies through the 32^3 world, per edge mode: the inputs and the
    restatement's outputs of every step, computed once."""
    steps = {}
    for mode in (0, B.OPEN_EDGES):
        rng = np.random.default_rng(11 + mode)
        lo, size, _ = B.random_bodies(rng, 1500, (32, 32, 32))
        seq = []
        for s in range(4):
            delta = B.random_bodies(rng, len(lo), (32, 32, 32))[2]
            out, fl = B.move(world32, lo, size, delta, mode)
            seq.append((lo, size, delta, out, fl))
            lo = out
        steps[mode] = seq
    return steps


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("mode", [0, B.OPEN_EDGES])
def test_invariants(world32, chained, mode):
    vox, op = world32, bool(mode)
    free = blocked = free_unblocked = start_solid = total = 0
    for (lo, size, delta, out, fl) in chained[mode]:
        assert not (fl & B.INVALID).any()
        for n in range(len(lo)):
            slabs = {}
            o, f = B.move_one(vox, lo[n], size[n], delta[n], op, slabs)
            assert np.array_equal(o.view(np.uint32), out[n].view(np.uint32)) and f == fl[n]
            total += 1
            start_solid += bool(f & B.START_SOLID)
            after = B.box_cells(vox, op, [B.occ(o[a], size[n][a]) for a in range(3)])[0]
            if not f & B.START_SOLID:
                free += 1
                assert not after, ("I1", n, lo[n], size[n], delta[n])
                blocked += bool(f & 63)
                free_unblocked += not f & 63
            for a in range(3):
                d, hit = delta[n][a], f & (3 << (2 * a))
                assert (o[a] - lo[n][a]) * d >= 0, ("I2", n, a)                       # 0 or along d
                assert hit in (0, (2 if d > 0 else 1) << (2 * a)), ("flag", n, a)
                if not hit:                                                           # I3
                    want = F(lo[n][a] + d) if d != 0 else lo[n][a]
                    assert o[a].view(np.uint32) == want.view(np.uint32), ("I3", n, a)
                    assert a not in slabs
                else:                                                                 # I4, by dense slices
                    i, r, before = slabs[a]
                    assert B.box_cells(vox, op, r)[0], ("I4 blocking", n, a)
                    for b in before:
                        r[a] = (b, b)
                        assert not B.box_cells(vox, op, r)[0], ("I4 before", n, a)
            if not f & 63:
                assert not f & B.EDGE
    # the inputs exercise both outcomes
    assert blocked >= free / 4 and free_unblocked >= free / 4, (free, blocked, free_unblocked)
    assert start_solid <= 0.6 * total, (start_solid, total)


# ---------------------------------------------------------------- the library's function == the restatement
@pytest.mark.parametrize("mode", [0, B.OPEN_EDGES])
def test_move_at_random_world(rv, world32, chained, mode):
    bits = pack(world32)
    for s, (lo, size, delta, out, fl) in enumerate(chained[mode]):
        _same(rv.bodies_move_at((5, 5, 5), bits, lo, size, delta, mode), (out, fl), (mode, s))


@pytest.mark.parametrize("kind", ["pillars", "blocks"])
def test_move_at_synthetic(rv, kind):
    vox = synthetic_voxels(kind, 32, 32, 64, np.random.default_rng(3))
    rng = np.random.default_rng(4)
    for mode in (0, B.OPEN_EDGES):
        lo, size, delta = B.random_bodies(rng, 600, (32, 32, 64))
        _same(rv.bodies_move_at((5, 5, 6), pack(vox), lo, size, delta, mode), B.move(vox, lo, size, delta, mode),
              (kind, mode))


def test_move_at_terrain(rv, oracle):
    lg = (7, 7, 7)
    bits = generated(oracle, lg, (0, 0))
    vox = voxels(bits, lg)
    rng = np.random.default_rng(6)
    lo, size, delta = B.random_bodies(rng, 800, (128, 128, 128))
    top = vox.any(axis=(0, 2)).nonzero()[0].max()
    lo[::2, 1] = np.minimum(lo[::2, 1], F(top + 3))         # half of them down where the terrain is
    want = B.move(vox, lo, size, delta, 0)
    assert (want[1] & 63).any() and (want[1] & B.START_SOLID).any() and not (want[1] & B.START_SOLID).all()
    _same(rv.bodies_move_at(lg, bits, lo, size, delta), want, "terrain")


@pytest.mark.parametrize("mode", [0, B.OPEN_EDGES])
def test_mask_boundaries(rv, mode):
    """Cross-sections over x = 7..8, 7..16, 31..32, y = 3..4, 7..8, z = 7..8 and a 16-wide body, in a world
    dense enough that which voxel of a word is read matters."""
    vox = np.random.default_rng(9).uniform(size=(32, 32, 64)) < 0.03
    vox[:, :2, :] = True
    lo, size, delta = B.straddling_bodies((64, 32, 32))
    want = B.move(vox, lo, size, delta, mode)
    assert (want[1] & 63).any() and ((want[1] & 63) == 0).any()
    _same(rv.bodies_move_at((6, 5, 5), pack(vox), lo, size, delta, mode), want, mode)
    # a single solid voxel on either side of each boundary stops the body exactly there
    for (x, y, z) in [(7, 5, 8), (8, 5, 7), (16, 4, 7), (31, 4, 8), (32, 7, 7), (33, 8, 8)]:
        one = np.zeros((32, 32, 64), bool)
        one[z, y, x] = True
        for a, d in ((0, 6.0), (0, -6.0), (1, 6.0), (1, -6.0), (2, 6.0), (2, -6.0)):
            p = np.array([x, y, z], F) - F(0.5)
            p[a] -= F(d / 2)
            dl = np.zeros(3, F)
            dl[a] = d
            got = rv.bodies_move_at((6, 5, 5), pack(one), [p], (2.0, 2.0, 2.0), dl, mode)
            _same(got, B.move(one, [p], (2.0, 2.0, 2.0), dl, mode), (x, y, z, a, d))
            assert got[1][0] == (2 if d > 0 else 1) << (2 * a)
            assert got[0][0][a] == (np.array([x, y, z])[a] - 2.0 if d > 0 else np.array([x, y, z])[a] + 1.0)


# ---------------------------------------------------------------- special cases
def test_resting_body_stays_put(rv, oracle):
    lg = (7, 7, 7)
    bits = generated(oracle, lg, (0, 0))
    vox = voxels(bits, lg)
    x, z = 40, 77
    top = int(vox[z:z + 1, :, x:x + 1].nonzero()[1].max()) + 1
    lo = np.array([[x + 0.2, top, z + 0.2]], F)
    for _ in range(50):
        out, fl = rv.bodies_move_at(lg, bits, lo, (0.6, 1.8, 0.6), (0.0, -0.1, 0.0))
        assert np.array_equal(out.view(np.uint32), lo.view(np.uint32)) and fl[0] == B.YN
        lo = out


def test_falling_body_lands_on_its_column(rv, oracle):
    lg = (7, 7, 7)
    bits = generated(oracle, lg, (0, 0))
    vox = voxels(bits, lg)
    rng = np.random.default_rng(2)
    xz = rng.integers(1, 126, (200, 2))
    xz = xz[[vox[z, 120:, x].sum() == 0 for x, z in xz]][:40]      # columns that end below the start
    assert len(xz) == 40
    lo = np.stack([xz[:, 0] + 0.125, np.full(40, 126.3), xz[:, 1] + 0.125], 1).astype(F)
    tops = np.array([vox[z, :, x].nonzero()[0].max() + 1 for x, z in xz], F)
    for _ in range(4):                                          # 4 x 40 rows: further than the world is high
        lo, fl = rv.bodies_move_at(lg, bits, lo, (0.75, 0.75, 0.75), (0.0, -40.0, 0.0))
    assert np.array_equal(lo[:, 1], tops) and (fl == B.YN).all()
    assert np.array_equal(lo[:, 0], (xz[:, 0] + 0.125).astype(F))


def test_overlap_query(rv, world32):
    rng = np.random.default_rng(8)
    lo, size, _ = B.random_bodies(rng, 600, (32, 32, 32))
    for mode in (0, B.OPEN_EDGES):
        out, fl = rv.bodies_move_at((5, 5, 5), pack(world32), lo, size, (0.0, 0.0, 0.0), mode)
        assert np.array_equal(out.view(np.uint32), lo.view(np.uint32))
        want = [B.START_SOLID if B.box_cells(world32, bool(mode), [B.occ(l[a], s[a]) for a in range(3)])[0] else 0
                for l, s in zip(lo, size)]
        assert fl.tolist() == want and 0 < sum(want) < 64 * len(want)


def test_invalid_bodies(rv, world32):
    bits = pack(world32)
    good = np.array([5.5, 9.0, 5.5, 1.0, 1.0, 1.0, 0.5, -0.5, 0.25], F)
    nan = np.array([0x7FC12345], np.uint32).view(F)[0]          # a NaN with a payload
    bad = []
    for field in range(9):
        values = [nan, F(np.inf), F(-np.inf)]
        values += [[F(16384.5), F(-16385)], [F(1 / 64), F(16.5), F(0), F(-1)], [F(64.5), F(-65)]][field // 3]
        for v in values:
            b = good.copy()
            b[field] = v
            bad.append(b)
    bad = np.array(bad, F)
    out, fl = rv.bodies_move_at((5, 5, 5), bits, bad[:, 0:3], bad[:, 3:6], bad[:, 6:9])
    assert (fl == B.INVALID).all()
    assert np.array_equal(out.view(np.uint32), bad[:, 0:3].view(np.uint32))        # bit for bit, payload included
    _same((out, fl), B.move(world32, bad[:, 0:3], bad[:, 3:6], bad[:, 6:9]), "invalid")
    # the bounds themselves are valid
    edge = np.array([[16384, 9, -16384, 1 / 32, 16, 1, 64, -64, 0]], F)
    out, fl = rv.bodies_move_at((5, 5, 5), bits, edge[:, 0:3], edge[:, 3:6], edge[:, 6:9], B.OPEN_EDGES)
    assert not fl[0] & B.INVALID
    _same((out, fl), B.move(world32, edge[:, 0:3], edge[:, 3:6], edge[:, 6:9], B.OPEN_EDGES), "bounds")


def test_walls_floor_and_edge_flag(rv):
    empty = np.zeros((32, 32, 32), bool)
    bits = pack(empty)
    at = lambda lo, d, mode=0: rv.bodies_move_at((5, 5, 5), bits, [lo], (1.0, 1.0, 1.0), d, mode)   # noqa: E731
    # the floor under an empty world, in both modes and outside the window too
    for mode, x in ((0, 10.0), (B.OPEN_EDGES, 10.0), (B.OPEN_EDGES, -7.5)):
        out, fl = at((x, 2.5, 10.0), (0, -5, 0), mode)
        assert out[0].tolist() == [x, 0.0, 10.0] and fl[0] == B.YN | B.EDGE
    # the window's walls stop a body at the last cell; with open edges it leaves
    out, fl = at((30.5, 5.0, 10.0), (4, 0, 0))
    assert out[0].tolist() == [31.0, 5.0, 10.0] and fl[0] == B.XP | B.EDGE
    out, fl = at((1.5, 5.0, 1.25), (-4, 0, -4))
    assert out[0].tolist() == [0.0, 5.0, 0.0] and fl[0] == B.XN | B.ZN | B.EDGE
    out, fl = at((30.5, 5.0, 10.0), (4, 0, 0), B.OPEN_EDGES)
    assert out[0].tolist() == [34.5, 5.0, 10.0] and fl[0] == 0
    # outside the window: in solid with walls, free with open edges
    assert at((40.0, 5.0, 10.0), (0, 0, 0))[1][0] == B.START_SOLID
    assert at((40.0, 5.0, 10.0), (0, 0, 0), B.OPEN_EDGES)[1][0] == 0
    # above the window nothing is solid: a body rises out of it and back
    out, fl = at((10.0, 30.5, 10.0), (0, 8, 0))
    assert out[0].tolist() == [10.0, 38.5, 10.0] and fl[0] == 0
    # a voxel in the blocking slab: no EDGE, even next to the wall
    one = empty.copy()
    one[10, 5, 31] = True
    out, fl = rv.bodies_move_at((5, 5, 5), pack(one), [(28.5, 5.0, 10.0)], (1.0, 1.0, 1.0), (4, 0, 0))
    assert out[0].tolist() == [30.0, 5.0, 10.0] and fl[0] == B.XP
    # ... and the wall and a voxel together in one slab: the voxel is inside the window, so no EDGE
    out, fl = rv.bodies_move_at((5, 5, 5), pack(one), [(31.25, 5.0, 11.25)], (1.0, 1.0, 1.0), (0, 0, -3))
    assert fl[0] == B.ZN | B.START_SOLID and out[0][2] == 11.0
    one[10, 5, 31] = False
    out, fl = rv.bodies_move_at((5, 5, 5), pack(one), [(31.25, 5.0, 11.25)], (1.0, 1.0, 1.0), (0, 0, -3))
    assert fl[0] == B.ZN | B.START_SOLID | B.EDGE and out[0][2] == 11.0


# ---------------------------------------------------------------- the ABI without a GPU
def test_struct_sizes(rv):
    assert C.sizeof(rv._lib.rv_body) == 36 and C.sizeof(rv._lib.rv_body_out) == 16


def test_status_codes(rv, world32):
    L, lib = rv._lib.load(), rv._lib
    bits = pack(world32)
    b = np.zeros((4, 9), F)
    b[:, 3:6] = 1
    out = np.zeros((4, 4), np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    at = lambda lg, bits_, in_, n, fl, out_: L.rv_world_bodies_move_at(*lg, bits_, in_, n, fl, out_)   # noqa: E731
    assert at((5, 5, 5), p(bits), p(b), 4, 0, p(out)) == lib.RV_OK
    assert at((5, 5, 5), p(bits), None, 0, 0, None) == lib.RV_OK
    for args in [((5, 5, 5), p(bits), None, 4, 0, p(out)), ((5, 5, 5), p(bits), p(b), 4, 0, None),
                 ((5, 5, 5), None, p(b), 4, 0, p(out)), ((5, 5, 5), p(bits), p(b), -1, 0, p(out)),
                 ((5, 5, 5), p(bits), p(b), (1 << 24) + 1, 0, p(out)), ((5, 5, 5), p(bits), p(b), 4, 2, p(out)),
                 ((4, 5, 5), p(bits), p(b), 4, 0, p(out)), ((5, 3, 5), p(bits), p(b), 4, 0, p(out))]:
        assert at(*args) == lib.RV_ERR_INVALID, args[3:5]
    # the three entry points that take a context: a NULL context
    assert L.rv_world_bodies_move(None, p(b), 4, 0, p(out)) == lib.RV_ERR_INVALID
    assert L.rv_world_bodies_move_device(None, p(b), 4, 0, p(out)) == lib.RV_ERR_INVALID
    assert L.rv_world_bodies_info(None, None, None) == lib.RV_ERR_INVALID
