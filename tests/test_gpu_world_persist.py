"""rv_world_persist: edited columns survive scrolling away and back.  The dirty
columns that leave the window are gathered on the device and kept in a host
store; a column the library generates again (rv_world_scroll's entering slab,
rv_world_build) takes its stored bits before the exits, the CSDF and the
entering GI cells are derived.  The yardsticks are those of the scroll tests:
the oracle (OracleWorld at an origin, build_csdf, gi_init), the numpy exit
tables of tests/np_exits.py and twin contexts fed through world_import.  Every
comparison is bit-exact."""
import numpy as np
import pytest

from gpu_world import dims, draw, generated, gi, rv, shifted, sparse_bits, step, sun, tables, voxels, world
import np_exits as E
import np_world as R
from np_world import column_bits

pytestmark = pytest.mark.gpu

W, H = 320, 192


def _boxes(bx, bz, variant=0):
    """Edits inside brick column (bx, bz) of a world 128 high: a block set high up, a shaft cleared through
    it down to the ground (variant 1: a different block and shaft)."""
    x, z = 8 * bx, 8 * bz
    if variant == 0:
        return [(x + 1, 90, z + 1, x + 7, 126, z + 7, 1), (x + 2, 0, z + 2, x + 6, 100, z + 6, 0)]
    return [(x, 60, z, x + 8, 80, z + 8, 1), (x + 3, 0, z + 1, x + 5, 128, z + 4, 0)]


def _info(r, *names):
    i = r.world_persist_info()
    return tuple(i[n] for n in names)


def _check_world(rv, oracle, sun, r, lg, want_bits, label):
    """Bits as expected; the CSDF is the oracle's build of them; ytop, column tops, skip table and horizon
    are those of a twin that imports the bits and builds the CSDF, and pass the numpy restatement."""
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, want_bits), (label, "bits")
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = bits
    ow.build_csdf()
    assert np.array_equal(csdf, ow.csdf), (label, "csdf")
    t = rv.StateRender(lg, 64, 64)
    t.world_import(rv.RV_WORLD_BITS, bits)
    t.csdf_build()
    tabs, twin = tables(rv, r), tables(rv, t)
    assert np.array_equal(t.world_export(rv.RV_WORLD_CSDF), csdf), (label, "twin csdf")
    t.close()
    assert tabs[0] == twin[0], (label, "ytop")
    for a, b in zip(tabs[1:], twin[1:]):
        assert np.array_equal(a, b), (label, "tables")
    E.check_tables(E.reference(voxels(bits, lg), sun), *tabs, label)
    return ow


# ---------------------------------------------------------------- 1. the gather kernel
@pytest.mark.parametrize("lg", [(9, 7, 7), (7, 7, 9), (6, 8, 6), (6, 10, 6)])
def test_columns_read(rv, lg):
    X, Y, Z = dims(lg)
    nbx, nbz = X // 8, Z // 8
    r = rv.StateRender(lg, 64, 64, seed=(16, -40))
    with pytest.raises(rv.RvError, match="RV_ERR_STATE"):
        r.world_columns_read([(0, 0)])
    r.world_build()
    rng = np.random.default_rng(7)
    cols = [(0, 0), (nbx - 1, 0), (0, nbz - 1), (nbx - 1, nbz - 1), (nbx - 1, 0)]   # the corners and a repeat
    cols += [(int(rng.integers(nbx)), int(rng.integers(nbz))) for _ in range(70 - len(cols))]
    got = r.world_columns_read(cols)
    assert got.shape == (70, 2 * Y)
    vox = voxels(r.world_export(rv.RV_WORLD_BITS), lg)
    some = False
    for (bx, bz), g in zip(cols, got):
        want = column_bits(vox, bx, bz)
        assert np.array_equal(g, want), (lg, bx, bz)
        some |= bool(want.any()) and not bool((want == 0xFFFFFFFF).all())
    assert some   # neither all empty nor all solid
    assert r.world_columns_read(np.zeros((0, 2), np.int32)).shape == (0, 2 * Y)
    for bad in ((nbx, 0), (0, nbz), (-1, 0), (0, -1)):
        with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
            r.world_columns_read([(0, 0), bad])
    L = rv._lib.load()
    one = np.zeros(2, np.int32)
    out = np.zeros(2 * Y, np.uint32)
    assert L.rv_world_columns_read(r._h, one.ctypes.data, 1, out.ctypes.data, out.nbytes - 4) == rv._lib.RV_ERR_INVALID
    assert _info(r, "on", "dirty_columns", "stored_columns", "captured_total") == (False, 0, 0, 0)
    r.close()


# ---------------------------------------------------------------- 2. away and back, either axis
@pytest.mark.parametrize("lg,axis,d,col", [((9, 7, 7), 0, 16, (1, 5)), ((7, 7, 9), 2, -16, (5, 62))])
def test_away_and_back(rv, oracle, sun, lg, axis, d, col):
    """Without persistence the generated terrain returns in place of the edited column, so the bits
    comparison after the way back fails on a library that lacks it."""
    origin = (16, -40)
    G = tuple(v // 4 for v in dims(lg))
    r = rv.StateRender(lg, 64, 64, seed=origin)
    r.world_persist(True)
    r.world_build()
    assert _info(r, "on", "dirty_columns", "stored_columns") == (True, 0, 0)
    r.world_edit(_boxes(*col))
    bits0 = r.world_export(rv.RV_WORLD_BITS)
    gen = generated(oracle, lg, origin)
    mine, theirs = column_bits(voxels(bits0, lg), *col), column_bits(voxels(gen, lg), *col)
    assert not np.array_equal(mine, theirs)      # the edit changed the column: the test cannot be vacuous
    assert _info(r, "dirty_columns", "stored_columns") == (1, 0)

    r.world_scroll(*step(axis, d))              # the column leaves
    assert _info(r, "dirty_columns", "stored_columns", "stored_bytes", "captured_total", "restored_total") == \
        (0, 1, 8 * dims(lg)[1], 1, 0)
    key = (origin[0] + 8 * col[0], origin[1] + 8 * col[1])
    assert r.world_store_list().tolist() == [list(key)]
    assert np.array_equal(r.world_store_get(*key), mine)
    g0 = gi(rv, r, lg)

    r.world_scroll(*step(axis, -d))             # ... and returns
    assert r.world_scroll_info()[3] == origin and not r.world_scroll_info()[2]
    ow = _check_world(rv, oracle, sun, r, lg, bits0, f"{lg} back")
    assert np.array_equal(r.world_columns_read([col])[0], mine)
    assert _info(r, "dirty_columns", "stored_columns", "captured_total", "restored_total") == (1, 0, 1, 1)
    assert len(r.world_store_list()) == 0
    # the GI grid of the step back (by -d): retained cells moved, entering cells the oracle's gi_init in the
    # final world -- the restored column's among them
    g1 = gi(rv, r, lg)
    g, ax = -d // 4, 2 - axis
    new, old, ent = ([slice(None)] * 3 for _ in range(3))
    new[ax] = slice(0, G[axis] - g) if g > 0 else slice(-g, G[axis])
    old[ax] = slice(g, G[axis]) if g > 0 else slice(0, G[axis] + g)
    ent[ax] = slice(G[axis] - g, G[axis]) if g > 0 else slice(0, -g)
    assert np.array_equal(g1[tuple(new)], g0[tuple(old)])
    ow.gi_init(saturate=False)
    init = ow.gi.view(np.uint32).reshape(G[2], G[1], G[0])
    assert np.array_equal(g1[tuple(ent)], init[tuple(ent)])
    r.close()


# ---------------------------------------------------------------- 3. diagonal
def test_diagonal(rv, oracle, sun):
    lg, origin, col = (7, 7, 7), (-8, 24), (0, 0)
    r = rv.StateRender(lg, 64, 64, seed=origin)
    r.world_persist(True)
    r.world_build()
    r.world_edit(_boxes(*col))
    bits0 = r.world_export(rv.RV_WORLD_BITS)
    assert not np.array_equal(bits0, generated(oracle, lg, origin))
    r.world_scroll(16, 8)
    assert _info(r, "dirty_columns", "stored_columns") == (0, 1)
    assert r.world_store_list().tolist() == [list(origin)]
    r.world_scroll(-16, -8)      # the x step first: the corner column enters with the z step
    _check_world(rv, oracle, sun, r, lg, bits0, "diagonal")
    assert _info(r, "dirty_columns", "stored_columns", "captured_total", "restored_total") == (1, 0, 1, 1)
    r.close()


# ---------------------------------------------------------------- 4. everything leaves
@pytest.mark.parametrize("dx,dz", [(128, 0), (0, -256)])
def test_everything_leaves(rv, oracle, sun, dx, dz):
    lg, origin = (7, 7, 7), (0, 0)
    r = rv.StateRender(lg, 64, 64, seed=origin)
    r.world_persist(True)
    r.world_build()
    r.world_edit(_boxes(1, 5) + _boxes(10, 12, 1))
    bits0 = r.world_export(rv.RV_WORLD_BITS)
    assert _info(r, "dirty_columns", "stored_columns") == (2, 0)
    r.world_scroll(dx, dz)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), generated(oracle, lg, (dx, dz)))
    assert _info(r, "dirty_columns", "stored_columns") == (0, 2)
    r.world_scroll(-dx, -dz)
    _check_world(rv, oracle, sun, r, lg, bits0, "everything leaves")
    assert _info(r, "dirty_columns", "stored_columns", "restored_total") == (2, 0, 2)
    r.close()


@pytest.mark.parametrize("lg", [(6, 10, 6), (7, 4, 7)])
def test_tall_and_flat_columns(rv, oracle, lg):
    """Columns of 128 bricks (the kernels stage 64 at a time: two passes) and of 2 (eight lanes at work)."""
    X, Y, Z = dims(lg)
    r = rv.StateRender(lg, 64, 64, seed=(8, 8))
    r.world_persist(True)
    r.world_build()
    cols = [(0, 0), (X // 8 - 1, Z // 8 - 2), (3, 5)]
    r.world_edit([b for bx, bz in cols for b in
                  ((8 * bx + 1, Y // 2, 8 * bz + 1, 8 * bx + 7, Y - 2, 8 * bz + 7, 1),
                   (8 * bx + 2, 0, 8 * bz + 2, 8 * bx + 6, Y // 2 + 4, 8 * bz + 6, 0))])
    bits0, csdf0 = world(rv, r)
    vox = voxels(bits0, lg)
    read = r.world_columns_read(cols)
    for (bx, bz), got in zip(cols, read):
        assert np.array_equal(got, column_bits(vox, bx, bz)), (lg, bx, bz)
    assert not np.array_equal(bits0, generated(oracle, lg, (8, 8)))
    r.world_scroll(X, -Z)
    assert _info(r, "dirty_columns", "stored_columns") == (0, 3)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), generated(oracle, lg, (8 + X, 8 - Z)))
    r.world_scroll(-X, Z)
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, bits0) and np.array_equal(csdf, csdf0)
    assert _info(r, "dirty_columns", "stored_columns") == (3, 0)
    r.close()


# ---------------------------------------------------------------- 5. an imported world
def test_imported_world(rv, oracle):
    lg = (10, 6, 6)
    X, Y, Z = dims(lg)
    r = rv.StateRender(lg, 64, 64, seed=R.ORIGIN)
    r.world_persist(True)
    imported = sparse_bits(lg, 2e-5, 31)
    r.world_import(rv.RV_WORLD_BITS, imported)
    r.csdf_build()
    assert _info(r, "dirty_columns") == (X // 8 * (Z // 8),)
    bits0, csdf0 = world(rv, r)
    assert np.array_equal(bits0, imported)
    # what the walk leaves without persistence: generated terrain in the left-hand 40 voxels
    gen = voxels(generated(oracle, lg, R.ORIGIN), lg)
    assert not np.array_equal(gen[:, :, :40], voxels(imported, lg)[:, :, :40])
    for _ in range(5):
        r.world_scroll(8, 0)
    assert _info(r, "stored_columns", "captured_total") == (5 * (Z // 8), 5 * (Z // 8))
    r.world_scroll(-40, 0)
    bits, csdf = world(rv, r)
    assert np.array_equal(bits, bits0) and np.array_equal(csdf, csdf0)
    # the five generated slabs that left on the way back were never dirty
    assert _info(r, "dirty_columns", "stored_columns", "restored_total") == (X // 8 * (Z // 8), 0, 5 * (Z // 8))
    r.close()


# ---------------------------------------------------------------- 6. newer wins; a no-op marks nothing
def test_newer_wins_and_noop_marks_nothing(rv, oracle):
    lg, origin, col = (7, 7, 7), (40, -24), (1, 5)
    r = rv.StateRender(lg, 64, 64, seed=origin)
    r.world_persist(True)
    r.world_build()
    r.world_edit(_boxes(*col))
    first = r.world_export(rv.RV_WORLD_BITS)
    r.world_scroll(16, 0)
    r.world_scroll(-16, 0)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), first)
    r.world_edit(_boxes(*col, variant=1))
    second = r.world_export(rv.RV_WORLD_BITS)
    assert not np.array_equal(second, first)
    r.world_scroll(16, 0)
    assert _info(r, "dirty_columns", "stored_columns", "captured_total") == (0, 1, 2)
    r.world_scroll(-16, 0)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), second)
    assert _info(r, "dirty_columns", "stored_columns", "restored_total") == (1, 0, 2)
    # an edit that changes no voxel, in a column that is not dirty: a box that re-writes what is there
    vox = voxels(second, lg)
    box = next(b for b in ((64, 120, 64, 72, 128, 72), (64, 0, 64, 72, 8, 72))
               if vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]].all() or not vox[b[2]:b[5], b[1]:b[4], b[0]:b[3]].any())
    solid = int(vox[box[2]:box[5], box[1]:box[4], box[0]:box[3]].all())
    edits = r.world_edit_info()[0]
    r.world_edit([box + (solid,)])
    assert r.world_edit_info()[0] == edits
    assert _info(r, "dirty_columns") == (1,)
    r.world_edit([box + (1 - solid,)])           # the same box with the other value does mark its column
    assert _info(r, "dirty_columns") == (2,)
    r.close()


# ---------------------------------------------------------------- 7. off is the behaviour without it
@pytest.mark.parametrize("toggle", [False, True])
def test_off_forgets_the_edit(rv, oracle, toggle):
    lg, origin, col = (9, 7, 7), (16, -40), (1, 5)
    zeros = {"on": False, "dirty_columns": 0, "stored_columns": 0, "stored_bytes": 0, "captured_total": 0,
             "restored_total": 0}
    r = rv.StateRender(lg, 64, 64, seed=origin)
    r.world_build()
    if toggle:
        r.world_persist(True)
        r.world_persist(False)
    r.world_edit(_boxes(*col))
    gen = generated(oracle, lg, origin)
    assert not np.array_equal(r.world_export(rv.RV_WORLD_BITS), gen)
    assert r.world_persist_info() == zeros
    r.world_scroll(16, 0)
    r.world_persist_flush()
    assert r.world_persist_info() == zeros
    r.world_scroll(-16, 0)
    assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), gen)
    assert r.world_persist_info() == zeros and len(r.world_store_list()) == 0
    r.close()


# ---------------------------------------------------------------- 8. save and load
def test_save_and_load(rv, oracle, sun):
    lg, origin = (7, 7, 7), (24, -16)
    Y = dims(lg)[1]
    a = rv.StateRender(lg, 64, 64, seed=origin)
    a.world_persist(True)
    a.world_build()
    a.world_edit(_boxes(1, 5))
    a.world_scroll(16, 0)                        # the first column has left
    a.world_edit(_boxes(6, 3, 1) + _boxes(9, 10))
    assert _info(a, "dirty_columns", "stored_columns") == (2, 1)
    a.world_persist_flush()
    assert _info(a, "dirty_columns", "stored_columns", "stored_bytes", "captured_total") == (2, 3, 3 * 8 * Y, 3)
    keys = a.world_store_list()
    want_keys = [(40 + 48, -16 + 24), (24 + 8, -16 + 40), (40 + 72, -16 + 80)]   # sorted by (wz, wx)
    assert keys.tolist() == [list(k) for k in want_keys]
    saved = [a.world_store_get(*k) for k in want_keys]
    assert np.array_equal(saved[0], a.world_columns_read([(6, 3)])[0])
    assert np.array_equal(saved[2], a.world_columns_read([(9, 10)])[0])
    a.world_persist_flush()                      # again: the same three entries
    assert _info(a, "stored_columns", "captured_total") == (3, 5)

    b = rv.StateRender(lg, 64, 64, seed=origin)
    b.world_persist(True)
    for k, bits in zip(want_keys, saved):
        b.world_store_put(*k, bits)
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        b.world_store_get(24, -16)               # not in the store
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        b.world_store_put(24, -16, saved[0][:-1])   # a wrong size
    with pytest.raises(rv.RvError, match="RV_ERR_INVALID"):
        b.world_store_put(25, -16, saved[0])     # no column can have this key
    assert b.world_store_list().tolist() == [list(k) for k in want_keys]
    assert all(np.array_equal(b.world_store_get(*k), s) for k, s in zip(want_keys, saved))
    b.world_build()
    assert _info(b, "dirty_columns", "stored_columns", "captured_total", "restored_total") == (3, 0, 0, 3)

    a.world_scroll(-16, 0)                       # back to the origin
    assert _info(a, "dirty_columns", "stored_columns") == (3, 2)
    bits, csdf = world(rv, a)
    assert not np.array_equal(bits, generated(oracle, lg, origin))
    _check_world(rv, oracle, sun, b, lg, bits, "loaded")
    assert np.array_equal(b.world_export(rv.RV_WORLD_CSDF), csdf)
    ta, tb = tables(rv, a), tables(rv, b)
    assert ta[0] == tb[0] and all(np.array_equal(x, y) for x, y in zip(ta[1:], tb[1:]))
    # rv_world_store_clear empties both
    a.world_store_clear()
    assert _info(a, "dirty_columns", "stored_columns", "stored_bytes") == (0, 0, 0)
    a.close()
    b.close()


# ---------------------------------------------------------------- 9. frames and work computed ahead
def test_frames_across_a_return(rv, oracle, atlas):
    """Flow frames (whose launch computes the next GI update ahead) before and after the scroll that brings
    edited columns back into view.  t: nothing computed ahead, the world handed over through world_import.
    g: the same calls without persistence -- its last frame shows the generated terrain instead."""
    from rvgrt_amd.configs import TEST_POSES_128, camera_path
    lg, (dx, dz) = (7, 7, 7), (16, 16)
    seq = camera_path(TEST_POSES_128["P0"], W, H, 3, pan=0.01, ref_compat=True)
    # the camera (at (110, 70, 120), looking towards low x and z) gets a clear view: the interior above the
    # ground is emptied -- columns the scroll retains -- and walls stand along the two low faces, inside the
    # columns that leave with the scroll and return
    walls = [(16, 34, 16, 128, 128, 128, 0), (2, 0, 0, 14, 128, 128, 1), (0, 0, 2, 128, 128, 14, 1)]
    r, t, g = (rv.StateRender(lg, W, H, flags=rv.RV_FLAGS_REFERENCE, atlas=atlas, gi_rays_per_frame=4096)
               for _ in range(3))
    for c in (r, t, g):
        c.world_build()
        c.gi_update(0)
    t.set_flow(0)
    t.set_gi_async(0)
    r.world_persist(True)
    for c in (r, g):
        c.world_edit(walls)
        c.world_scroll(dx, dz)
    # stored: the columns under x < 16 or z < 16; still dirty: the interior's
    assert _info(r, "dirty_columns", "stored_columns") == (14 * 14, 2 * 16 + 2 * 14)
    away = [shifted(rv, d, dx, dz) for d in seq[:2]]
    for c in (r, t, g):
        for d in away:
            c.update_gi_data()
            draw(c, d)
    assert r.flow_info()[0] and r.flow_info()[1] == 2
    for c in (r, g):
        c.world_scroll(-dx, -dz)
    bits = r.world_export(rv.RV_WORLD_BITS)
    assert not np.array_equal(bits, g.world_export(rv.RV_WORLD_BITS))
    t.world_import(rv.RV_WORLD_BITS, bits)
    t.world_import(rv.RV_WORLD_CSDF, r.world_export(rv.RV_WORLD_CSDF))
    t.world_import(rv.RV_WORLD_GI, r.world_export(rv.RV_WORLD_GI))
    for c in (r, t, g):
        c.update_gi_data()
        draw(c, seq[2])
    for k in (rv.RV_IMAGE_COLOR, rv.RV_IMAGE_MOTION, rv.RV_IMAGE_DEPTH):
        assert np.array_equal(r.readback(k), t.readback(k)), k
    assert np.array_equal(r.world_export(rv.RV_WORLD_GI), t.world_export(rv.RV_WORLD_GI))
    assert r.flow_info()[2] == 0
    # an edited column is in view: without persistence the frame differs
    assert not np.array_equal(r.readback(rv.RV_IMAGE_COLOR), g.readback(rv.RV_IMAGE_COLOR))
    for c in (r, t, g):
        c.close()
