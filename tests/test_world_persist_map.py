"""rv_world_persist on a machine without a GPU: rv_persist_column_map -- the index
arithmetic both persistence kernels run, evaluated on the host by the function
they call -- against a numpy restatement of the brick layout of
include/rvgrt/rv_device.h, and the status codes of the new entry points."""
import ctypes as C

import numpy as np
import pytest

from gpu_world import rv
from np_world import column_bits

WORLDS = [(7, 6, 7), (9, 7, 7), (7, 7, 9), (6, 8, 6)]   # lbx != lbz both ways; ly below and above lx


def brick_array(vox):
    """The bit records of voxels [z, y, x] as rv_device.h lays them out: brick b = bz | by << lbz | bx << lbzy,
    16 dwords per brick, bit (x & 7) | (y & 7) << 3 | (z & 7) << 6 of the brick's 512."""
    Z, Y, X = vox.shape
    v = vox.reshape(Z // 8, 8, Y // 8, 8, X // 8, 8)       # bz, z, by, y, bx, x
    v = v.transpose(4, 2, 0, 1, 3, 5)                       # bx, by, bz | z, y, x: bz fastest of the bricks
    return np.packbits(v.reshape(-1), bitorder="little").view(np.uint32)


def columns_of(lg):
    nbx, nbz = (1 << lg[0]) // 8, (1 << lg[2]) // 8
    return [(0, 0), (nbx - 1, 0), (0, nbz - 1), (nbx - 1, nbz - 1), (nbx // 2 + 1, nbz // 3)]


@pytest.mark.parametrize("lg", WORLDS)
def test_column_map_matches_numpy(rv, lg):
    X, Y, Z = (1 << l for l in lg)
    vox = np.random.default_rng(sum(lg)).random((Z, Y, X)) < 0.5
    bricks = brick_array(vox)
    assert bricks.size == X * Y * Z // 32
    maps = []
    for bx, bz in columns_of(lg):
        m = rv.persist_column_map(lg, bx, bz)
        assert m.shape == (2 * Y,) and m.dtype == np.uint32
        assert int(m.max()) < bricks.size
        assert np.array_equal(bricks[m], column_bits(vox, bx, bz)), (lg, bx, bz)
        assert len(np.unique(m)) == m.size, "the map of one column is injective"
        maps.append(m)
    every = np.concatenate(maps)
    assert len(np.unique(every)) == every.size, "the maps of two columns are disjoint"


@pytest.mark.parametrize("lg", WORLDS)
def test_column_map_is_the_documented_formula(rv, lg):
    """Word (y >> 2) | z << (ly - 2) is dword ((y >> 2) & 1) | (z & 7) << 1 of brick (bx, y >> 3, bz)."""
    lbz, lby = lg[2] - 3, lg[1] - 3
    for bx, bz in columns_of(lg):
        i = np.arange(2 << lg[1], dtype=np.int64)
        yq, z = i & ((1 << (lg[1] - 2)) - 1), i >> (lg[1] - 2)
        brick = bz | ((yq >> 1) << lbz) | (bx << (lbz + lby))
        want = brick * 16 + ((yq & 1) | (z << 1))
        assert np.array_equal(rv.persist_column_map(lg, bx, bz).astype(np.int64), want)


def test_column_map_rejects_bad_arguments(rv):
    L = rv._lib.load()
    INV = rv._lib.RV_ERR_INVALID
    out = np.zeros(2 << 7, np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    assert L.rv_persist_column_map(9, 7, 7, 63, 15, p) == 0
    assert L.rv_persist_column_map(9, 7, 7, 64, 0, p) == INV       # bx outside the world
    assert L.rv_persist_column_map(9, 7, 7, 0, 16, p) == INV       # bz outside the world
    assert L.rv_persist_column_map(9, 7, 7, -1, 0, p) == INV
    assert L.rv_persist_column_map(3, 7, 7, 0, 0, p) == INV        # rv_create's limits on the dims
    assert L.rv_persist_column_map(9, 7, 7, 0, 0, None) == INV


def test_null_context_status_codes(rv):
    L = rv._lib.load()
    INV = rv._lib.RV_ERR_INVALID
    buf = np.zeros(256, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_int64()
    assert L.rv_world_persist(None, 1) == INV
    assert L.rv_world_persist_info(None, None, None, None, None, None, None) == INV
    assert L.rv_world_persist_flush(None) == INV
    assert L.rv_world_store_list(None, None, 0, C.byref(n)) == INV
    assert L.rv_world_store_get(None, 0, 0, p, 1024) == INV
    assert L.rv_world_store_put(None, 0, 0, p, 1024) == INV
    assert L.rv_world_store_clear(None) == INV
    assert L.rv_world_columns_read(None, p, 1, p, 1024) == INV


def test_new_entry_points_are_declared_and_bound(rv):
    import re
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rvgrt.h")).read()
    declared = set(re.findall(r"^\s*rv_status\s+(rv_\w+)\s*\(", hdr, re.M))
    new = {"rv_world_persist", "rv_world_persist_info", "rv_world_persist_flush", "rv_world_store_list",
           "rv_world_store_get", "rv_world_store_put", "rv_world_store_clear", "rv_world_columns_read",
           "rv_persist_column_map"}
    assert new <= declared
    assert new <= {name for name, _, _ in rv._lib.SIGNATURES}
    L = rv._lib.load()
    assert all(hasattr(L, name) for name in new)
    assert L.rv_abi_version() == 2   # no struct changed
