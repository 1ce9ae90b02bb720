"""The numpy references of the exit tables (tests/np_exits.py) proved on the CPU, before
tests/test_gpu_exits.py holds the GPU's tables to them: on every world that file uses, the
tables the host harness builds (tests/host/rv_host_trace.cpp, compiled with the tables' entry
point by tests/host_exits: the functions the four table
kernels call -- brick_top_y, brick_subcolumn_tops, the 3x3 clip, horizon_column -- driven by
host loops) equal the integer references, and their horizon satisfies the safety bound, the
tightness bound and the float32 restatement.  Also here: the references reject tables that
are too eager or too timid, and the ray sets of the GPU file meet its conditions (hit share,
the skip firing, both branches of the row bound) on its worlds.  Runs without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_world import sun
import np_exits as E

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host_exits")   # tests/host's harness plus rvh_exit_tables
HIT = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("hit", "<i4"),
                ("undef", "<i4"), ("sphere", "<i4"), ("dda", "<i4"), ("check", "<i4"), ("pad", "<i4")])


@pytest.fixture(scope="module")
def host_lib():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    L = C.CDLL(os.path.join(HOST, "build", "librvhost_exits.so"))
    V = C.c_void_p
    L.rvh_exit_tables.restype = C.c_int
    L.rvh_exit_tables.argtypes = [C.c_int] * 3 + [V] * 6
    L.rvh_trace_sun.restype = C.c_int
    L.rvh_trace_sun.argtypes = [C.c_int] * 4 + [V] * 5 + [C.c_int64, V, V]
    L.rvh_trace_col.restype = C.c_int
    L.rvh_trace_col.argtypes = [C.c_int] * 5 + [V] * 5 + [C.c_int64, V]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_tables(L, lg, vox, sun):
    X, Z = 1 << lg[0], 1 << lg[2]
    bits = E.bits_of(vox)
    yt = C.c_uint32()
    ct, hz = np.zeros((Z // 2, X // 2), np.uint32), np.zeros((Z // 2, X // 2), np.uint32)
    dt = np.zeros((Z // 8, X // 8), np.int32)
    assert L.rvh_exit_tables(*lg, _p(bits), _p(sun), C.byref(yt), _p(ct), _p(hz), _p(dt)) == 0
    return int(yt.value), ct, hz, dt


@pytest.mark.parametrize("name", list(E.WORLDS))
def test_references_hold_on_the_host_tables(host_lib, oracle, sun, name):
    lg, make = E.WORLDS[name]
    vox = make(oracle)
    assert vox.shape == (1 << lg[2], 1 << lg[1], 1 << lg[0])
    yt, ct, hz, dt = _host_tables(host_lib, lg, vox, sun)
    slack = E.check_tables(E.reference(vox, sun, name), yt, ct, hz, dt, name)
    print(f"{name} {vox.shape[::-1]}: ytop {yt}, {ct.size} coltop / horizon cells, {dt.size} dtop cells; "
          f"horizon - safety {slack[0]}, tightness - horizon {slack[1]}")
    if name == "empty":
        assert yt == 1 and not ct.any() and not hz.any() and not dt.any()
    if name == "full":
        assert yt == vox.shape[1] and (ct == vox.shape[1]).all()
    if name.startswith("terrain") and name != "terrain16":
        assert hz.min() < hz.max() and ct.min() < ct.max()   # the tables vary over the terrain


def test_references_hold_after_each_edit(host_lib, oracle, sun):
    """The edits tests/test_gpu_exits.py applies through rv_world_edit, one after the other, and the pillar
    it raises into the skimming rays' path: every table of the edited voxels against the references, and each
    edit moves the table it is meant to move."""
    lg, make = E.EDIT_WORLD
    vox = make(oracle)
    before = _host_tables(host_lib, lg, vox, sun)
    E.check_tables(E.reference(vox, sun, "edit0"), *before, "edit world")
    moved = []
    for n, (what, boxes) in enumerate(E.edit_steps(vox), 1):
        vox = E.apply_boxes(vox, boxes)
        after = _host_tables(host_lib, lg, vox, sun)
        slack = E.check_tables(E.reference(vox, sun, f"edit{n}"), *after, what)
        moved.append([bool(np.any(a != b)) for a, b in zip(before, after)])
        print(f"{what} {boxes}: ytop/coltop/horizon/dtop moved {moved[-1]}; slack {slack}")
        before = after
    assert moved[0] == [True] * 4 and moved[1][1:3] == [True] * 2 and moved[2][1:] == [True] * 3
    vox = E.apply_boxes(make(oracle), E.pillar_boxes(make(oracle)))
    E.check_tables(E.reference(vox, sun, "pillar"), *_host_tables(host_lib, lg, vox, sun), "pillar")


def test_references_reject_wrong_tables(oracle, sun):
    """Each statement bites on its own: a horizon one row too low behind the highest column fails the
    safety bound (too eager), one left at its "off" fill or raised by two rows fails the tightness bound (too
    timid), a one-row error anywhere fails the float32 restatement; the integer tables are compared exactly."""
    lg, make = E.WORLDS["terrain_6_7_5"]
    vox = make(oracle)
    ref = E.reference(vox, sun, "terrain_6_7_5")
    good = (ref["ytop"], ref["coltop"], ref["f32"], ref["dtop"])
    E.check_tables(ref, *good)
    lo = ref["safety"]
    c = np.unravel_index(np.argmax(lo), lo.shape)
    eager = ref["f32"].copy()
    eager[c] = np.uint32(np.ceil(lo[c]) - 1)                 # below the column's own top
    off = np.full_like(ref["f32"], E.HORIZON_OFF)
    timid = ref["f32"] + np.uint32(2)
    one = ref["f32"].copy()
    one[0, 0] += 1
    for hz, word in ((eager, "eager"), (off, "timid"), (timid, "timid"), (one, None)):
        with pytest.raises(AssertionError, match=word):
            E.check_tables(ref, good[0], good[1], hz, good[3])
    ct = ref["coltop"].copy()
    ct[-1, -1] += 1
    dt = ref["dtop"].copy()
    dt[0, -1] -= 1
    for bad in ((good[0] + 1, good[1], good[2], good[3]), (good[0], ct, good[2], good[3]),
                (good[0], good[1], good[2], dt), (good[0], good[1], good[2], np.full_like(dt, E.DTOP_OFF))):
        with pytest.raises(AssertionError):
            E.check_tables(ref, *bad)


def _oracle_world(oracle, lg, vox):
    ow = oracle.OracleWorld(*lg)
    ow.bits[:] = E.bits_of(vox)
    ow.build_csdf()
    return ow


RAY_WORLDS = {"terrain128_cut90": E.WORLDS["terrain128_cut90"], "terrain_8_6_7_cut56": E.EDIT_WORLD}


@pytest.mark.parametrize("name", list(RAY_WORLDS))
def test_ray_sets_meet_their_conditions(host_lib, oracle, sun, name):
    """The sun and column-skip rays of tests/test_gpu_exits.py on its two ray worlds, through the host build
    of the same traversals: shadowed and lit points both (hit share 0.1 .. 0.9), the skip firing on more
    than 5 % of the groups and on both branches of the iy - G row bound, the hits the oracle's."""
    lg, make = RAY_WORLDS[name]
    vox = make(oracle)
    ow = _oracle_world(oracle, lg, vox)
    org, dirs, dist = E.sun_rays(ow, sun)
    assert len(org) % 64 != 0
    g = np.zeros(len(org), HIT)
    hz = np.zeros((ow.Z // 2) * (ow.X // 2), np.uint32)
    assert host_lib.rvh_trace_sun(0, *lg, _p(ow.bits), _p(ow.csdf), _p(sun), _p(org), _p(dist), len(org), _p(g),
                                  _p(hz)) == 0
    o = ow.trace_batch(org, dirs, dist)
    assert np.array_equal(g["hit"], o["hit"]) and np.array_equal(g["pos"].view(np.uint32), o["pos"].view(np.uint32))
    assert 0.1 < o["hit"].mean() < 0.9
    assert (g["sphere"] <= o["n_sphere"]).all() and g["sphere"].sum() < 0.8 * o["n_sphere"].sum()
    org, d, dist, _ = E.column_rays(vox)
    o = ow.trace_batch(org, d, dist)
    for g8 in (0, 1):
        a = np.zeros(len(org), HIT)
        assert host_lib.rvh_trace_col(g8, 1, *lg, _p(ow.bits), _p(ow.csdf), _p(org), _p(d), _p(dist), len(org),
                                      _p(a)) == 0
        assert np.array_equal(a["hit"], o["hit"]) and np.array_equal(a["pos"].view(np.uint32), o["pos"].view(np.uint32))
        groups = E.groups_walked(a["dda"], 8 if g8 else 4)
        assert a["pad"].sum() > 0.05 * groups.sum(), (a["pad"].sum(), groups.sum())
        desc = d[:, 1] < 0
        assert a["pad"][desc].sum() > 0 and a["pad"][~desc].sum() > 0
    print(f"{name}: {len(dirs)} sun rays, hit share {o['hit'].mean():.2f} (column rays); skip share "
          f"{a['pad'].sum() / groups.sum():.2f} of the groups at look-ahead 8")


def test_the_pillar_stands_in_the_skimming_rays_path(oracle, sun):
    """The pillar test_gpu_exits.py raises changes what some of the column-skip rays and some of the sun
    rays hit (oracle against oracle): a stale dtop or horizon after that edit would show in those rays."""
    lg, make = E.EDIT_WORLD
    vox = make(oracle)
    ow0 = _oracle_world(oracle, lg, vox)
    ow1 = _oracle_world(oracle, lg, E.apply_boxes(vox, E.pillar_boxes(vox)))
    org, d, dist, _ = E.column_rays(vox)
    a, b = ow0.trace_batch(org, d, dist), ow1.trace_batch(org, d, dist)
    changed = int((a["pos"].view(np.uint32) != b["pos"].view(np.uint32)).any(axis=1).sum())
    org, dirs, dist = E.sun_rays(ow0, sun)
    a, b = ow0.trace_batch(org, dirs, dist), ow1.trace_batch(org, dirs, dist)
    shadowed = int((a["hit"] != b["hit"]).sum())
    print(f"pillar: {changed} column rays and {shadowed} sun rays change their result")
    assert changed >= 10 and shadowed >= 10


def test_max_over_columns_equals_the_column_by_column_loop():
    """np_exits._max_over_columns walks the valid offsets; the plain statement walks the columns."""
    rng = np.random.default_rng(3)
    for ncz, ncx in ((5, 9), (16, 4), (1, 7), (12, 12)):
        ct = rng.integers(0, 40, (ncz, ncx)).astype(np.uint32)
        ct[rng.uniform(size=ct.shape) < 0.3] = 0                       # empty columns
        for density in (0.0, 0.05, 0.5, 1.0):
            valid = rng.uniform(size=(2 * ncz - 1, 2 * ncx - 1)) < density
            cost = rng.normal(0, 20, valid.shape)
            cost[~valid & (rng.uniform(size=valid.shape) < 0.5)] = np.inf   # as the safety bound leaves them
            base = np.where(ct > 0, ct.astype(np.float64), -np.inf)
            pen = np.where(valid, cost, np.inf)
            want = np.full((ncz, ncx), -np.inf)
            for cz in range(ncz):
                for cx in range(ncx):
                    want[cz, cx] = (base - pen[ncz - 1 - cz:2 * ncz - 1 - cz, ncx - 1 - cx:2 * ncx - 1 - cx]).max()
            assert np.array_equal(E._max_over_columns(ct, cost, valid), want), (ncz, ncx, density)
