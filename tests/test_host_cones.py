"""The six cones of a land pixel as the frame kernels run them (rv_device.h trace_cones6: the per-normal
first-sample offset table, the interior fast path with its all-opaque case, one cold loop for the cones
that go past step 0) against the reference form, six trace_cone calls summed in order, both compiled for the
CPU (tests/host/rv_host_cones.cpp): bit-equal sums and equal step counts.  Runs without a GPU; the GPU build
of the same source is checked by tests/test_gpu_cone_constants.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LG = (5, 5, 5)
N = 32
ALPHAS = np.array([0, 1, 128, 254, 255], np.uint32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """The harness, compiled here (host pass only, uncontracted) and linked as a plain host library."""
    d = tmp_path_factory.mktemp("host_cones")
    obj, so = str(d / "rv_host_cones.o"), str(d / "librvhostcones.so")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--cuda-host-only",
                    "-x", "hip", "-c", os.path.join(HOST, "rv_host_cones.cpp"), "-o", obj], check=True)
    subprocess.run(["g++", "-shared", "-o", so, obj], check=True)
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int
    L.rvc_table.argtypes = [vp]
    L.rvc_table_generic.argtypes = [vp]
    L.rvc_normal_code.argtypes = [C.c_float] * 3
    L.rvc_normal_code.restype = i32
    L.rvc_cones.argtypes = [i32] * 3 + [vp] * 4 + [C.c_int64, i32, vp, vp]
    L.rvc_cones.restype = i32
    L.rvc_cones_ref.argtypes = [i32] * 3 + [vp] * 4 + [C.c_int64, vp, vp, vp]
    L.rvc_cones_ref.restype = i32
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def scene(oracle):
    """A 32^3 world of random bits with the oracle's CSDF of them, and hits on random voxel faces of all six
    normals plus hits with a zero normal (the undefined hit)."""
    from gpu_world import oracle_of, sparse_bits
    ow = oracle_of(oracle, LG, sparse_bits(LG, 0.004, 99))
    csdf = np.ascontiguousarray(ow.csdf, np.uint8)
    rng = np.random.default_rng(2024)
    n = 24000
    pos = rng.uniform(0.0, N, (n, 3)).astype(np.float32)
    nrm = np.zeros((n, 3), np.float32)
    code = rng.integers(0, 7, n)                       # 6: a zero normal
    for c in range(6):
        m = code == c
        nrm[m, c >> 1] = -1.0 if c & 1 else 1.0
        pos[m, c >> 1] = rng.integers(0, N + 1, m.sum()).astype(np.float32)   # on a voxel face plane
    return csdf, pos, nrm, code


def _gi(seed, opaque):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 1 << 24, (N // 4) ** 3, dtype=np.uint32)
    a = np.full(g.shape, 255, np.uint32) if opaque else ALPHAS[rng.integers(0, 5, g.shape)]
    return np.ascontiguousarray(g | (a << 24), np.uint32)


def _run(L, csdf, gi, pos, nrm, use_tab):
    n = len(pos)
    s, st = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    assert L.rvc_cones(*LG, _p(csdf), _p(gi), _p(pos), _p(nrm), n, use_tab, _p(s), _p(st)) == 0
    return s, st


def _ref(L, csdf, gi, pos, nrm):
    n = len(pos)
    s, st, more = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert L.rvc_cones_ref(*LG, _p(csdf), _p(gi), _p(pos), _p(nrm), n, _p(s), _p(st), _p(more)) == 0
    return s, st, more


def test_offset_table_equals_generic(lib):
    """The host-computed first-sample offsets (constant basis scales, as the kernels read them) equal
    scale(cone_dir(k, up, normalize(cross(up, c)), normalize(cross(up, right))), 3) for all 6 x 6 entries, and
    cone_normal_code finds each normal's row."""
    t, g = np.zeros(108, np.float32), np.zeros(108, np.float32)
    lib.rvc_table(_p(t))
    lib.rvc_table_generic(_p(g))
    assert np.array_equal(t.view(np.uint32), g.view(np.uint32))
    assert np.abs(t).max() <= 3.0          # the fast path's margin: no first sample farther than 3 voxels
    for c in range(6):
        n = [0.0, 0.0, 0.0]
        n[c >> 1] = -1.0 if c & 1 else 1.0
        assert lib.rvc_normal_code(*n) == c


@pytest.mark.parametrize("opaque", [False, True], ids=["mixed_alpha", "opaque"])
def test_cones_equal_reference(lib, scene, opaque):
    csdf, pos, nrm, code = scene
    gi = _gi(7 + opaque, opaque)
    want, wsteps, more = _ref(lib, csdf, gi, pos, nrm)
    # caps on the inputs, from the reference form alone
    margin = np.minimum(pos, N - pos).min(axis=1)
    assert len(pos) >= 20000
    assert (margin < 4).mean() >= 0.25 and (margin >= 4).mean() >= 0.25
    assert all((code == c).sum() >= 1000 for c in range(7))
    if not opaque:
        assert more.sum() >= 0.05 * 6 * len(pos), more.sum()
    for use_tab in (1, 0):
        got, steps = _run(lib, csdf, gi, pos, nrm, use_tab)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), use_tab
        assert np.array_equal(steps, wsteps), use_tab
