"""The host evaluation of rv_world_edit_shapes (include/rvgrt/rv_shapes.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host_shapes builds a stand-alone program with the sanitizer runtimes linked in
statically -- the test puts nothing into the environment but the two option strings -- that runs the extremes of the arithmetic, the far corner of the bit array and a few
hundred random lists against the definition, every report fatal.  The same program checks what the in-place
voxel writes share (include/rvgrt/rv_words.h): the word grid and the brick columns of a voxel box against a scan
of its voxels, and a component record's box.  A CPU test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "host_shapes")


def test_host_evaluation_under_asan_ubsan():
    env = dict(os.environ)
    b = subprocess.run(["make", "-s", "-C", DIR], capture_output=True, text=True, env=env)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr) and "cannot find" in b.stderr:
        pytest.skip("the toolchain cannot link the sanitizer runtimes: " + b.stderr.strip().splitlines()[-1])
    assert b.returncode == 0, b.stdout + b.stderr
    env.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "build", "host_shapes")], capture_output=True, text=True, env=env, timeout=600)
    out = p.stdout + p.stderr
    assert "runtime error:" not in out and "ERROR: AddressSanitizer" not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
    assert "host_shapes ok" in p.stdout
