"""The host evaluation of rv_world_stamp (include/rvgrt/rv_stamp.h) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/host_stamp builds a stand-alone program with the sanitizer runtimes linked in
statically -- the test puts nothing into the environment but the two option strings -- that runs every
orientation and op over pattern rows of every interesting width at every offset, the far corners of the world
and of the patterns, the extreme offsets and a few hundred random lists against the definition written out
naively, every report fatal.  The world and the patterns' layouts are heap blocks of exactly their size.  A CPU
test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "host_stamp")


def test_host_evaluation_under_asan_ubsan(tmp_path):
    env = dict(os.environ)
    # asked of the toolchain beforehand: can it link an empty program with the static sanitizer runtimes at all
    cxx = env.get("CXX", "g++")
    probe = subprocess.run([cxx, "-x", "c++", "-", "-o", str(tmp_path / "probe"), "-fsanitize=address,undefined", "-static-libasan",
                            "-static-libubsan"], input="int main() { return 0; }\n", capture_output=True, text=True, env=env)
    if probe.returncode != 0:
        pytest.skip("the toolchain cannot link the sanitizer runtimes: " + (probe.stderr.strip().splitlines() or ["?"])[-1])
    b = subprocess.run(["make", "-s", "-C", DIR], capture_output=True, text=True, env=env)
    assert b.returncode == 0, b.stdout + b.stderr
    env.update(ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "build", "host_stamp")], capture_output=True, text=True, env=env, timeout=600)
    out = p.stdout + p.stderr
    assert "runtime error:" not in out and "ERROR: AddressSanitizer" not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
    assert "host_stamp ok" in p.stdout
