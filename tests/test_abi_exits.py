"""The exits' diagnostic entry points on a machine without a GPU (tests/test_abi.py checks every
declared entry point from the header; this file names the test hooks of tests/test_gpu_exits.py and
their constants): declared in include/rvgrt.h, exported by the library, bound in Python with the header's
values, and refusing null arguments before any device work."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exit_test_hooks_are_declared_exported_and_bound():
    from rvgrt_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "rvgrt.h")).read()
    declared = re.findall(r"^\s*rv_status\s+(rv_\w+)\s*\(", hdr, re.M)
    for n in ("rv_trace_rays_variant", "rv_world_top_info"):
        assert n in declared and hasattr(L, n) and n in {s[0] for s in _lib.SIGNATURES}, n
    for n in ("RV_WORLD_COLTOP", "RV_WORLD_HORIZON", "RV_WORLD_DTOP", "RV_TRACE_SKY", "RV_TRACE_SUN", "RV_TRACE_COL"):
        m = re.search(rf"\b{n}\s*=\s*(0x[0-9A-Fa-f]+|\d+)", hdr)
        assert m and int(m.group(1), 0) == getattr(_lib, n), n
    assert L.rv_trace_rays_variant(None, 4, None, None, None, 0, None) == _lib.RV_ERR_INVALID
    assert L.rv_world_top_info(None, None) == _lib.RV_ERR_INVALID
