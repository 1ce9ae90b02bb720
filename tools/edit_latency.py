#!/usr/bin/env python3
"""Latency of one block edit (rv_world_edit) next to the only other way to
change a voxel through the C ABI: rv_world_import(RV_WORLD_BITS) of the
patched bits + rv_csdf_build() on the same context.

Per world: the centre voxel is set and cleared in turn.  Every call is timed
with a host clock around the call and a device synchronise (both paths are
synchronous: they end in a stream synchronise); the first calls warm the
code objects and the scratch allocations and are dropped; the figures are
medians.  The two paths alternate inside one loop, so they see the same
machine state.  The import path is given the already patched host bits: its
figure leaves out the export and the host patch a caller would also pay.

  tools/edit_latency.py [--worlds 10,10,10 12,9,12] [--reps 20] [--out profiles/edit_latency.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(r, fn):
    r.sync()
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def measure(rv, lg, reps, warm, import_reps):
    X, Y, Z = (1 << l for l in lg)
    r = rv.StateRender(lg, 320, 192, tex_table=-1)
    t0 = time.perf_counter()
    r.world_build()
    r.sync()
    build_s = time.perf_counter() - t0
    x, y, z = X // 2, Y // 2, Z // 2
    box = (x, y, z, x + 1, y + 1, z + 1)
    idx = x | (y << lg[0]) | (z << (lg[0] + lg[1]))
    word, bit = idx >> 5, np.uint32(1 << (idx & 31))
    host = r.world_export(rv.RV_WORLD_BITS)
    state = int(bool(host[word] & bit))
    local = {0: [], 1: []}
    full = {0: [], 1: []}
    cells = None
    every = max(1, reps // import_reps)
    for i in range(warm + reps):
        state ^= 1
        ms = timed(r, lambda: r.world_edit([box + (state,)]))
        edits, n, was_full = r.world_edit_info()
        assert n > 0, "the edit changed nothing"
        cells = (n, was_full)
        if i >= warm:
            local[state].append(ms)
        if i < min(warm, 2) or (i >= warm and (i - warm) % every == 0):
            state ^= 1
            host[word] = (host[word] | bit) if state else (host[word] & ~bit)

            def imp():
                r.world_import(rv.RV_WORLD_BITS, host)
                r.csdf_build()
            ms = timed(r, imp)
            if i >= warm:
                full[state].append(ms)
        host[word] = (host[word] | bit) if state else (host[word] & ~bit)
    r.close()
    med = statistics.median
    out = {"log2_dims": list(lg), "coarse_cells": X * Y * Z // 8, "world_build_s": round(build_s, 3),
           "csdf_cells": cells[0], "last_full": bool(cells[1]),
           "edit_set_ms": round(med(local[1]), 4), "edit_clear_ms": round(med(local[0]), 4),
           "edit_min_ms": round(min(local[0] + local[1]), 4), "edit_max_ms": round(max(local[0] + local[1]), 4),
           "edit_calls": len(local[0]) + len(local[1]),
           "import_build_set_ms": round(med(full[1]), 3) if full[1] else None,
           "import_build_clear_ms": round(med(full[0]), 3) if full[0] else None,
           "import_build_calls": len(full[0]) + len(full[1])}
    both = full[0] + full[1]
    out["import_build_ms"] = round(med(both), 3)
    out["ratio"] = round(med(both) / med(local[0] + local[1]), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", nargs="+", default=["10,10,10"], help="log2 dims, e.g. 10,10,10 12,9,12")
    ap.add_argument("--reps", type=int, default=20, help="timed edits per world (half set, half clear)")
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--import-reps", type=int, default=10, help="timed import + build calls per world")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_latency.json"))
    a = ap.parse_args()
    import rvgrt_amd as rv
    res = {"what": "median ms per call, host clock around a synchronous call; centre voxel set / cleared in turn",
           "worlds": []}
    for wd in a.worlds:
        lg = tuple(int(v) for v in wd.split(","))
        m = measure(rv, lg, a.reps, a.warm, a.import_reps)
        print(json.dumps(m), flush=True)
        res["worlds"].append(m)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
