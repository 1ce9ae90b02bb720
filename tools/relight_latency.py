#!/usr/bin/env python3
"""Latency of a GI relight (rv_gi_relight) of the cells around a one-block edit
next to what the library offered for refreshing them at once before it: K calls
of rv_gi_update(frame, first, count) over the single linear span from the box's
first cell to its last.  The span is NOT equivalent -- it also updates every
unrelated cell in between (about 58x the box's cells for a 33^3 box in a 256^3
grid) -- but a box is otherwise one call per x-row.

The centre block is set (rv_world_edit), a slab of whole planes is relit one
step and compared with rv_gi_update over the same range (results at the
timed size), then the box is
relight_box(edit, margin) and both paths run K steps, alternating inside one
loop so they see the same machine state.  Every figure is a host clock around
the call(s) plus rv_sync; the first rounds warm the code objects and the scratch
allocations and are dropped; the figures are medians.

  tools/relight_latency.py [--world 10,10,10] [--margin 16] [--steps 1 16 64] [--reps 12]
                           [--out profiles/relight_latency.json]
  --only relight           run the relight alone (for a kernel-trace run of its own)
  --kernel-stats CSV       merge a profiler's kernel statistics (columns Name, Calls, AverageNs, MinNs, MaxNs) of such a
                           run into the output file: mean us per launch of the relight's kernels
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(r, fn):
    r.sync()
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def measure(rv, lg, margin, steps, reps, warm, only):
    from rvgrt_amd.atlas import load_atlas
    X, Y, Z = (1 << l for l in lg)
    GX, GY, GZ = X // 4, Y // 4, Z // 4
    r = rv.StateRender(lg, 320, 192, atlas=load_atlas())
    r.world_build()
    x, y, z = X // 2, Y // 2, Z // 2
    edit = [(x, y, z, x + 1, y + 1, z + 1, 1)]
    r.world_edit(edit)
    box = rv.relight_box(lg, edit, margin)
    cells = (box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2])
    first = box[0] + GX * (box[1] + GY * box[2])
    last = (box[3] - 1) + GX * ((box[4] - 1) + GY * (box[5] - 1))
    span = last - first + 1
    out = {"log2_dims": list(lg), "gi_cells": GX * GY * GZ, "margin_cells": margin, "box": list(box),
           "box_cells": cells, "span_cells": span, "span_over_box": round(span / cells, 1), "steps": []}
    # results at the timed size: a slab of whole planes, one step, equals rv_gi_update over the planes' range
    z0 = box[2]
    g0 = r.world_export(rv.RV_WORLD_GI)
    r.gi_relight((0, 0, z0, GX, GY, z0 + 2), 7, 1)
    a = r.world_export(rv.RV_WORLD_GI)
    r.world_import(rv.RV_WORLD_GI, g0)
    r.gi_update(7, z0 * GX * GY, 2 * GX * GY)
    assert (a == r.world_export(rv.RV_WORLD_GI)).all() and (a != g0).any(), "relight differs from rv_gi_update"
    r.world_import(rv.RV_WORLD_GI, g0)
    out["slab_check"] = "2 planes (%d cells), 1 step == rv_gi_update over their range" % (2 * GX * GY)
    t0 = r.stats()["gi_traces"]
    r.gi_relight(box, 999, 1)
    out["traced_cells"] = (r.stats()["gi_traces"] - t0) // 2   # box cells whose centre voxel is not solid
    frame = 1000
    for K in steps:
        relight, base = [], []
        for i in range(warm + reps):
            ms = timed(r, lambda: r.gi_relight(box, frame, K))
            if i >= warm:
                relight.append(ms)
            if only != "relight":
                def spans():
                    for s in range(K):
                        r.gi_update(frame + s, first, span)
                ms = timed(r, spans)
                if i >= warm:
                    base.append(ms)
            frame += K
        med = statistics.median
        row = {"K": K, "records": cells * K, "relight_ms": round(med(relight), 4), "relight_min_ms": round(min(relight), 4),
               "relight_max_ms": round(max(relight), 4), "calls": len(relight)}
        if base:
            row.update({"span_updates_ms": round(med(base), 4), "span_updates_min_ms": round(min(base), 4),
                        "span_updates_max_ms": round(max(base), 4), "ratio": round(med(base) / med(relight), 1)})
        print(json.dumps(row), flush=True)
        out["steps"].append(row)
    assert r.gi_relight_info()[0] == 2 + len(steps) * (warm + reps)
    r.close()
    return out


def kernel_stats(path):
    """Mean us per launch of the GI kernels in a profiler's kernel statistics."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].split("(")[0]
            if "relight" in name or "k_gi_update" in name:
                short = name.split("::")[-1]
                out[short] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims")
    ap.add_argument("--margin", type=int, default=16, help="GI cells around the edit")
    ap.add_argument("--steps", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", choices=["relight"], default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relight_latency.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            res = json.load(f)
        res["kernel_us"] = {"source": "kernel trace of a run of its own (--only relight --steps 64: one 1-step call, "
                                      "then K = 64 calls), us per launch", **kernel_stats(a.kernel_stats)}
    else:
        import rvgrt_amd as rv
        lg = tuple(int(v) for v in a.world.split(","))
        res = {"what": "median ms, host clock around the call(s) + rv_sync; relight of the box around a one-block edit "
                       "at the world centre vs K rv_gi_update calls over the box's linear span (not equivalent: the "
                       "span also updates the unrelated cells in between)"}
        res.update(measure(rv, lg, a.margin, a.steps, a.reps, a.warm, a.only))
        if a.only:
            return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
