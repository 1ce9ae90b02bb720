#!/usr/bin/env python3
"""What persistence (rv_world_persist) adds to a scroll step.

One context, one world, one step (axis, d); three legs alternate inside one loop
so that they see the same machine state, each one rv_world_scroll by the step
(+d in one round, -d in the next):

  off      persistence off: the scroll as it is without the feature, the baseline;
  idle     persistence on, nothing dirty and an empty store: no launch, copy or
           wait is added, only the host-side look-ups;
  busy     persistence on, every leaving column dirty and every entering column
           in the store: one gather launch and one copy to the host before the
           retained bricks move, one copy to the device and one scatter launch
           after the slab is generated.

The state each leg needs is prepared outside the timed call (rv_world_store_clear;
for busy an edit across the leaving slab and rv_world_store_put of the entering
columns' keys), and the counters of rv_world_persist_info are checked after it.
Every call is timed with a host clock around the call and a device synchronise
(the call is synchronous); the first rounds warm the code objects and the scratch
allocations and are dropped; the figures are medians with the range.

  tools/persist_latency.py [--world 10,10,10] [--step 0,8] [--reps 12] [--warm 2]
                           [--out profiles/persist_latency.json]
"""
import argparse
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


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "calls": len(ms)}


def slabs(dims, axis, d):
    """(leaving, entering) brick columns of a step by d along axis, each in the grid it is named in: the
    leaving ones in the window before the step, the entering ones in the window after it."""
    nb = [dims[0] // 8, dims[2] // 8]
    a, k = (0 if axis == 0 else 1), abs(d) // 8
    lo, hi = range(0, k), range(nb[a] - k, nb[a])
    along = {True: (lo, hi), False: (hi, lo)}[d > 0]
    def cols(rng):
        return [(i, j) if a == 0 else (j, i) for j in range(nb[1 - a]) for i in rng]
    return cols(along[0]), cols(along[1])


def prepare_busy(r, dims, axis, d):
    """Every leaving column dirty (an edit that changes a voxel in each) and every entering column's key in
    the store (any bits: those of the leaving columns)."""
    r.world_store_clear()
    leaving, entering = slabs(dims, axis, d)
    ox, oz = r.world_scroll_info()[3]
    lo = [min(c[0] for c in leaving) * 8, min(c[1] for c in leaving) * 8]
    hi = [max(c[0] for c in leaving) * 8 + 8, max(c[1] for c in leaving) * 8 + 8]
    # the bottom row, under the terrain, so that no column top, exit or sun trace changes with it: cleared, or
    # set again where an earlier round left it cleared
    for solid in (0, 1):
        r.world_edit([(lo[0], 0, lo[1], hi[0], 1, hi[1], solid)])
        if r.world_persist_info()["dirty_columns"] == len(leaving):
            break
    assert r.world_persist_info()["dirty_columns"] == len(leaving)
    bits = r.world_columns_read(leaving)
    nx, nz = ox + (d if axis == 0 else 0), oz + (d if axis == 2 else 0)
    for (bx, bz), b in zip(entering, bits):
        r.world_store_put(nx + 8 * bx, nz + 8 * bz, b)
    return len(leaving)


def measure(rv, lg, axis, d, reps, warm):
    dims = [1 << v for v in lg]
    r = rv.StateRender(lg, 320, 192, tex_table=-1)
    r.world_build()
    step = (d, 0) if axis == 0 else (0, d)
    legs = {"off": [], "idle": [], "busy": []}
    sign, ncols = 1, 0
    for i in range(warm + reps):
        mv = (sign * step[0], sign * step[1])
        r.world_persist(False)
        r.world_store_clear()
        ms = {"off": timed(r, lambda: r.world_scroll(*mv))}
        r.world_persist(True)
        before = r.world_persist_info()
        ms["idle"] = timed(r, lambda: r.world_scroll(*mv))
        assert r.world_persist_info() == before and before["dirty_columns"] == before["stored_columns"] == 0
        ncols = prepare_busy(r, dims, axis, sign * d)
        before = r.world_persist_info()
        ms["busy"] = timed(r, lambda: r.world_scroll(*mv))
        after = r.world_persist_info()
        assert after["captured_total"] - before["captured_total"] == ncols
        assert after["restored_total"] - before["restored_total"] == ncols
        sign = -sign
        if i >= warm:
            for k, v in ms.items():
                legs[k].append(v)
    r.close()
    res = {"log2_dims": list(lg), "axis": "xyz"[axis], "d": d, "columns": ncols, "column_bytes": 8 * dims[1],
           "staged_bytes_each_way": ncols * 8 * dims[1],
           "off": summary(legs["off"]), "idle": summary(legs["idle"]), "busy": summary(legs["busy"])}
    res["idle_minus_off_ms"] = round(res["idle"]["median_ms"] - res["off"]["median_ms"], 3)
    res["busy_minus_off_ms"] = round(res["busy"]["median_ms"] - res["off"]["median_ms"], 3)
    res["idle_median_within_off_range"] = res["off"]["min_ms"] <= res["idle"]["median_ms"] <= res["off"]["max_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (default: C4's world)")
    ap.add_argument("--step", default="0,8", help="axis,d (axis 0 = x, 2 = z)")
    ap.add_argument("--reps", type=int, default=12, help="timed calls of each leg")
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "persist_latency.json"))
    a = ap.parse_args()
    import rvgrt_amd as rv
    axis, d = (int(v) for v in a.step.split(","))
    res = {"what": "ms per rv_world_scroll call, host clock around the synchronous call + rv_sync, one context, "
                   "three legs alternating in one loop: persistence off; on with nothing dirty and an empty store; "
                   "on with every leaving column dirty and every entering column restored from the store",
           **measure(rv, tuple(int(v) for v in a.world.split(",")), axis, d, a.reps, a.warm)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
