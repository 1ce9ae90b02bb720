#!/usr/bin/env python3
"""Latency of moving the world window (rv_world_scroll) next to the only other
way to show terrain beyond the grid's edge: rv_world_build on a context created
at the shifted seed.

Per world and per step (axis, d): the window is moved by +d and back by -d in
turn on one context, and a second context created at the shifted seed rebuilds
its world, the two alternating inside one loop so they see the same machine
state.  Every call is timed with a host clock around the call and a device
synchronise (both calls are synchronous); the first calls warm the code objects
and the scratch allocations and are dropped; the figures are medians with the
range.  The two are not equivalent in the GI grid: a rebuild resets it
(rv_gi_init over every cell), a scroll keeps the retained cells and initialises
the entering ones only.

  tools/scroll_latency.py [--worlds 10,10,10 12,9,12] [--steps 0,8 0,64 2,8 2,64] [--reps 12]
                          [--out profiles/scroll_latency.json]

--tex-follow measures what anchoring the textures to the terrain adds to a scroll
(rv_texture_follow_scroll), on one context that has the tile table, three calls
alternating inside one loop: (a) rv_world_scroll with follow off, (b) the same
scroll with follow on -- the retained table entries moved in place and the
entering ones evaluated -- and (c) rv_texture_origin_set to another origin alone,
the whole-table rebuild that the in-place move exists to beat.  (b) - (a) is the
cost of the table work; the table's bytes and the bytes the move reads and writes
are recorded so that it can be read against the memory bandwidth.

  tools/scroll_latency.py --tex-follow [--worlds 10,10,10] [--out profiles/tex_anchor_latency.json]
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


def measure(rv, lg, steps, reps, warm):
    r = rv.StateRender(lg, 320, 192, tex_table=-1)
    r.world_build()
    out = {"log2_dims": list(lg), "coarse_cells": (1 << sum(lg)) // 8, "steps": []}
    for axis, d in steps:
        step = (d, 0) if axis == 0 else (0, d)
        t = rv.StateRender(lg, 320, 192, tex_table=-1, seed=step)
        t.world_build()
        scroll, build = [], []
        sign = 1
        for i in range(warm + reps):
            ms = timed(r, lambda: r.world_scroll(sign * step[0], sign * step[1]))
            sign = -sign
            ms_b = timed(t, t.world_build)
            if i >= warm:
                scroll.append(ms)
                build.append(ms_b)
        if sign < 0:   # back at the origin for the next step
            r.world_scroll(-step[0], -step[1])
        n, cells, full, origin = r.world_scroll_info()
        assert origin == (0, 0)
        t.close()
        tr, ld, plan_cells, plan_full = rv.scroll_region(lg, axis, d)
        res = {"axis": "xyz"[axis], "d": d, "csdf_cells": plan_cells, "last_full": plan_full,
               "scroll": summary(scroll), "world_build": summary(build)}
        res["ratio"] = round(res["world_build"]["median_ms"] / res["scroll"]["median_ms"], 2)
        print(json.dumps({"log2_dims": list(lg), **res}), flush=True)
        out["steps"].append(res)
    r.close()
    return out


def measure_tex_follow(rv, lg, steps, reps, warm):
    r = rv.StateRender(lg, 320, 192, tex_table=1)
    r.world_build()
    active, table_bytes = r.tex_table_info()
    assert active, "the tile table did not fit"
    dims = [1 << v for v in lg]
    out = {"log2_dims": list(lg), "table_bytes": table_bytes, "table_rows": table_bytes // (4 * dims[0] * dims[2]),
           "steps": []}
    for axis, d in steps:
        step = (d, 0) if axis == 0 else (0, d)
        off, on, rebuild = [], [], []
        sign = 1
        for i in range(warm + reps):
            mv = (sign * step[0], sign * step[1])
            r.texture_follow_scroll(0)
            ms_a = timed(r, lambda: r.world_scroll(*mv))
            r.texture_follow_scroll(1)
            ms_b = timed(r, lambda: r.world_scroll(*mv))
            (ox, oz), _ = r.texture_origin()
            ms_c = timed(r, lambda: r.texture_origin_set(ox + 8 * sign, oz))
            sign = -sign
            if i >= warm:
                off.append(ms_a)
                on.append(ms_b)
                rebuild.append(ms_c)
        if sign < 0:   # back at the origin for the next step
            r.world_scroll(-2 * step[0], -2 * step[1])
        assert r.world_scroll_info()[3] == (0, 0)
        kept = max(0.0, 1.0 - abs(d) / dims[axis])
        res = {"axis": "xyz"[axis], "d": d, "launches_move": -(-(dims[axis] - abs(d)) // abs(d)) if kept else 0,
               "bytes_moved": int(2 * kept * table_bytes), "bytes_evaluated": int((1.0 - kept) * table_bytes),
               "scroll_follow_off": summary(off), "scroll_follow_on": summary(on), "origin_set_rebuild": summary(rebuild)}
        res["table_work_ms"] = round(res["scroll_follow_on"]["median_ms"] - res["scroll_follow_off"]["median_ms"], 3)
        res["rebuild_over_table_work"] = round(res["origin_set_rebuild"]["median_ms"] / max(res["table_work_ms"], 1e-3), 2)
        print(json.dumps({"log2_dims": list(lg), **res}), flush=True)
        out["steps"].append(res)
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", nargs="+", default=["10,10,10", "12,9,12"], help="log2 dims: C4's world, the native world")
    ap.add_argument("--steps", nargs="+", default=["0,8", "0,64", "2,8", "2,64"], help="axis,d pairs (axis 0 = x, 2 = z)")
    ap.add_argument("--reps", type=int, default=12, help="timed calls of each path per step")
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--tex-follow", action="store_true", help="the texture origin following the scroll (see above)")
    ap.add_argument("--out", default=None, help="default profiles/scroll_latency.json (tex_anchor_latency.json with --tex-follow)")
    a = ap.parse_args()
    import rvgrt_amd as rv
    steps = [tuple(int(v) for v in s.split(",")) for s in a.steps]
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tex_anchor_latency.json" if a.tex_follow else "scroll_latency.json")
    if a.tex_follow:
        res = {"what": "ms per call, host clock around a synchronous call + rv_sync, on one context with the tile "
                       "table; alternating in one loop: rv_world_scroll with rv_texture_follow_scroll 0, the same "
                       "scroll with follow 1, rv_texture_origin_set to another origin (whole-table rebuild); "
                       "table_work_ms = follow on - follow off (medians); bytes_moved = read + written by the "
                       "in-place move, bytes_evaluated = entering entries written",
               "worlds": [measure_tex_follow(rv, tuple(int(v) for v in wd.split(",")), steps, a.reps, a.warm)
                          for wd in (a.worlds if a.worlds != ["10,10,10", "12,9,12"] else ["10,10,10"])]}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    res = {"what": "ms per call, host clock around a synchronous call + rv_sync; rv_world_scroll by +d / -d in turn "
                   "against rv_world_build on a second context at the shifted seed, alternating in one loop; "
                   "not equivalent in the GI grid (a rebuild resets it)",
           "worlds": []}
    for wd in a.worlds:
        res["worlds"].append(measure(rv, tuple(int(v) for v in wd.split(",")), steps, a.reps, a.warm))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
