#!/usr/bin/env python3
"""Time per call of rv_world_stamp at C4's world (1024^3): 1, 64 and 1024 SET stamps of one 16 x 24 x 16 "tree"
pattern, in all 8 orientations, scattered (seeded) over a 256 x 64 x 256 region around the surface under the bench
pose's column; and rv_pattern_capture of a 64^3 box there.

Timed with the host clock around the synchronous calls, the scene put back by rv_world_import + rv_csdf_build
between repetitions outside the timed region:
  stamp    rv_world_stamp, one call with the whole list;
  route    what the library offered before: the same voxels set as rv_world_edit x-run boxes, in calls of at most
           RV_EDIT_MAX_BOXES boxes, each of which finishes the world separately.  The boxes are made before the
           clock starts; rasterising the trees on the host, which an engine would have to do, is not in the figure;
  capture  rv_pattern_capture of the 64^3 box (both layouts made; the pattern destroyed outside the timed region).
The first calls warm the code object and the context's scratch and are dropped; the figures are medians with
their minimum and maximum.  Before anything is timed the call's counts and the world it leaves are checked
against rv_world_stamp_at, and the route's world against the call's.

  tools/stamp_latency.py [--world 10,10,10] [--counts 1 64 1024] [--reps 5] [--out profiles/stamp_latency.json] [--commit ID]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from detached_latency import median_ms, surface   # noqa: E402
from fall_latency import set_runs, sub_voxels     # noqa: E402


def tree():
    """A 16 x 24 x 16 tree [z, y, x]: a 2 x 2 trunk of 12 rows under a rounded crown."""
    t = np.zeros((16, 24, 16), bool)
    t[7:9, :12, 7:9] = True
    z, y, x = np.meshgrid(np.arange(16), np.arange(24), np.arange(16), indexing="ij")
    t |= (2 * x - 15) ** 2 * 49 + (2 * z - 15) ** 2 * 49 + (2 * y - 33) ** 2 * 64 <= 225 * 49
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (C4's world: 10,10,10)")
    ap.add_argument("--counts", nargs="+", type=int, default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stamp_latency.json"))
    ap.add_argument("--commit", default="", help="the commit to record when the tree is not a git checkout")
    a = ap.parse_args()
    import rvgrt_amd as rv
    from rvgrt_amd.configs import CONFIGS
    lg = tuple(int(v) for v in a.world.split(","))
    X, Y, Z = (1 << l for l in lg)
    r = rv.StateRender(lg, 320, 192, tex_table=-1)
    r.world_build()
    pos = CONFIGS["c4"].pose()[0]
    px, pz = min(int(pos[0]), X - 1), min(int(pos[2]), Z - 1)
    top = surface(r, px, pz, Y)
    # the region: 256 x 64 x 256 voxels around the column, from 20 rows below its surface
    rx0, rz0 = min(max(px - 128, 0), X - 256), min(max(pz - 128, 0), Z - 256)
    ry0 = min(max(top - 20, 0), Y - 64)
    generated = r.world_export(rv.RV_WORLD_BITS)
    commit, dirty = a.commit, None   # the tree the figures were taken on; outside a git checkout: what --commit says
    try:
        g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        if g.returncode == 0:
            commit = g.stdout.strip()
            dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"],
                                        capture_output=True, text=True).stdout.strip())
    except OSError:
        pass
    res = {"what": "median (min - max) ms per repetition after warm-up, host clock, the generated world restored between "
                   "repetitions outside the timed region; stamp: one rv_world_stamp with n SET stamps of a 16 x 24 x 16 tree "
                   "scattered over the region; route: the same voxels as rv_world_edit x-run boxes in calls of at most 1024 "
                   "(boxes made before the clock starts); capture: rv_pattern_capture of a 64^3 box",
           "log2_dims": list(lg), "reps": a.reps, "warm": a.warm, "pose_column": [px, pz], "surface_row": top,
           "region": [rx0, ry0, rz0, rx0 + 256, ry0 + 64, rz0 + 256], "commit": commit, "dirty": dirty, "rows": []}

    def restore():
        r.world_import(rv.RV_WORLD_BITS, generated)
        r.csdf_build()
        r.sync()
    pat = tree()
    pid = r.pattern_create(pat)
    rng = np.random.default_rng(1)
    for n in a.counts:
        stamps = [(0, rv.RV_STAMP_SET, int(rng.integers(0, 8)), (rx0 + int(rng.integers(0, 241)), ry0 + int(rng.integers(0, 41)),
                                                                 rz0 + int(rng.integers(0, 241)))) for _ in range(n)]
        dev = [(pid,) + s[1:] for s in stamps]
        restore()
        # the call against the host form
        want = rv.stamp_at(lg, generated, [pat], stamps)
        got = r.world_stamp(dev)
        box = got[2]
        assert got[:2] == want[1:] and got[0] > 0 and box == rv.stamp_box(lg, [pat], stamps)[1], (n, got, want[1:])
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[0]), (n, "bits")
        full = r.world_edit_info()[2]
        # the route: the x-runs of the voxels the call set
        new, ox = sub_voxels(want[0], lg, box)
        new &= ~sub_voxels(generated, lg, box)[0]
        runs = set_runs(new, (ox, box[1], box[2]))
        edits = [runs[i:i + rv._lib.RV_EDIT_MAX_BOXES] for i in range(0, len(runs), rv._lib.RV_EDIT_MAX_BOXES)]
        restore()
        for e in edits:
            r.world_edit(e)
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[0]), (n, "route")
        restore()
        # the C calls on arrays made once: no allocation inside the timed region
        sarr = rv.render._stamps(dev)
        ebuf = [(np.array(e, np.int32), len(e)) for e in edits]
        n_set, n_cleared, ch = C.c_uint64(), C.c_uint64(), rv._lib.rv_voxel_box()

        def stamp():
            assert r._L.rv_world_stamp(r._h, sarr, n, C.byref(n_set), C.byref(n_cleared), C.byref(ch)) == 0

        def route():
            for arr, k in ebuf:
                assert r._L.rv_world_edit(r._h, arr.ctypes.data_as(C.POINTER(rv._lib.rv_edit_box)), k) == 0
        t_stamp = median_ms(stamp, a.reps, a.warm, restore)
        t_route = median_ms(route, a.reps, a.warm, restore)
        row = {"stamps": n, "box": list(box), "set_voxels": got[0], "whole_grid_csdf": bool(full),
               "route_edit_calls": len(edits), "route_boxes": len(runs), "stamp": t_stamp, "route": t_route}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    # the capture of a 64^3 box of the region
    cbox = (rx0 + 99, ry0, rz0 + 77, rx0 + 163, ry0 + 64, rz0 + 141)   # x0 is no multiple of 8
    made = []
    cap = C.c_int32()
    vb = rv._lib.rv_voxel_box(*cbox)

    def capture():
        assert r._L.rv_pattern_capture(r._h, C.byref(vb), C.byref(cap)) == 0
        made.append(cap.value)

    def drop():
        r.pattern_destroy(made.pop())
    first = r.pattern_capture(cbox)
    assert np.array_equal(r.pattern_read(first), sub_voxels(generated, lg, cbox)[0][:, :, cbox[0] % 32:cbox[0] % 32 + 64]), "capture"
    r.pattern_destroy(first)
    res["capture"] = {"box": list(cbox), **median_ms(capture, 4 * a.reps, a.warm, drop)}
    print(json.dumps(res["capture"]), flush=True)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
