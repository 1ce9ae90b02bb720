#!/usr/bin/env python3
"""Time per call of rv_world_edit_shapes at C4's world (1024^3): a voxel-centred sphere of radius 4, 16, 32 and
64 voxels cleared out of the generated terrain, centred on the surface under the bench pose's column.

Timed with the host clock around the synchronous calls, the scene put back by rv_world_import + rv_csdf_build
between repetitions outside the timed region:
  shapes   rv_world_edit_shapes, one call with the one sphere;
  route    what the call replaces: the same voxels cleared as rv_world_edit x-run boxes, in calls of at most
           1024 boxes.  The boxes are made before the clock starts; rasterising the sphere on the host, which
           an engine would have to do, is not in the figure;
  box      one rv_world_edit call that clears the sphere's whole bounding box: what one box edit of the same
           extent costs (it clears other voxels; it has the same union box and so the same finish).
The first calls warm the code object and the context's scratch and are dropped; the figures are medians with
their minimum and maximum.  Before anything is timed the call's counts and the world it leaves are checked
against rv_world_edit_shapes_at, and the route's world against the call's.

  tools/shapes_latency.py [--world 10,10,10] [--radii 4 16 32 64] [--reps 7] [--out profiles/shapes_latency.json]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (C4's world: 10,10,10)")
    ap.add_argument("--radii", nargs="+", type=int, default=[4, 16, 32, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapes_latency.json"))
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
    generated = r.world_export(rv.RV_WORLD_BITS)
    commit, dirty = "", None   # the tree the figures were taken on; unknown outside a git checkout
    try:
        g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        if g.returncode == 0:
            commit = g.stdout.strip()
            dirty = bool(subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"],
                                        capture_output=True, text=True).stdout.strip())
    except OSError:
        pass
    res = {"what": "median (min - max) ms per repetition after warm-up, host clock, the generated world restored between "
                   "repetitions outside the timed region; shapes: rv_world_edit_shapes clearing one voxel-centred sphere; "
                   "route: the same voxels as rv_world_edit x-run boxes in calls of at most 1024 (boxes made before the "
                   "clock starts); box: one rv_world_edit clearing the sphere's bounding box",
           "log2_dims": list(lg), "reps": a.reps, "warm": a.warm, "pose_column": [px, pz], "surface_row": top,
           "commit": commit, "dirty": dirty, "rows": []}

    def restore():
        r.world_import(rv.RV_WORLD_BITS, generated)
        r.csdf_build()
        r.sync()
    for rad in a.radii:
        shape = (rv.RV_SHAPE_ELLIPSOID, 0, (2 * px + 1, 2 * top + 1, 2 * pz + 1), (2 * rad,) * 3)
        _, box = rv.edit_shapes_box(lg, [shape])
        restore()
        # the call against the host form
        want = rv.edit_shapes_at(lg, generated, [shape])
        got = r.world_edit_shapes([shape])
        assert got == want[1:] and got[1] > 0, (rad, got, want[1:])
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[0]), (rad, "bits")
        full = r.world_edit_info()[2]
        # the route: the x-runs of the voxels the call cleared
        gone, ox = sub_voxels(generated, lg, box)
        gone &= ~sub_voxels(want[0], lg, box)[0]
        runs = [b[:6] + (0,) for b in set_runs(gone, (ox, box[1], box[2]))]
        edits = [runs[i:i + 1024] for i in range(0, len(runs), 1024)]
        restore()
        for e in edits:
            r.world_edit(e)
        assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[0]), (rad, "route")
        restore()
        # the C calls on arrays made once: no allocation inside the timed region
        sarr = rv.render._edit_shapes([shape])
        ebuf = [(np.array(e, np.int32), len(e)) for e in edits]
        one = np.array([box + (0,)], np.int32)
        n_set, n_cleared = C.c_uint64(), C.c_uint64()

        def shapes():
            assert r._L.rv_world_edit_shapes(r._h, sarr, 1, C.byref(n_set), C.byref(n_cleared)) == 0

        def route():
            for arr, k in ebuf:
                assert r._L.rv_world_edit(r._h, arr.ctypes.data_as(C.POINTER(rv._lib.rv_edit_box)), k) == 0

        def single():
            assert r._L.rv_world_edit(r._h, one.ctypes.data_as(C.POINTER(rv._lib.rv_edit_box)), 1) == 0
        t_shapes = median_ms(shapes, a.reps, a.warm, restore)
        t_route = median_ms(route, a.reps, a.warm, restore)
        t_box = median_ms(single, a.reps, a.warm, restore)
        row = {"radius": rad, "box": list(box), "cleared_voxels": got[1], "whole_grid_csdf": bool(full),
               "route_edit_calls": len(edits), "route_boxes": len(runs), "shapes": t_shapes, "route": t_route, "box_edit": t_box}
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
