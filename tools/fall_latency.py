#!/usr/bin/env python3
"""Time per call of rv_world_fall at C4's world (1024^3), over the scenes of tools/detached_latency.py: boxes of
32^3, 64^3 and 128^3 voxels centred on the terrain surface under the bench pose, with a few blocks in the air
("blocks") or everything above a cut come loose ("slab").

Timed with the host clock around the synchronous calls, the scene put back by rv_world_import + rv_csdf_build
between repetitions outside the timed region:
  fall     rv_world_fall, one round;
  clear    rv_world_detached with RV_DETACHED_CLEAR on the same scene;
  route    what the call replaces on the device side: that clear, then rv_world_edit calls that set the
           x-runs of the voxels at their landing rows, at most 1024 boxes each.  The boxes are made before
           the clock starts; the search for the landing rows, which an engine would do on the host after
           reading the world back (profiles/detached_latency.json, row readback), is not in the figure.
The first calls warm the code object and the context's scratch and are dropped; the figures are medians with
their minimum and maximum.  Before anything is timed the call's results and the world it leaves are checked
against rv_world_fall_at, and the route's world against the call's.

  tools/fall_latency.py [--world 10,10,10] [--sides 32 64 128] [--reps 10] [--out profiles/fall_latency.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from detached_latency import median_ms, scene, surface   # noqa: E402


def sub_voxels(bits, lg, box):
    """[z, y, x] of the voxel box grown to whole words along x, and the x it starts at."""
    X, Y, Z = (1 << l for l in lg)
    x0, y0, z0, x1, y1, z1 = box
    w0, w1 = x0 >> 5, ((x1 - 1) >> 5) + 1
    words = np.ascontiguousarray(bits.reshape(Z, Y, X // 32)[z0:z1, y0:y1, w0:w1])
    return np.unpackbits(words.view(np.uint8), bitorder="little").reshape(z1 - z0, y1 - y0, 32 * (w1 - w0)).astype(bool), 32 * w0


def set_runs(vox, origin):
    """One solid rv_world_edit box per run along x of the [z, y, x] array at `origin`."""
    ox, oy, oz = origin
    out = []
    for z, y in zip(*np.nonzero(vox.any(axis=2))):
        row = np.concatenate([[False], vox[z, y], [False]])
        edge = np.flatnonzero(row[1:] != row[:-1])
        out += [(ox + int(a), oy + int(y), oz + int(z), ox + int(b), oy + int(y) + 1, oz + int(z) + 1, 1)
                for a, b in zip(edge[::2], edge[1::2])]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (C4's world: 10,10,10)")
    ap.add_argument("--sides", nargs="+", type=int, default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fall_latency.json"))
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
    res = {"what": "median (min - max) ms per repetition after warm-up, host clock, the scene restored between "
                   "repetitions outside the timed region; fall: rv_world_fall, one round; clear: rv_world_detached "
                   "with RV_DETACHED_CLEAR; route: that clear, then rv_world_edit calls of at most 1024 boxes that "
                   "set the x-runs at their landing rows (boxes made before the clock starts)",
           "log2_dims": list(lg), "reps": a.reps, "warm": a.warm, "pose_column": [px, pz], "surface_row": top, "rows": []}
    for s in a.sides:
        lo = [int(np.clip(c - s // 2, 1, n - s - 1)) for c, n in ((px, X), (top, Y), (pz, Z))]
        box = (lo[0], lo[1], lo[2], lo[0] + s, lo[1] + s, lo[2] + s)
        for kind in ("blocks", "slab"):
            r.world_import(rv.RV_WORLD_BITS, generated)
            r.csdf_build()
            r.world_edit(scene(kind, box))
            bits = r.world_export(rv.RV_WORLD_BITS)

            def restore():
                r.world_import(rv.RV_WORLD_BITS, bits)
                r.csdf_build()
                r.sync()
            # the call against the host form
            want = rv.fall_at(lg, bits, box)
            got = r.world_fall(box)
            assert got[1:4] == want[1:4] and got[0].tobytes() == want[0].tobytes(), (s, kind, "fall")
            assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[4]), (s, kind, "bits")
            full = r.world_edit_info()[2]
            # the route: the clear, then the voxels the clear left unset at their landing places
            restore()
            r.world_detached(box, rv.RV_DETACHED_CLEAR, cap=0, want_mask=False)
            changed = want[3]
            landed, ox = sub_voxels(want[4], lg, changed)
            landed &= ~sub_voxels(r.world_export(rv.RV_WORLD_BITS), lg, changed)[0]
            runs = set_runs(landed, (ox, changed[1], changed[2]))
            edits = [runs[i:i + 1024] for i in range(0, len(runs), 1024)]
            for e in edits:
                r.world_edit(e)
            assert np.array_equal(r.world_export(rv.RV_WORLD_BITS), want[4]), (s, kind, "route")
            restore()
            # the C calls on arrays made once: no numpy allocation inside the timed region
            vb = rv._lib.rv_voxel_box(*box)
            n, v = C.c_int64(), C.c_uint64()
            ebuf = [(np.array(e, np.int32), len(e)) for e in edits]

            def fall():
                assert r._L.rv_world_fall(r._h, C.byref(vb), 0, None, 0, C.byref(n), C.byref(v), None) == 0

            def clear():
                assert r._L.rv_world_detached(r._h, C.byref(vb), rv.RV_DETACHED_CLEAR, None, 0, C.byref(n), C.byref(v),
                                              None, 0) == 0

            def route():
                clear()
                for arr, k in ebuf:
                    assert r._L.rv_world_edit(r._h, arr.ctypes.data_as(C.POINTER(rv._lib.rv_edit_box)), k) == 0
            t_fall = median_ms(fall, a.reps, a.warm, restore)
            t_clear = median_ms(clear, a.reps, a.warm, restore)
            t_route = median_ms(route, a.reps, a.warm, restore)
            row = {"side": s, "scene": kind, "box": list(box), "components": want[1], "moved_voxels": want[2],
                   "changed": list(changed), "whole_grid_csdf": bool(full), "route_edit_calls": len(edits),
                   "route_boxes": len(runs), "fall": t_fall, "clear": t_clear, "route": t_route}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
