#!/usr/bin/env python3
"""Time per call of rv_world_detached at C4's world (1024^3) for boxes of 32^3, 64^3 and 128^3 voxels centred on
the terrain surface under the bench pose.

Two scenes per box, both made with rv_world_edit:
  blocks   a few 3^3 blocks placed in the air of the box's upper half;
  slab     a one-voxel slab cleared under the whole box a quarter of its height up, and a one-voxel moat
           cleared around the box from there to its top, so that everything of the box above the slab comes
           loose.
Timed with the host clock around the synchronous call: the query alone, and the query with RV_DETACHED_CLEAR
(the scene is put back by rv_world_import + rv_csdf_build between clearing calls, outside the timed region).
The first calls warm the code object and the context's scratch and are dropped; the figures are medians with
their minimum and maximum.  Beside it, timed the same way, the route the call replaces: rv_world_export of the
bits and rv_world_detached_at, the same query on the CPU.  Before anything is timed each result is checked
against rv_world_detached_at.

  tools/detached_latency.py [--world 10,10,10] [--sides 32 64 128] [--reps 20] [--out profiles/detached_latency.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warm, between=None):
    ms = []
    for _ in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
        if between:
            between()
    ms = ms[warm:]
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def surface(r, x, z, Y):
    """The highest solid row + 1 of column (x, z)."""
    col = r.world_columns_read([(x >> 3, z >> 3)])[0]
    vox = np.unpackbits(col.view(np.uint8), bitorder="little").reshape(8, Y, 8)   # [z, y, x] of the brick column
    rows = vox[z & 7, :, x & 7].nonzero()[0]
    return int(rows.max()) + 1 if len(rows) else 0


def scene(kind, box):
    x0, y0, z0, x1, y1, z1 = box
    s = x1 - x0
    if kind == "blocks":
        at = [(x0 + s // 4, y1 - s // 4), (x0 + s // 2, y1 - s // 8 - 3), (x1 - s // 4, y1 - s // 4 - 2)]
        return [(x, y, z0 + s // 3 + 2 * i, x + 3, y + 3, z0 + s // 3 + 2 * i + 3, 1) for i, (x, y) in enumerate(at)]
    k = y0 + s // 4
    return [(x0 - 1, k, z0 - 1, x1 + 1, k + 1, z1 + 1, 0),
            (x0 - 1, k, z0 - 1, x0, y1, z1 + 1, 0), (x1, k, z0 - 1, x1 + 1, y1, z1 + 1, 0),
            (x0, k, z0 - 1, x1, y1, z0, 0), (x0, k, z1, x1, y1, z1 + 1, 0)]


def same(a, b):
    return a[1:3] == b[1:3] and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[3], b[3])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (C4's world: 10,10,10)")
    ap.add_argument("--sides", nargs="+", type=int, default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detached_latency.json"))
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
    res = {"what": "median (min - max) ms per synchronous call after warm-up, host clock; query: rv_world_detached; "
                   "clear: with RV_DETACHED_CLEAR, the scene restored between calls outside the timed region; "
                   "readback: rv_world_export of the bits + rv_world_detached_at, the route the call replaces",
           "log2_dims": list(lg), "reps": a.reps, "warm": a.warm, "pose_column": [px, pz], "surface_row": top, "rows": []}
    for s in a.sides:
        lo = [int(np.clip(c - s // 2, 1, n - s - 1)) for c, n in ((px, X), (top, Y), (pz, Z))]
        box = (lo[0], lo[1], lo[2], lo[0] + s, lo[1] + s, lo[2] + s)
        for kind in ("blocks", "slab"):
            r.world_import(rv.RV_WORLD_BITS, generated)
            r.csdf_build()
            r.world_edit(scene(kind, box))
            bits = r.world_export(rv.RV_WORLD_BITS)
            want = rv.detached_at(lg, bits, box)
            assert same(r.world_detached(box), want), (s, kind, "query")
            cap = max(want[1], 1)
            # the C call on arrays made once: no numpy allocation inside the timed region
            vb = rv._lib.rv_voxel_box(*box)
            comps, mask = np.zeros(cap, rv.COMPONENT_DTYPE), np.zeros((s ** 3 + 31) // 32, np.uint32)
            n, v = C.c_int64(), C.c_uint64()

            def call(flags):
                assert r._L.rv_world_detached(r._h, C.byref(vb), flags, comps.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                              C.byref(v), mask.ctypes.data_as(C.c_void_p), mask.nbytes) == 0

            def restore():
                r.world_import(rv.RV_WORLD_BITS, bits)
                r.csdf_build()
                r.sync()
            got = r.world_detached(box, rv.RV_DETACHED_CLEAR, cap=cap)
            assert same(got, want) and r.world_detached(box)[2] == 0, (s, kind, "clear")
            full = r.world_edit_info()[2]
            restore()
            query = median_ms(lambda: call(0), a.reps, a.warm)
            clear = median_ms(lambda: call(rv.RV_DETACHED_CLEAR), a.reps, a.warm, restore)
            back = median_ms(lambda: rv.detached_at(lg, r.world_export(rv.RV_WORLD_BITS), box, cap=cap), a.reps, a.warm)
            row = {"side": s, "scene": kind, "box": list(box), "components": want[1], "detached_voxels": want[2],
                   "clear_whole_grid_csdf": bool(full), "query": query, "clear": clear, "readback": back}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
