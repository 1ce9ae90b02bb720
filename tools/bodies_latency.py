#!/usr/bin/env python3
"""Time per call of rv_world_bodies_move at C4's world (1024^3) for n = 1, 10^3, 10^5 and 10^6 bodies.

Two workloads, both placed by the library itself (the bodies are dropped onto the generated terrain with
rv_world_bodies_move until every one stands on the ground):
  debris   boxes of size 0.25 a few voxels above the ground, falling by 0.5 a call with a small drift;
  players  0.6 x 1.8 x 0.6 boxes standing on the ground, walking by up to 0.3 a call under a pull of -0.1.
The host form (host arrays, synchronous) is timed with the host clock around the call; the device form
(caller-owned device arrays, enqueued) with the host clock around the call plus rv_sync.  The first calls
warm the code object and the context's scratch and are dropped; the figures are medians, and bodies per
second from them.  For context only -- not an equivalent -- rv_trace_rays over the same n is timed the same
way: the existing call with the same upload, launch and download plumbing.  Before anything is timed a
4096-body sample of each workload is checked against rv_world_bodies_move_at on the exported bits.

  tools/bodies_latency.py [--world 10,10,10] [--counts 1 1000 100000 1000000] [--reps 20]
                          [--out profiles/bodies_latency.json]
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

F = np.float32


class Device:
    """Device buffers from the HIP runtime the library loaded."""
    def __init__(self):
        for name in ("libamdhip64.so", "libamdhip64.so.7"):
            try:
                self.L = C.CDLL(name)
                break
            except OSError:
                continue
        else:
            raise RuntimeError("no HIP runtime")
        self.owned = []

    def malloc(self, n):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
        self.owned.append(p)
        return p.value

    def upload(self, dst, arr):
        assert self.L.hipMemcpy(C.c_void_p(dst), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1) == 0

    def download(self, arr, src):
        assert self.L.hipMemcpy(arr.ctypes.data_as(C.c_void_p), C.c_void_p(src), C.c_size_t(arr.nbytes), 2) == 0

    def close(self):
        self.L.hipDeviceSynchronize()
        for p in self.owned:
            self.L.hipFree(p)


def timed(r, fn):
    r.sync()
    t0 = time.perf_counter()
    fn()
    r.sync()
    return (time.perf_counter() - t0) * 1e3


def median_ms(r, fn, reps, warm):
    ms = [timed(r, fn) for _ in range(warm + reps)][warm:]
    return statistics.median(ms), min(ms), max(ms)


def dropped(r, rng, n, dims, size):
    """n boxes of this size standing on the terrain: dropped from the top of the window."""
    X, Y, Z = dims
    lo = np.stack([rng.uniform(8, X - 8, n), np.full(n, Y - 4.0), rng.uniform(8, Z - 8, n)], 1).astype(F)
    fall = np.array([0.0, -64.0, 0.0], F)
    for _ in range(Y // 64 + 1):
        lo, fl = r.bodies_move(lo, size, fall)
    assert (fl & 4).all(), "a body did not land"
    return lo


def workloads(r, rng, n, dims):
    debris = dropped(r, rng, n, dims, (0.25, 0.25, 0.25))
    debris[:, 1] += rng.uniform(0.5, 8.0, n).astype(F)
    drift = rng.normal(0, 0.05, (n, 3)).astype(F)
    drift[:, 1] = F(-0.5)
    players = dropped(r, rng, n, dims, (0.6, 1.8, 0.6))
    walk = rng.uniform(-0.3, 0.3, (n, 3)).astype(F)
    walk[:, 1] = F(-0.1)
    return {"debris": (debris, np.broadcast_to(np.array([0.25, 0.25, 0.25], F), (n, 3)), drift),
            "players": (players, np.broadcast_to(np.array([0.6, 1.8, 0.6], F), (n, 3)), walk)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", default="10,10,10", help="log2 dims (C4's world: 10,10,10)")
    ap.add_argument("--counts", nargs="+", type=int, default=[1, 1000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bodies_latency.json"))
    a = ap.parse_args()
    import rvgrt_amd as rv
    lg = tuple(int(v) for v in a.world.split(","))
    dims = tuple(1 << l for l in lg)
    r = rv.StateRender(lg, 320, 192, tex_table=-1)
    r.world_build()
    rng = np.random.default_rng(1)
    nmax = max(a.counts + [4096])
    work = workloads(r, rng, nmax, dims)

    bits = r.world_export(rv.RV_WORLD_BITS)
    checked = {}
    for name, (lo, size, delta) in work.items():
        got = r.bodies_move(lo[:4096], size[:4096], delta[:4096])
        want = rv.bodies_move_at(lg, bits, lo[:4096], size[:4096], delta[:4096])
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1]), name
        checked[name] = {"bodies": 4096, "blocked": int((got[1] & 63).astype(bool).sum()),
                         "on_ground": int((got[1] & 4).astype(bool).sum())}
    del bits

    dev = Device()
    d_in, d_out = dev.malloc(36 * nmax), dev.malloc(16 * nmax)
    res = {"what": "median ms per call after warm-up, host clock; host form = the synchronous call, device form = "
                   "the call + rv_sync; trace_rays: rv_trace_rays over the same n, for context only",
           "log2_dims": list(lg), "reps": a.reps, "warm": a.warm, "checked_against_move_at": checked, "rows": []}
    for name, (lo, size, delta) in work.items():
        for n in a.counts:
            b = np.empty((n, 9), F)
            b[:, 0:3], b[:, 3:6], b[:, 6:9] = lo[:n], size[:n], delta[:n]
            dev.upload(d_in, b)
            hout = np.zeros((n, 4), np.uint32)
            pb, pout = b.ctypes.data_as(C.c_void_p), hout.ctypes.data_as(C.c_void_p)

            def host_call():     # the C call on packed arrays: no numpy packing inside the timed region
                assert r._L.rv_world_bodies_move(r._h, pb, n, 0, pout) == 0
            host = median_ms(r, host_call, a.reps, a.warm)
            devf = median_ms(r, lambda: r.bodies_move_device(d_in, n, d_out), a.reps, a.warm)
            out = np.zeros((n, 4), np.uint32)
            dev.download(out, d_out)
            assert np.array_equal(out, hout), "the two forms differ"
            org = (lo[:n] + size[:n] * F(0.5)).astype(F)
            dirs = np.broadcast_to(np.array([0.0, -1.0, 0.0], F), (n, 3))
            rays = median_ms(r, lambda: r.trace_rays(org, dirs, np.zeros(n, F)), max(3, a.reps // 4), 2)
            row = {"workload": name, "n": n,
                   "host_ms": round(host[0], 4), "host_min_ms": round(host[1], 4), "host_max_ms": round(host[2], 4),
                   "device_ms": round(devf[0], 4), "device_min_ms": round(devf[1], 4),
                   "device_max_ms": round(devf[2], 4),
                   "host_bodies_per_s": round(n / (host[0] * 1e-3)), "device_bodies_per_s": round(n / (devf[0] * 1e-3)),
                   "trace_rays_ms": round(rays[0], 4)}
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
    dev.close()
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
