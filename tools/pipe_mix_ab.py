#!/usr/bin/env python3
"""A/B of RV_OPT_PIPE_MIX settings on one GPU, in ONE context (one world build): the native loop as
bench.py runs it (rv_render_frame_seq over the bench's camera path, one k_ref_pipe launch per frame, the
same 20 warm-up + 200 timed frames for every setting), the settings taken in turn, ROUNDS times over.
Prints every run and, per setting, the median and the range.  Not part of the product.

usage: python tools/pipe_mix_ab.py [config] [pose] [rounds] [steps] [WxH]
       PIPE_MIX_SETTINGS="0 1:0:4 1:0:4@1/8 ..." overrides the settings (r_pp:r_gi:r_render[@head
       as a fraction of the pre-pass rows])
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ["0"] + [f"{p}{h}" for h in ("", "@1/8", "@1/4") for p in ("1:0:4", "1:0:3", "1:0:2", "1:1:4")]


def pack(spec, pp_rows):
    if spec == "0":
        return 0
    pat, _, head = spec.partition("@")
    rp, rg, rr = (int(v) for v in pat.split(":"))
    h = 0
    if head:
        a, b = (int(v) for v in head.split("/"))
        h = pp_rows * a // b
    return h << 24 | rp << 16 | rg << 8 | rr


def main():
    import torch
    import rvgrt_amd as rv
    from rvgrt_amd.atlas import load_atlas
    from rvgrt_amd.configs import CONFIGS, camera_path, pose_f32

    cfg = CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "c4"]
    pose = sys.argv[2] if len(sys.argv) > 2 else "P0"
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    if len(sys.argv) > 5:   # the configuration's world and frame at another size
        import dataclasses
        w, h = (int(v) for v in sys.argv[5].lower().split("x"))
        cfg = dataclasses.replace(cfg, width=w, height=h)
    warmup, settle = 20, 100
    settings = os.environ.get("PIPE_MIX_SETTINGS", "").split() or DEFAULT
    torch.cuda.set_device(0)
    W, H = cfg.width, cfg.height
    pp_rows = ((W // 2 + 7) // 8) * ((H // 2 + 7) // 8) // 8   # 8x8-texel waves of the half-res grid, 8 per row
    r = rv.StateRender((cfg.log2_n,) * 3, W, H, flags=cfg.flags, atlas=load_atlas())
    r.set_frames_in_flight(1)
    r.set_frame_group(0)   # one pipelined launch per frame
    r.world_build()
    for s in range(max(cfg.gi_sweeps, 0)):
        r.gi_update(s)
    r.sync()
    path = camera_path(pose_f32(cfg, pose), W, H, max(settle, warmup + steps) + 1)

    def run(a, k):
        r.render_frame_seq(path[a:a + k], next_desc=path[a + k], flags=cfg.flags, gi_per_frame=True)

    run(0, settle)
    r.sync()
    ms = {s: [] for s in settings}
    print(f"{cfg.name} {pose}: {W}x{H}, {pp_rows} pre-pass rows, {rounds} rounds of {steps} frames", flush=True)
    for i in range(rounds):
        for s in settings:
            r.set_option(rv.RV_OPT_PIPE_MIX, pack(s, pp_rows))
            run(0, warmup)
            r.sync()
            t0 = time.perf_counter()
            run(warmup, steps)
            r.sync()
            v = (time.perf_counter() - t0) * 1e3 / steps
            assert r.get_option(rv.RV_OPT_PIPE_MIX_LAST) == pack(s, pp_rows)
            ms[s].append(v)
            print(f"  round {i} {s:12s} {v:.4f} ms/frame", flush=True)
    base = statistics.median(ms[settings[0]])
    print(f"{'setting':12s} {'packed':>12s} {'median':>8s} {'min':>8s} {'max':>8s} {'vs ' + settings[0]:>8s}")
    for s in settings:
        m = statistics.median(ms[s])
        print(f"{s:12s} {pack(s, pp_rows):#12x} {m:8.4f} {min(ms[s]):8.4f} {max(ms[s]):8.4f} {m / base:8.4f}")
    r.close()


if __name__ == "__main__":
    main()
