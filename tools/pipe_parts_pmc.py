#!/usr/bin/env python3
"""VALU-issue and TD-busy fractions of each part of the reference frame, from rocprofv3 --pmc passes of the
unpipelined loop (bench.py --pipe 0: k_prepass, k_gi_update and k_render as separate kernels), with
bench.py binding_limit's formulas: GRBM_GUI_ACTIVE / 8 = cycles, TD busy = TD_TD_BUSY_sum / (256 cycles),
VALU issue = SQ_INSTS_VALU / (2 * 256 cycles).  SQ_WAIT_INST_ANY and SQ_BUSY_CYCLES are printed per
cycle where the passes hold them.

    python tools/pipe_parts_pmc.py DIR [DIR ...]     directories holding *counter_collection.csv
"""
import collections
import csv
import glob
import os
import sys

PARTS = [("pre-pass", "k_prepass"), ("GI update", "k_gi_update"), ("render", "k_render")]


def main():
    rows = {p: [] for p, _ in PARTS}
    for d in sys.argv[1:]:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for part, key in PARTS:
                    if key in row["Kernel_Name"]:
                        rows[part].append((row["Grid_Size"], row["Counter_Name"], float(row["Counter_Value"])))
    # the frame loop's launches only: the kernel's most frequent grid (the world build's full GI sweeps are larger)
    vals = {p: collections.defaultdict(list) for p, _ in PARTS}
    for part, rs in rows.items():
        if rs:
            grid = collections.Counter(g for g, _, _ in rs).most_common(1)[0][0]
            for g, name, v in rs:
                if g == grid:
                    vals[part][name].append(v)
    print(f"{'part':10s} {'launches':>8s} {'cycles':>10s} {'us@2.4GHz':>10s} {'VALU insts':>12s} {'valu_issue':>10s} "
          f"{'td_busy':>8s} {'wait_any/wave-cyc':>18s} {'sq_busy/cyc':>12s}")
    for part, _ in PARTS:
        v = vals[part]
        avg = {k: sum(x) / len(x) for k, x in v.items()}
        cyc = avg.get("GRBM_GUI_ACTIVE", 0.0) / 8.0
        if cyc <= 0:
            print(f"{part:10s} no GRBM_GUI_ACTIVE rows")
            continue
        n = len(v["GRBM_GUI_ACTIVE"])
        valu = avg.get("SQ_INSTS_VALU", float("nan")) / (2.0 * 256.0 * cyc)
        td = avg.get("TD_TD_BUSY_sum", float("nan")) / (256.0 * cyc)
        # SQ_WAIT_INST_ANY counts wave-cycles spent waiting; per cycle and SIMD (1024 SIMDs): waiting waves
        wait = avg.get("SQ_WAIT_INST_ANY", float("nan")) / (1024.0 * cyc)
        busy = avg.get("SQ_BUSY_CYCLES", float("nan")) / cyc
        print(f"{part:10s} {n:8d} {cyc:10.0f} {cyc / 2400.0:10.1f} {avg.get('SQ_INSTS_VALU', float('nan')):12.0f} "
              f"{valu:10.3f} {td:8.3f} {wait:18.2f} {busy:12.2f}")


if __name__ == "__main__":
    main()
