#!/usr/bin/env python3
"""Effective clock and matrix-pipe busy fraction per kernel, from the one rocprofv3 pass
`--pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES --kernel-trace` of tools/kbench.py bf16 that tools/prof_all.sh makes:
python tools/pmc_busy_summary.py KERNEL_TRACE.csv COUNTER_COLLECTION.csv    (the ten kernels with the most time)"""
import collections
import csv
import re

import _common


def short(name):
    return re.sub(r"\(anonymous namespace\)::|void ", "", name)[:50]


def busy(kernel_trace_csv, counters_csv, label=short):
    """-> [(kernel, dispatches, ns, clock in GHz, MFMA-busy fraction)], most time first; label(name) names a kernel, None drops it."""
    dur = {r["Dispatch_Id"]: int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(kernel_trace_csv))}
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(counters_csv)):
        k = label(r["Kernel_Name"])
        if not k:
            continue
        acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "GRBM_GUI_ACTIVE":
            acc[k]["ns"] += dur.get(r["Dispatch_Id"], 0)
            acc[k]["n"] += 1
    rows = []
    for k, c in sorted(acc.items(), key=lambda kv: -kv[1]["ns"]):
        clk = c["GRBM_GUI_ACTIVE"] / 8 / max(c["ns"], 1)                         # GHz
        util = c["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024 / max(c["ns"] * clk, 1)      # busy cycles summed over 1024 SIMDs; wall cycles = ns * clk
        rows.append((k, int(c["n"]), c["ns"], clk, util))
    return rows


PARSER = _common.parser(__doc__)
PARSER.add_argument("kernel_trace_csv")
PARSER.add_argument("counters_csv")

if __name__ == "__main__":
    o = PARSER.parse_args()
    for k, n, ns, clk, util in busy(o.kernel_trace_csv, o.counters_csv)[:10]:
        print(f"{k:52s} n={n:4d} total={ns / 1e6:8.2f} ms clk={clk:5.2f} GHz  mfma_busy={util:5.2f}")
