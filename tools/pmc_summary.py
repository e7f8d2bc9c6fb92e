#!/usr/bin/env python3
"""Summarise a rocprofv3 --pmc counter_collection.csv: per kernel (short name) mean counter values per dispatch.
python tools/pmc_summary.py DIR...    (each DIR holds one *counter_collection.csv, directly or one level down)"""
import collections
import csv
import glob

import _common
from pmc_busy_summary import short


PARSER = _common.parser(__doc__)
PARSER.add_argument("dirs", nargs="+", metavar="DIR")

if __name__ == "__main__":
    for d in PARSER.parse_args().dirs:
        f = glob.glob(d + "/*/*counter_collection.csv") + glob.glob(d + "/*counter_collection.csv")
        acc = collections.defaultdict(lambda: collections.defaultdict(list))
        for r in csv.DictReader(open(f[0])):
            acc[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k, cs in acc.items():
            print(k, "dispatches", len(next(iter(cs.values()))))
            for c, v in cs.items():
                print(f"    {c:28s} mean {sum(v) / len(v):16.1f}")
