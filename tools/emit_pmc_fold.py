#!/usr/bin/env python3
"""Fold a `rocprofv3 --pmc ... -- python tools/emit_plane_split.py --one-launch` run: the k_emit launches of the run, in
dispatch order, are the variants of emit_plane_split.VARIANTS; prints one JSON line per variant with the counters of its launch.
Usage: python tools/emit_pmc_fold.py DIR"""
import collections
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emit_plane_split import VARIANTS

rows = collections.defaultdict(dict)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if k == "k_emit":
            d = rows[int(r["Dispatch_Id"])]
            d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
ids = sorted(rows)
if len(ids) != len(VARIANTS):
    sys.exit(f"{len(ids)} k_emit launches, expected {len(VARIANTS)}")
for name, i in zip(VARIANTS, ids):
    print(json.dumps({"variant": name, "counters": {c: rows[i][c] for c in sorted(rows[i])}}))
