#!/usr/bin/env python3
"""One line of a bench.py result file: headline, compress / decompress, k_emit in timing mode, parity.
Usage: python tools/bench_brief.py FILE [label ...]"""
import json
import sys

d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
km = d["roofline"]["kernel_ms"]
print(" ".join(sys.argv[2:]), "value", d["value"], "ms_per_step", d["ms_per_step"], "compress_GBps", d["compress_GBps"], "decompress_GBps", d["decompress_GBps"],
      "k_emit", km.get("k_emit"), "parity", (d.get("cpu_baseline") or {}).get("parity_check"))
