#!/usr/bin/env python3
"""Compare decode against the way a caller gets the same numbers without it, on one GPU: bench.py's 1 GiB volume (256 header words
+ N(10, 3^2), default_rng(1234)), one -b 8 and one eps = 1e-3 container, records and original HBM-resident, 43 chunks in one batch.

  compare    (a) uncompress_compare_device over the whole container + compare_finish_device
  baseline   (b) uncompress_device of the whole container, then torch reductions over original and decoded in float64:
                 max |d| and its index, sum of d * d, min and max of the original
  full       (c) uncompress_device of the whole container alone

Times are host clocks around calls that end in a device synchronise (medians over --reps calls after --warmup), the three
alternating.  A second pass with the per-kernel timers on (mrcz_set_timing) gives k_compare_fold's own time.  Every compare
result is checked against the baseline's numbers (max error and index, sum of squares within rounding, min and max).  --bench N
runs `python bench.py` N times in this tree and N times in the built checkout of the parent commit --parent-tree names, alternating.  Prints one JSON
object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from datacompressionfloat_amd import CHUNK_FLOATS, MrcZipCodec  # noqa: E402
from datacompressionfloat_amd._lib import MrczCompare  # noqa: E402

NFL = (1 << 30) // 4
EPS = 1e-3
STREAM_TBS = 6.0   # MI355X_MICROARCH: a 1.2 GB table swept in order reads at 6.0-6.1 TB/s


def _time(fns, reps, warmup):
    """median wall ms of every fn (each ends synchronised), the fns alternating"""
    ms = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": reps} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    out = {"volume": "1 GiB, 256 header words + N(10, 3^2), numpy default_rng(1234)", "chunks": (NFL + CHUNK_FLOATS - 1) // CHUNK_FLOATS,
           "device": torch.cuda.get_device_name(0), "timing": "host clock around synchronised calls, median", "containers": {}}
    codec = MrcZipCodec(0, max_batch_chunks=64)
    w = torch.from_numpy(bench.make_volume(NFL, 1234, True).view(np.int32)).to(codec.device)
    nch = out["chunks"]
    acc = torch.empty(nch * 8 * len(MrczCompare._fields_), dtype=torch.uint8, device=codec.device)
    dec = torch.empty(NFL, dtype=torch.int32, device=codec.device)
    for tag, kw in (("b8", dict(bits=8)), ("eps1e-3", dict(bits=0, abs_err=EPS))):
        rec = codec.compress_device(w, **kw)[0].clone()
        res = {}

        def compare():
            codec.uncompress_compare_device(rec, NFL, w, acc, abs_err=EPS)
            res["t"] = codec.compare_finish_device(acc, 0, nch)

        def full():
            codec.uncompress_device(rec, NFL, out=dec)

        def baseline():
            codec.uncompress_device(rec, NFL, out=dec)
            a = w[256:].view(torch.float32).to(torch.float64)
            d = dec[256:].view(torch.float32).to(torch.float64) - a
            e = d.abs()
            i = torch.argmax(e)
            res["b"] = (float(e[i]), int(i) + 256, float((d * d).sum()), float(a.min()), float(a.max()))

        t = _time({"compare": compare, "baseline": baseline, "full": full}, args.reps, args.warmup)
        tot, b = res["t"], res["b"]
        assert (tot.max_err, tot.max_err_index, tot.orig_min, tot.orig_max) == (b[0], b[1], b[3], b[4]), (tag, tot.max_err, tot.max_err_index, b)
        assert abs(tot.sum_err2 - b[2]) <= 1e-9 * b[2] + 1e-300, (tot.sum_err2, b[2])
        fold_ms = t["compare"]["median_ms"] - t["full"]["median_ms"]
        codec.set_timing(True)
        codec.uncompress_compare_device(rec, NFL, w, acc, abs_err=EPS)
        kern = {k: round(v, 4) for k, v in codec.last_timings().items()}
        codec.set_timing(False)
        out["containers"][tag] = {
            "record_bytes": int(rec.numel()), **t, "compare_minus_full_ms": round(fold_ms, 4),
            "ms_of_12N_bytes_at_%g_TBps" % STREAM_TBS: round(12 * NFL / (STREAM_TBS * 1e12) * 1e3, 4),
            "kernel_ms_timers_on": kern,
            "k_compare_fold_GBps_of_8N_read": round(8 * NFL / (kern.get("k_compare_fold", float("nan")) * 1e-3) / 1e9, 1),
            "result": {"max_err": tot.max_err, "max_err_index": tot.max_err_index, "rmse": float(np.sqrt(tot.sum_err2 / tot.n_finite)),
                       "n_over_abs": tot.n_over_abs, "n_diff": tot.n_diff}}
        del rec
    codec.close()
    del w, dec, acc
    torch.cuda.empty_cache()
    if args.bench:
        runs = {"this_commit": [], "parent": []}
        for _ in range(args.bench):
            for who in ("this_commit", "parent"):
                if who == "parent" and not args.parent_tree:
                    continue
                tree = os.path.abspath(args.parent_tree) if who == "parent" else ROOT
                r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline"],
                                   cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"bench.py ({who}) failed: {r.stderr[-2000:]}")
                runs[who].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
        out["bench_py"] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
