#!/usr/bin/env python3
"""Digest decode against decode alone and against compare decode, on one GPU: bench.py's 1 GiB volume (256 header words +
N(10, 3^2), default_rng(1234)), one -b 8 and one eps = 1e-3 container, records and original HBM-resident, 43 chunks in one batch.

  digest     (a) uncompress_digest_device over the whole container + digest_finish_device
  full       (b) uncompress_device of the whole container alone
  compare    (c) uncompress_compare_device + compare_finish_device on the same container (the closest existing streaming fold)
  words_*    (d) digest_words_device of the resident original + digest_finish_device, xform None and the container's own

Times are host clocks around calls that end in a device synchronise (medians over --reps calls after --warmup), the variants
alternating.  A second pass with the per-kernel timers on (mrcz_set_timing) gives k_crc_fold's and k_crc_chunk's own times.  The
digest is checked against zlib.crc32 of the host copy of the decoded volume.  The kernel_trace block of profiles/digest.json comes from a run of its own,
  rocprofv3 --kernel-trace --stats -d DIR -o digest -- python tools/digest_bench.py --trace
(--trace: five digest decodes and five digest_words MASK of the -b 8 volume, nothing timed), read from the top_kernels view of
DIR/digest_results.db with the template argument kept in the name.  --bench N runs `python bench.py` N times in this
tree and N times in the built checkout of the parent commit --parent-tree names, alternating.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

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
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        codec = MrcZipCodec(0, max_batch_chunks=64)
        w = torch.from_numpy(bench.make_volume(NFL, 1234, True).view(np.int32)).to(codec.device)
        rec = codec.compress_device(w, 8)[0].clone()
        acc = torch.empty(16 * ((NFL + CHUNK_FLOATS - 1) // CHUNK_FLOATS), dtype=torch.uint8, device=codec.device)
        for _ in range(5):
            codec.uncompress_digest_device(rec, NFL, acc)
            codec.digest_words_device(w, "mask", 8, acc=acc)
        print(json.dumps({"trace": "done", "crc32": "%08x" % codec.digest_finish_device(acc, 0, acc.numel() // 16)[0]}))
        return
    out = {"volume": "1 GiB, 256 header words + N(10, 3^2), numpy default_rng(1234)", "chunks": (NFL + CHUNK_FLOATS - 1) // CHUNK_FLOATS,
           "device": torch.cuda.get_device_name(0), "timing": "host clock around synchronised calls, median", "containers": {}}
    codec = MrcZipCodec(0, max_batch_chunks=64)
    w = torch.from_numpy(bench.make_volume(NFL, 1234, True).view(np.int32)).to(codec.device)
    nch = out["chunks"]
    acc = torch.empty(nch * 16, dtype=torch.uint8, device=codec.device)
    cacc = torch.empty(nch * 8 * len(MrczCompare._fields_), dtype=torch.uint8, device=codec.device)
    dec = torch.empty(NFL, dtype=torch.int32, device=codec.device)
    for tag, kw, xf in (("b8", dict(bits=8), dict(xform="mask", bits=8)), ("eps1e-3", dict(bits=0, abs_err=EPS), dict(xform="abs", abs_err=EPS))):
        rec = codec.compress_device(w, **kw)[0].clone()
        res = {}

        def digest():
            codec.uncompress_digest_device(rec, NFL, acc)
            res["d"] = codec.digest_finish_device(acc, 0, nch)

        def full():
            codec.uncompress_device(rec, NFL, out=dec)

        def compare():
            codec.uncompress_compare_device(rec, NFL, w, cacc, abs_err=EPS)
            codec.compare_finish_device(cacc, 0, nch)

        def words_none():
            codec.digest_words_device(w, acc=acc)
            res["n"] = codec.digest_finish_device(acc, 0, nch)

        def words_mode():
            codec.digest_words_device(w, acc=acc, **xf)
            res["m"] = codec.digest_finish_device(acc, 0, nch)

        t = _time({"digest": digest, "full": full, "compare": compare, "words_none": words_none, "words_mode": words_mode}, args.reps, args.warmup)
        full()
        want = zlib.crc32(dec.cpu().numpy().tobytes())
        assert res["d"] == (want, 4 * NFL) and res["m"] == (want, 4 * NFL), (tag, res, want)
        assert res["n"][0] == zlib.crc32(w.cpu().numpy().tobytes())
        kern = {}
        codec.set_timing(True)
        codec.uncompress_digest_device(rec, NFL, acc)
        kern["uncompress_digest"] = {k: round(v, 4) for k, v in codec.last_timings().items()}
        codec.uncompress_compare_device(rec, NFL, w, cacc, abs_err=EPS)
        kern["uncompress_compare"] = {k: round(v, 4) for k, v in codec.last_timings().items() if k.startswith("k_compare")}
        codec.digest_words_device(w, acc=acc, **xf)
        kern["digest_words_mode"] = {k: round(v, 4) for k, v in codec.last_timings().items()}
        codec.set_timing(False)
        fold = kern["uncompress_digest"].get("k_crc_fold", float("nan"))
        out["containers"][tag] = {
            "record_bytes": int(rec.numel()), **t, "digest_minus_full_ms": round(t["digest"]["median_ms"] - t["full"]["median_ms"], 4),
            "ms_of_4N_bytes_at_%g_TBps" % STREAM_TBS: round(4 * NFL / (STREAM_TBS * 1e12) * 1e3, 4),
            "kernel_ms_timers_on": kern, "k_crc_fold_GBps_of_4N_read": round(4 * NFL / (fold * 1e-3) / 1e9, 1),
            "crc32": "%08x" % want}
        del rec
    codec.close()
    del w, dec, acc, cacc
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
