#!/usr/bin/env python3
"""Top-planes decode against the full decode, on one GPU: bench.py's 1 GiB volume (256 header words + N(10, 3^2),
default_rng(1234)) in four containers (-b 0, -b 8, -b 12, eps = 1e-3), records HBM-resident, 43 chunks in one batch.

  kept_share    kept payload bytes / container bytes for keep 2 and 3, from the chunk headers (exact; --shares-only needs no GPU
                beyond the compress that makes the containers)
  full          uncompress_device alone
  full_mask     uncompress_device, then the torch `&` a caller needs today for the keep-3 words
  full_bf16     uncompress_device, then the torch shift and narrowing a caller needs today for bfloat16 bit patterns
  top2_u16      uncompress_top_device keep 2, torch.bfloat16
  top2_f32      uncompress_top_device keep 2, torch.float32
  top3_f32      uncompress_top_device keep 3, torch.float32

Times are host clocks around calls that end in a device synchronise (medians over --reps calls after --warmup), the cases
alternating.  A second pass with the per-kernel timers on (mrcz_set_timing) gives every kernel's own time per case: k_merge_top
against k_merge_segments, k_blk_count with 2, 3 and 4 planes.  Every top result is checked against full & mask on the device.
The kernel_trace block of profiles/top_decode.json comes from a run of its own,
  rocprofv3 --kernel-trace --stats -d DIR -o top -- python tools/top_bench.py --trace
(--trace: five decodes of every case of the -b 8 volume, nothing timed).  --bench N runs `python bench.py` N times in this tree
and N times in the built checkout of the parent commit --parent-tree names, alternating.  Prints one JSON object."""
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

NFL = (1 << 30) // 4
EPS = 1e-3
CONTAINERS = (("b0", dict(bits=0)), ("b8", dict(bits=8)), ("b12", dict(bits=12)), ("eps1e-3", dict(bits=0, abs_err=EPS)))


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


def kept_share(rec: bytes, nfl: int, chk: int = CHUNK_FLOATS):
    """kept payload bytes over container bytes (17-byte file header included) for keep 2 and 3, and the plane sums"""
    planes, off = [0, 0, 0, 0], 0
    for _ in range((nfl + chk - 1) // chk):
        ln = [int(x) & 0x7fffffff for x in np.frombuffer(rec[off: off + 16], "<u4")]
        planes = [a + b for a, b in zip(planes, ln)]
        off += 16 + sum(ln)
    assert off == len(rec)
    tot = 17 + len(rec)
    return {"container_bytes": tot, "plane_payload_bytes": planes, "keep2": round(sum(planes[2:]) / tot, 6), "keep3": round(sum(planes[1:]) / tot, 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench", type=int, default=0)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shares-only", action="store_true")
    args = ap.parse_args()
    codec = MrcZipCodec(0, max_batch_chunks=64)
    w = torch.from_numpy(bench.make_volume(NFL, 1234, True).view(np.int32)).to(codec.device)
    dec = torch.empty(NFL, dtype=torch.int32, device=codec.device)
    o32 = torch.empty(NFL, dtype=torch.float32, device=codec.device)
    o16 = torch.empty(NFL, dtype=torch.bfloat16, device=codec.device)
    out = {"volume": "1 GiB, 256 header words + N(10, 3^2), numpy default_rng(1234)", "chunks": (NFL + CHUNK_FLOATS - 1) // CHUNK_FLOATS,
           "device": torch.cuda.get_device_name(0), "timing": "host clock around synchronised calls, median", "containers": {}}
    for tag, kw in CONTAINERS:
        if args.trace and tag != "b8":
            continue
        rec = codec.compress_device(w, **kw)[0].clone()
        cases = {
            "full": lambda: codec.uncompress_device(rec, NFL, out=dec),
            "full_mask": lambda: codec.uncompress_device(rec, NFL, out=dec)[0].bitwise_and_(-256),
            "full_bf16": lambda: (codec.uncompress_device(rec, NFL, out=dec)[0] >> 16).to(torch.int16),
            "top2_u16": lambda: codec.uncompress_top_device(rec, NFL, 2, torch.bfloat16, out=o16),
            "top2_f32": lambda: codec.uncompress_top_device(rec, NFL, 2, torch.float32, out=o32),
            "top3_f32": lambda: codec.uncompress_top_device(rec, NFL, 3, torch.float32, out=o32),
        }
        if args.trace:
            for _ in range(5):
                for k in ("full", "top2_u16", "top2_f32", "top3_f32"):
                    cases[k]()
            print(json.dumps({"trace": "done"}))
            return
        res = {"record_bytes": int(rec.numel()), "kept_share": kept_share(rec.cpu().numpy().tobytes(), NFL)}
        if not args.shares_only:
            # correctness first: every case against the full decode under its mask, on the device
            codec.uncompress_device(rec, NFL, out=dec)
            assert torch.equal(cases["top2_u16"]().view(torch.int16), (dec >> 16).to(torch.int16)), tag
            assert torch.equal(cases["top2_f32"]().view(torch.int32), dec & -65536), tag
            assert torch.equal(cases["top3_f32"]().view(torch.int32), dec & -256), tag
            res.update(_time(cases, args.reps, args.warmup))
            for k in ("top2_u16", "top2_f32", "top3_f32"):
                res[k]["over_full"] = round(res[k]["median_ms"] / res["full"]["median_ms"], 4)
            res["top2_u16"]["over_full_bf16"] = round(res["top2_u16"]["median_ms"] / res["full_bf16"]["median_ms"], 4)
            res["top3_f32"]["over_full_mask"] = round(res["top3_f32"]["median_ms"] / res["full_mask"]["median_ms"], 4)
            kern = {}
            codec.set_timing(True)
            for k in ("full", "top2_u16", "top2_f32", "top3_f32"):
                cases[k]()
                kern[k] = {n: round(v, 4) for n, v in codec.last_timings().items()}
            codec.set_timing(False)
            res["kernel_ms_timers_on"] = kern
            ms = lambda k, n: kern[k].get(n, float("nan"))
            res["merge"] = {"k_merge_segments_ms": ms("full", "k_merge_segments"), "k_merge_segments_bytes": 8 * NFL,
                            "k_merge_top_2_u16_ms": ms("top2_u16", "k_merge_top"), "k_merge_top_2_u16_bytes": 4 * NFL,
                            "k_merge_top_2_f32_ms": ms("top2_f32", "k_merge_top"), "k_merge_top_2_f32_bytes": 6 * NFL,
                            "k_merge_top_3_f32_ms": ms("top3_f32", "k_merge_top"), "k_merge_top_3_f32_bytes": 7 * NFL}
            res["k_blk_count_ms"] = {"4_planes": ms("full", "k_blk_count"), "3_planes": ms("top3_f32", "k_blk_count"), "2_planes": ms("top2_u16", "k_blk_count")}
        out["containers"][tag] = res
        del rec
    codec.close()
    del w, dec, o32, o16
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
