#!/usr/bin/env python3
"""Box decode against whole-file decode on one GPU: the 1 GiB App. D volume (device generator) read as a float32 MRC volume
(header words nx = ny = 1024, nz = 255, mode 2, nsymbt 0: data from word 256), b = 8, 43 chunks.

  dense     768 boxes of 64^3 tiling z in [0, 192) (16 x 16 x 3)
  many      2000 boxes of 32^3 at seeded random centres, some over the edges
  one       a single 64^3 box in mid-volume; one_range = uncompress_range_device over the same chunk span
  baseline  uncompress_device of all records, then a torch gather of the dense (and the many) boxes

Records are HBM-resident and the box calls get the whole container (chunks no box touches are walked, not decoded).  Times are
CUDA-event medians over --reps calls after --warmup.  A second pass with the per-kernel timers on (mrcz_set_timing) gives
every kernel's own time, k_gather_boxes and k_fill_boxes among them, and the chunks decoded.  Device memory of a fresh context
doing the many case is read from hipMemGetInfo.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from datacompressionfloat_amd import CHUNK_FLOATS as CHK, MrcZipCodec  # noqa: E402
from datacompressionfloat_amd._lib import MrczBoxGeom  # noqa: E402

NX, NY, NZ, D0 = 1024, 1024, 255, 256


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps}


def _gather_index(org, size):
    """flat file-word index of every box voxel (0 where outside) and the inside mask, on the device"""
    o = torch.from_numpy(np.asarray(org, np.int64)).cuda()
    r = torch.arange(size, device="cuda")
    x = o[:, 0, None, None, None] + r[None, None, None, :]
    y = o[:, 1, None, None, None] + r[None, None, :, None]
    z = o[:, 2, None, None, None] + r[None, :, None, None]
    inside = (x >= 0) & (x < NX) & (y >= 0) & (y < NY) & (z >= 0) & (z < NZ)
    return torch.where(inside, D0 + (z * NY + y) * NX + x, torch.zeros_like(x)), inside


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    n = 268435456
    big = MrcZipCodec(0, max_batch_chunks=43)
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    words[0:4] = torch.tensor([NX, NY, NZ, 2], dtype=torch.int32, device="cuda")
    words[23] = 0
    rec, _ = big.compress_device(words, a.bits, 0)
    rec = rec.clone()
    del words
    full = torch.empty(n, dtype=torch.int32, device="cuda")

    def geom(size):
        return MrczBoxGeom(D0, NX, NY, NZ, size, size, size, 0)

    dense = np.array([(x, y, z) for z in range(0, 192, 64) for y in range(0, NY, 64) for x in range(0, NX, 64)], np.int32)
    rng = np.random.default_rng(2024)
    centres = np.stack([rng.uniform(-20, NX + 20, 2000), rng.uniform(-20, NY + 20, 2000), rng.uniform(-20, NZ + 20, 2000)], 1)
    many = (np.floor(centres + 0.5) - 16).astype(np.int32)
    one = np.array([[512 - 32, 512 - 32, 128 - 32]], np.int32)
    cases = {"dense": (dense, 64), "many": (many, 32), "one": (one, 64)}
    outs = {k: torch.empty((len(o), s, s, s), dtype=torch.int32, device="cuda") for k, (o, s) in cases.items()}

    res = {"workload": f"1 GiB App. D volume (device generator) as a {NX} x {NY} x {NZ} float32 MRC volume, b={a.bits}, 43 chunks, "
                       "HBM-resident records, whole container passed to every box call",
           "gpu": torch.cuda.get_device_name(0), "record_bytes_all": int(rec.numel())}
    res["full"] = _time(lambda: big.uncompress_device(rec, n, out=full), a.reps, a.warmup)
    for k, (o, s) in cases.items():
        res[k] = _time(lambda: big.uncompress_boxes_device(rec, n, geom(s), o, out=outs[k]), a.reps, a.warmup)
        res[k]["boxes"], res[k]["size"] = len(o), s
        res[k]["out_bytes"] = 4 * len(o) * s ** 3
    # the one box's chunks through range decode: the same chunk span, all of its words
    w0 = D0 + int(one[0, 2]) * NX * NY + int(one[0, 1]) * NX + int(one[0, 0])
    w1 = D0 + (int(one[0, 2]) + 63) * NX * NY + (int(one[0, 1]) + 63) * NX + int(one[0, 0]) + 64
    c_lo, c_hi = w0 // CHK, (w1 + CHK - 1) // CHK
    rout = torch.empty(c_hi * CHK - c_lo * CHK, dtype=torch.int32, device="cuda")
    rw1 = min(c_hi * CHK, n)
    res["one_range"] = _time(lambda: big.uncompress_range_device(rec, n, c_lo * CHK, rw1, out=rout), a.reps, a.warmup)
    res["one_range"]["chunks"] = [c_lo, c_hi]
    res["one_vs_range"] = round(res["one"]["median_ms"] / res["one_range"]["median_ms"], 4)

    # baseline: the whole volume decoded, then the boxes gathered by torch
    for k in ("dense", "many"):
        o, s = cases[k]
        idx, inside = _gather_index(o, s)

        def base():
            big.uncompress_device(rec, n, out=full)
            return torch.where(inside, full[idx], torch.zeros_like(full[:1]))
        res[f"baseline_{k}"] = _time(base, a.reps, a.warmup)
        big.uncompress_boxes_device(rec, n, geom(s), o, out=outs[k])
        assert torch.equal(outs[k], base()), f"box decode differs from decode + gather ({k})"
        del idx, inside
    res["dense_vs_baseline"] = round(res["dense"]["median_ms"] / res["baseline_dense"]["median_ms"], 4)

    # kernels' own times and chunks decoded (timers bracket every launch with a host sync: not the wall times above)
    for k, (o, s) in cases.items():
        big.set_timing(True)
        _, dec = big.uncompress_boxes_device(rec, n, geom(s), o, out=outs[k])
        t = big.last_timings()
        big.set_timing(False)
        res[k]["chunks_decoded"] = dec
        res[k]["kernels_ms"] = {kk: round(v, 4) for kk, v in t.items()}
        res[k]["gather_fill_ms"] = round(t.get("k_gather_boxes", 0.0) + t.get("k_fill_boxes", 0.0), 4)
        res[k]["gather_fill_share_of_kernels"] = round(res[k]["gather_fill_ms"] / sum(t.values()), 4)
    big.close()

    # device memory of the many case on a fresh context: records + workspace + staging + output, no decoded volume
    torch.cuda.synchronize()
    free0, total = torch.cuda.mem_get_info()
    ctx = MrcZipCodec(0, max_batch_chunks=16)
    o, s = cases["many"]
    ctx.uncompress_boxes_device(rec, n, geom(s), o, out=outs["many"])
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    res["many_memory"] = {"context_bytes_after_call": int(free0 - free1), "staging_bytes": 16 * CHK * 4,
                          "records_bytes": int(rec.numel()), "out_bytes": res["many"]["out_bytes"], "decoded_volume_bytes": 4 * n,
                          "note": "context_bytes_after_call = workspace + planes + scratch + staging of a 16-chunk context"}
    ctx.close()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
