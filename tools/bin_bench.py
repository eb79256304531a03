#!/usr/bin/env python3
"""Binned decode against whole-file decode on one GPU: the 1 GiB App. D volume (device generator) read as a float32 MRC volume
(nx = ny = 1024, nz = 255, data from word 256; the file's last 1048320 words are a tail after the volume), b = 8, 43 chunks.

  bin2, bin4, bin1x1x255   uncompress_binned_device over the whole container + binned_finish_device, factors 2, 4, (1, 1, 255)
  full                     uncompress_device of all records alone
  baseline_*               uncompress_device of all records, then torch avg_pool3d (float32) of the volume

Records are HBM-resident.  Times are CUDA-event medians over --reps calls after --warmup, on one 43-chunk context (the whole
container in one batch, as full decode runs it) and again on a 16-chunk context (three batches: the streaming shape).  A second
pass with the per-kernel timers on (mrcz_set_timing) gives every kernel's own time, k_bin_fold among them.  Each result is
checked bit for bit against a float64 torch fold of the full decode.  Device memory of a fresh 16-chunk context doing factor 2 is
read from hipMemGetInfo.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from datacompressionfloat_amd import MrcZipCodec  # noqa: E402
from datacompressionfloat_amd._lib import MrczBinGeom  # noqa: E402

NX, NY, NZ, D0 = 1024, 1024, 255, 256
FACTORS = {"bin2": (2, 2, 2), "bin4": (4, 4, 4), "bin1x1x255": (1, 1, 255)}


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


def _fold(full, f):
    """the binned volume in float64 torch: the voxels of a bin added in file order, the first one first"""
    fx, fy, fz = f
    mz, my, mx = NZ // fz, NY // fy, NX // fx
    v = full[D0: D0 + NX * NY * NZ].view(torch.float32).reshape(NZ, NY, NX)[: mz * fz, : my * fy, : mx * fx].reshape(mz, fz, my, fy, mx, fx)
    s = None
    for k in range(fz):
        for j in range(fy):
            for l in range(fx):
                t = v[:, k, :, j, :, l].to(torch.float64)
                s = t.clone() if s is None else s.add_(t)
    return (s / float(fx * fy * fz)).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    n = 268435456
    big = MrcZipCodec(0, max_batch_chunks=43)
    small = MrcZipCodec(0, max_batch_chunks=16)
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    words[0:4] = torch.tensor([NX, NY, NZ, 2], dtype=torch.int32, device="cuda")
    words[23] = 0
    rec, _ = big.compress_device(words, a.bits, 0)
    rec = rec.clone()
    del words
    full = torch.empty(n, dtype=torch.int32, device="cuda")

    def geom(f):
        return MrczBinGeom(D0, NX, NY, NZ, *f)

    res = {"workload": f"1 GiB App. D volume (device generator) as a {NX} x {NY} x {NZ} float32 MRC volume, b={a.bits}, 43 chunks, "
                       "HBM-resident records, whole container passed to every binned call",
           "gpu": torch.cuda.get_device_name(0), "record_bytes_all": int(rec.numel())}
    res["full"] = _time(lambda: big.uncompress_device(rec, n, out=full), a.reps, a.warmup)
    vol = full[D0: D0 + NX * NY * NZ].view(torch.float32).reshape(1, 1, NZ, NY, NX)
    for k, f in FACTORS.items():
        g = geom(f)
        shape = (NZ // f[2], NY // f[1], NX // f[0])
        acc = torch.empty(shape, dtype=torch.float64, device="cuda")
        out = torch.empty(shape, dtype=torch.float32, device="cuda")

        def binned(c=big):
            c.uncompress_binned_device(rec, n, g, acc)
            c.binned_finish_device(g, acc, out)
        res[k] = _time(binned, a.reps, a.warmup)
        res[k]["context16"] = _time(lambda: binned(small), a.reps, a.warmup)
        res[k]["factor"], res[k]["out_shape"] = list(f), list(shape)
        res[k]["vs_full"] = round(res[k]["median_ms"] / res["full"]["median_ms"], 4)

        def base():
            big.uncompress_device(rec, n, out=full)
            return torch.nn.functional.avg_pool3d(vol, (f[2], f[1], f[0]))
        res[f"baseline_{k}"] = _time(base, a.reps, a.warmup)
        res[k]["vs_baseline"] = round(res[k]["median_ms"] / res[f"baseline_{k}"]["median_ms"], 4)
        pool = base()[0, 0]
        binned()
        assert torch.equal(out.view(torch.int32), _fold(full, f).view(torch.int32)), f"binned decode differs from the fold ({k})"
        res[k]["max_abs_diff_vs_avg_pool3d"] = float((out - pool).abs().max())
        # kernels' own times and chunks decoded (timers bracket every launch with a host sync: not the wall times above)
        big.set_timing(True)
        dec = big.uncompress_binned_device(rec, n, g, acc)
        t = big.last_timings()
        big.binned_finish_device(g, acc, out)
        t.update(big.last_timings())
        big.set_timing(False)
        res[k]["chunks_decoded"] = dec
        res[k]["kernels_ms"] = {kk: round(v, 4) for kk, v in t.items()}
        res[k]["fold_finish_ms"] = round(t.get("k_bin_fold", 0.0) + t.get("k_binned_finish", 0.0), 4)
        res[k]["fold_share_of_kernels"] = round(t.get("k_bin_fold", 0.0) / sum(t.values()), 4)
        res[k]["fold_bytes"] = 4 * NX * NY * NZ + 16 * shape[0] * shape[1] * shape[2]
        res[k]["fold_GBps"] = round(res[k]["fold_bytes"] / (t.get("k_bin_fold", 1e9) * 1e-3) / 1e9, 1)
        del acc, out
    big.close()
    small.close()
    del vol
    torch.cuda.synchronize()

    # device memory of factor 2 on a fresh context: workspace + staging of the context, the sums and the output; no decoded volume
    f = FACTORS["bin2"]
    nbins = (NZ // 2) * (NY // 2) * (NX // 2)
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    ctx = MrcZipCodec(0, max_batch_chunks=16)
    acc = torch.empty(nbins, dtype=torch.float64, device="cuda")
    out = torch.empty(nbins, dtype=torch.float32, device="cuda")
    ctx.uncompress_binned_device(rec, n, geom(f), acc)
    ctx.binned_finish_device(geom(f), acc, out)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    res["bin2_memory"] = {"bytes_after_call": int(free0 - free1), "acc_bytes": 8 * nbins, "out_bytes": 4 * nbins,
                          "staging_bytes": 16 * 6 * 1048576 * 4, "records_bytes": int(rec.numel()), "decoded_volume_bytes": 4 * n,
                          "note": "bytes_after_call = a 16-chunk context (workspace, planes, scratch, staging) + acc + out "
                                  "(torch's caching allocator rounds acc and out up to its blocks)"}
    ctx.close()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(s + "\n")


if __name__ == "__main__":
    main()
