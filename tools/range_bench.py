#!/usr/bin/env python3
"""Range decode against whole-file decode on one GPU: the 1 GiB App. D volume (device generator, 43 chunks), b = 8.

  full    uncompress_device of all records (what bench.py's decompress half does)
  slab    one section-sized window (1 Mi words = 4 MiB) inside chunk 20, from that chunk's record alone (first_chunk = 20):
          what mrc_extract / read_mrc_slab decode after reading the covering record
  walk    the same window from the whole container (first_chunk = 0: the 20 records in front are walked on the device)

Times are CUDA-event medians over --reps calls (after --warmup), HBM-resident, no host copies.  A second pass with the
per-kernel timers on (mrcz_set_timing) gives the kernels' own times, k_merge_window among them, and the bytes the windowed
merge must move: the window's words out, at most the covering tiles of the four planes in.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from datacompressionfloat_amd import CHUNK_FLOATS as CHK, MrcZipCodec  # noqa: E402

MTILE = 4096  # plane positions per merge tile (mrcz_inflate_par.hip)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=20)
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    n = 268435456
    big = MrcZipCodec(0, max_batch_chunks=43)
    one = MrcZipCodec(0, max_batch_chunks=1)   # the slab's context: a workspace of one chunk
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    rec, _ = big.compress_device(words, a.bits, 0)
    rec = rec.clone()
    del words
    full = torch.empty(n, dtype=torch.int32, device="cuda")
    # chunk records: byte offsets from the 16-byte headers (read on the host: 16 bytes per chunk)
    offs, off = [], 0
    for _ in range(a.chunk + 1):
        offs.append(off)
        h = rec[off: off + 16].cpu().numpy().view("<u4")
        off += 16 + int(sum(int(x) & 0x7fffffff for x in h))
    offs.append(off)
    crec = rec[offs[a.chunk]: offs[a.chunk + 1]].clone()       # the covering record alone, in an allocation of its own
    w0 = a.chunk * CHK + 1000003                               # a 1024 x 1024 section that starts at no particular alignment
    w1 = w0 + 1048576
    sout = torch.empty(w1 - w0, dtype=torch.int32, device="cuda")

    res = {"workload": f"1 GiB App. D volume (device generator), b={a.bits}, 43 chunks; window = words [{w0}, {w1}) "
                       f"(1 Mi words, inside chunk {a.chunk}), HBM-resident",
           "gpu": torch.cuda.get_device_name(0), "record_bytes_all": int(rec.numel()), "record_bytes_chunk": int(crec.numel())}
    res["full"] = _time(lambda: big.uncompress_device(rec, n, out=full), a.reps, a.warmup)
    res["slab"] = _time(lambda: one.uncompress_range_device(crec, n, w0, w1, first_chunk=a.chunk, out=sout), a.reps, a.warmup)
    res["walk"] = _time(lambda: one.uncompress_range_device(rec, n, w0, w1, first_chunk=0, out=sout), a.reps, a.warmup)
    assert torch.equal(sout, full[w0:w1]), "range decode differs from the whole-file decode"
    res["slab_vs_full"] = round(res["slab"]["median_ms"] / res["full"]["median_ms"], 4)

    # kernels' own times (timers bracket every launch with a host sync: these are not the wall times above)
    for name, c, fn in (("full", big, lambda: big.uncompress_device(rec, n, out=full)),
                        ("slab", one, lambda: one.uncompress_range_device(crec, n, w0, w1, first_chunk=a.chunk, out=sout))):
        c.set_timing(True)
        fn()
        res[f"{name}_kernels_ms"] = {k: round(v, 4) for k, v in c.last_timings().items()}
        c.set_timing(False)
    t0, t1 = (w0 - a.chunk * CHK) // MTILE, (w1 - a.chunk * CHK + MTILE - 1) // MTILE
    res["merge_window_bytes"] = {"window_out": 4 * (w1 - w0), "covering_tiles": t1 - t0,
                                 "plane_bytes_in_max": 4 * MTILE * (t1 - t0),
                                 "note": "k_merge_window reads the four planes of the covering tiles only and writes the window; "
                                         "compare FETCH_SIZE / WRITE_SIZE of a --pmc run"}
    mw = res["slab_kernels_ms"].get("k_merge_window")
    if mw:
        res["merge_window_GBps"] = round((res["merge_window_bytes"]["window_out"] + res["merge_window_bytes"]["plane_bytes_in_max"]) / mw / 1e6, 1)
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
