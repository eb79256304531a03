#!/usr/bin/env python3
"""Developer tool (GPU): where k_emit's time goes, plane by plane, on the bench volume (1 GiB, N(10, 3^2)).

The kernel has no per-plane switch, so the split is made on the input side: besides the volume itself ("all") the tool
compresses copies of it in which only ONE byte plane keeps the volume's bytes and the other three are constant (a constant
plane is one run: its waves find no symbol start in a tile part and leave), and one copy in which all four are constant
("none": the kernel's floor).  k_emit is timed by the context timers (timing mode: one lane, one launch per call).

  python tools/emit_plane_split.py [--bits B] [--reps R]          one JSON line per variant with the k_emit times
  rocprofv3 --pmc <counters> -d DIR -- python tools/emit_plane_split.py --one-launch
                                                                  exactly one k_emit launch per variant, in the order of
                                                                  VARIANTS: tools/emit_pmc_fold.py DIR maps them back
MRCZ_LIB_PATH selects the build of the kernels."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ["all", "none", "plane0", "plane1", "plane2", "plane3"]
CONST = 0x41200000  # 10.0f: the bytes the constant planes hold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one-launch", action="store_true", help="one timing-mode compress per variant and nothing else (counter runs)")
    args = ap.parse_args()

    import torch
    import bench
    from datacompressionfloat_amd import MrcZipCodec

    n = 1 << 28
    dev = torch.device("cuda", 0)
    w = torch.from_numpy(bench.make_volume(n, 1234, True).view("int32")).to(dev)
    nchunks = (n + bench.CHUNK - 1) // bench.CHUNK
    codec = MrcZipCodec(0, max_batch_chunks=nchunks)
    rec_buf = torch.empty(codec.records_bound(n), dtype=torch.uint8, device=dev)
    codec.set_timing(True)
    v = torch.empty_like(w)
    for name in VARIANTS:
        if name == "all":
            v.copy_(w)
        elif name == "none":
            v.fill_(CONST)
        else:
            keep = 0xff << (8 * int(name[-1]))
            keep_i32 = keep - (1 << 32) if keep >= (1 << 31) else keep
            torch.bitwise_and(w, keep_i32, out=v)
            v.bitwise_or_(CONST & ~keep & 0xffffffff)
        ms = []
        for _ in range(1 if args.one_launch else args.reps):
            rec, planes = codec.compress_device(v, args.bits, 0, out=rec_buf)
            ms.append(round(codec.last_timings().get("k_emit", 0.0), 4))
        print(json.dumps({"variant": name, "bits": args.bits, "k_emit_ms": ms, "zbytes": int(rec.numel()),
                          "plane_bytes": [int(p) for p in planes]}), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
