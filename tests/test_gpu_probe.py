"""GPU: the probe on the MI355X (mrcz_probe_chunks through MrcZipCodec.probe_device, MrcZipCodec.sweep, choose, mrc_verify -p).
Every expectation comes from the CPU oracle and numpy (tests/probe_ref.py): the size is the length of the oracle's container of the
setting, the plane sums those of its chunk headers, and every chunk record the numpy fold of tests/compare_ref.py over the original
and what the container decodes to: counts, extremes and indices exactly, the sums within compare_ref.assert_matches' bound.  On top
of that the records must equal, in counts, extremes and indices, what compare decode assigns for the container compress_device
really writes.  No point and no chunk is left out of any comparison."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compare_ref as ref
import probe_ref as pr
import util
from abs_error_ref import f32_toward_zero

pytestmark = pytest.mark.gpu

BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")
CHK = util.CHUNK
EPS = f32_toward_zero(0.01)
RSZ = ctypes.sizeof(ref.Compare)
BOUNDS = dict(err_abs=1e-3, err_rel=2.0 ** -10)
THREE_SETTINGS = [("bits", 0), ("bits", 8), ("bits", 12), ("abs", EPS), ("int",)]
ids = lambda s: "-".join(str(v) for v in s)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def small(oracle):
    """the 300 001-word volume and what all 33 mask levels must give with the bounds off (computed once)"""
    w = pr.small_volume()
    return w, [pr.expectation(oracle, w, ("bits", b)) for b in range(33)]


@pytest.fixture(scope="module")
def three(oracle):
    """the three-chunk volume of tests/test_sim_binned.py and a cache of what each setting must give"""
    from test_sim_binned import _volume
    w = _volume()
    cache = {}

    def want(setting):
        if setting not in cache:
            cache[setting] = pr.expectation(oracle, w, setting, 1e-3, 2.0 ** -10)
        return cache[setting]
    return w, want


def kw_of(setting):
    if setting[0] == "bits":
        return dict(bits=setting[1])
    return dict(abs_err=float(setting[1])) if setting[0] == "abs" else dict(int_mode=True)


def probe(torch, codec, dw, setting, nch, first_chunk=0, acc=None, garbage=0xA5, bounds=BOUNDS):
    """(record bytes, plane_bytes, chunk records, raw accumulator bytes) of one probe_device call"""
    if acc is None:
        acc = torch.full((nch * RSZ,), garbage, dtype=torch.uint8, device=codec.device)       # d_acc needs no zeroing
    size, planes, acc = codec.probe_device(dw, first_chunk=first_chunk, acc=acc, **kw_of(setting), **bounds)
    raw = acc.cpu().numpy().tobytes()
    return size, planes, pr.records(raw, nch), raw


def check_row(row, setting, want, fsz):
    assert row["setting"] == setting and row["container_bytes"] == want["container_bytes"] and row["plane_bytes"] == want["plane_bytes"]
    assert row["ratio"] == fsz / want["container_bytes"]
    ref.assert_matches(row, want["total"], (setting, "sweep"))
    for k, x in ref.derived(want["total"]).items():
        assert row[k] == x or abs(row[k] - x) <= 1e-9 * abs(x), (setting, k, row[k], x)


def test_short_chunk_all_33_mask_levels_sweep_and_choose(torch, small, oracle):
    from datacompressionfloat_amd import MrcZipCodec, choose
    w, wants = small
    codec = MrcZipCodec(0, max_batch_chunks=2)
    dw = torch.from_numpy(w.view(np.int32).copy()).to(codec.device)
    for b, want in enumerate(wants):
        size, planes, recs, _ = probe(torch, codec, dw, ("bits", b), 1, bounds={})
        pr.assert_probe(size, planes, recs, want, ("bits", b))
    for b in (8, 23):                                                         # and with both bounds on
        size, planes, recs, _ = probe(torch, codec, dw, ("bits", b), 1)
        pr.assert_probe(size, planes, recs, pr.expectation(oracle, w, ("bits", b), 1e-3, 2.0 ** -10), ("bits", b, "bounded"))
    rows, plain = codec.sweep(w.tobytes(), per_chunk=True), codec.sweep(w.tobytes())
    assert len(rows) == len(plain) == 33
    for b, (row, want) in enumerate(zip(rows, wants)):
        check_row(row, ("bits", b), want, 4 * len(w))
        assert len(row["chunks"]) == 1 and {k: v for k, v in row.items() if k != "chunks"} == plain[b]
        for k in ref.COUNTS + ref.EXACT:
            assert row["chunks"][0][k] == want["chunks"][0][k], (b, k)
    # choose: the row numpy picks = the smallest oracle container among the levels whose numpy max_err is within x, the first on a tie
    for x in (0.0, wants[12]["total"]["max_err"], 0.3, 1e30):
        ok = [b for b in range(33) if wants[b]["total"]["max_err"] <= x]
        pick = min(ok, key=lambda b: (wants[b]["container_bytes"], b))
        assert choose(rows, max_err=x) is rows[pick], (x, pick)
    assert choose(rows, max_err=-1.0) is None
    codec.close()


def test_sweep_of_a_file_with_no_words(torch):
    from datacompressionfloat_amd import MrcZipCodec
    codec = MrcZipCodec(0, max_batch_chunks=2)
    rows = codec.sweep(b"abc", settings=[("bits", 8), ("int",)])
    assert [(r["setting"], r["container_bytes"], r["ratio"], r["n"], r["n_finite"], r["psnr_db"]) for r in rows] == \
        [(("bits", 8), 0, 0.0, 0, 0, float("inf")), (("int",), 0, 0.0, 0, 0, float("inf"))]
    codec.close()


@pytest.mark.parametrize("setting", THREE_SETTINGS, ids=ids)
def test_three_chunks_across_a_batch_boundary(torch, three, setting):
    """batches of 2 + 1 chunks: the oracle's size, the numpy fold, and compare decode of the container compress_device writes"""
    from datacompressionfloat_amd import MrcZipCodec
    w, want_of = three
    want = want_of(setting)
    codec = MrcZipCodec(0, max_batch_chunks=2)
    dw = torch.from_numpy(w.view(np.int32).copy()).to(codec.device)
    size, planes, recs, _ = probe(torch, codec, dw, setting, 3)
    pr.assert_probe(size, planes, recs, want, setting)
    rec, cplanes = codec.compress_device(dw, **{"bits": 0, **kw_of(setting)})
    assert rec.numel() == size and cplanes == planes
    acc = torch.full((3 * RSZ,), 0x5A, dtype=torch.uint8, device=codec.device)
    codec.uncompress_compare_device(rec, len(w), dw, acc, abs_err=BOUNDS["err_abs"], rel_err=BOUNDS["err_rel"], int_mode=setting == ("int",))
    for c, (g, x) in enumerate(zip(recs, pr.records(acc.cpu().numpy().tobytes(), 3))):
        for k in ref.COUNTS + ref.EXACT:
            assert g[k] == x[k], (setting, c, k, g[k], x[k])
    codec.close()


def test_three_chunks_cuts_do_not_change_bits_or_sizes(torch, three):
    from datacompressionfloat_amd import MrcZipCodec
    w, want_of = three
    want = want_of(("bits", 8))
    two, one, whole = (MrcZipCodec(0, max_batch_chunks=m) for m in (2, 1, 3))
    dw = torch.from_numpy(w.view(np.int32).copy()).to(two.device)
    size, planes, _, base = probe(torch, two, dw, ("bits", 8), 3)
    assert size == want["record_bytes"]
    for c in (one, whole):
        assert probe(torch, c, dw, ("bits", 8), 3, garbage=0x3C) == (size, planes, pr.records(base, 3), base)
    acc = torch.full((3 * RSZ,), 0x77, dtype=torch.uint8, device=two.device)
    sizes = [probe(torch, c, dw[k * CHK: (k + 1) * CHK], ("bits", 8), 3, first_chunk=k, acc=acc)[0] for c, k in ((whole, 2), (one, 1), (two, 0))]
    offs = want["offsets"]
    assert sizes == [offs[k + 1] - offs[k] for k in (2, 1, 0)] and acc.cpu().numpy().tobytes() == base
    s, p, _, _ = probe(torch, two, dw[CHK:], ("bits", 8), 3, first_chunk=1)     # the records from chunk 1 on
    assert s == offs[3] - offs[1] and p == pr.plane_sums(want["z"], len(w), first_chunk=1)
    for c in (two, one, whole):
        c.close()


def test_three_chunks_sweep_from_a_path_bytes_and_a_tensor(torch, three, tmp_path):
    from datacompressionfloat_amd import MrcZipCodec
    w, want_of = three
    settings = [("bits", 8), ("abs", float(EPS)), ("int",), ("bits", 0)]
    codec = MrcZipCodec(0, max_batch_chunks=2)
    path = tmp_path / "vol.mrc"
    path.write_bytes(w.tobytes())
    from_path = codec.sweep(path, settings)
    assert codec.sweep(w.tobytes(), settings) == from_path
    assert codec.sweep(torch.from_numpy(w.view(np.int32).copy()).to(codec.device), settings) == from_path
    for row, st, key in zip(from_path, settings, (("bits", 8), ("abs", EPS), ("int",), ("bits", 0))):
        want = want_of(key)
        assert row["setting"] == st and row["container_bytes"] == want["container_bytes"] and row["plane_bytes"] == want["plane_bytes"]
        for k in ref.COUNTS[:5] + ref.EXACT:                                  # (the sweep's bounds are off)
            assert row[k] == want["total"][k], (st, k)
    codec.close()


def test_eight_chunks_where_compress_runs_two_lanes(torch, oracle):
    from datacompressionfloat_amd import MrcZipCodec
    w = util.kat_words(8 * CHK)
    z = oracle.compress(w.tobytes(), 8, threads=16)
    codec = MrcZipCodec(0)
    dw = torch.from_numpy(w.view(np.int32)).to(codec.device)
    rec, cplanes = codec.compress_device(dw, 8)
    size, planes, _ = codec.probe_device(dw, 8)
    assert size == rec.numel() == len(z) - 17 and planes == cplanes == pr.plane_sums(z, len(w))
    rec, _ = codec.compress_device(dw, 8)                                     # straight after the probe
    assert rec.cpu().numpy().tobytes() == z[17:]
    codec.close()


def test_mrc_verify_p(small, oracle, tmp_path):
    w, wants = small
    f = tmp_path / "f.mrc"
    f.write_bytes(w.tobytes())
    run = lambda spec: subprocess.run([os.path.join(BIN, "mrc_verify"), "-a", str(f), "-p", spec], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, timeout=120)
    r = run("b0:2,b8,e0.01,int")
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert all(p[0] == "probe" for p in lines) and len(lines) == 6
    expect = [("b %d" % b, wants[b]) for b in (0, 1, 2, 8)] + [("e 0.01", pr.expectation(oracle, w, ("abs", EPS))), ("int", pr.expectation(oracle, w, ("int",)))]
    for p, (label, want) in zip(lines, expect):
        k = p.index("bytes")
        assert " ".join(p[1:k]) == label
        got = dict(zip(p[k::2], p[k + 1::2]))
        assert list(got) == ["bytes", "ratio", "max_err", "rmse", "psnr_db", "special_diff"]
        t, d = want["total"], ref.derived(want["total"])
        assert int(got["bytes"]) == want["container_bytes"] and float(got["ratio"]) == 4 * len(w) / want["container_bytes"]
        assert float(got["max_err"]) == t["max_err"] and repr(float(got["max_err"])) == repr(t["max_err"])
        assert int(got["special_diff"]) == t["n_special_diff"]
        for key in ("rmse", "psnr_db"):
            assert float(got[key]) == d[key] or abs(float(got[key]) - d[key]) <= 1e-9 * abs(d[key]), (label, key)
    # a bad SPEC leaves through die(): status 255, no signal (checked only after the run above came back clean)
    for spec in ("b33", "b5:3", "e0", "x8", "b1,,b2", ""):
        r = run(spec)
        assert r.returncode == 255 and "ERROR" in r.stderr and r.stdout == "", (spec, r.returncode, r.stderr)
