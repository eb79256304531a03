"""CPU-only: compare decode (mrcz_uncompress_compare, k_compare_fold, k_compare_chunk, mrcz_compare_finish) on the SIMT emulator
build of the product sources.  The three-chunk volume of tests/test_sim_binned.py (chunk boundaries inside sections, +-0, denormals,
+-Inf, NaN, noisy and constant regions) is compressed by the CPU oracle at -b 8, at -b 0 and, rounded by abs_error_ref.abs_round
first, at an absolute bound; every chunk record and the total must equal the numpy fold of tests/compare_ref.py over the oracle's
decode: counts, extremes and indices exactly, the sums within (n + 2) * 2^-53 * fsum(|terms|) (any order of adding n doubles is
within that of the exact sum; the + 2 covers the rounding of d * d, which the device may contract into an fma).  No point is left
out of any comparison."""
import ctypes
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import compare_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero
from test_sim_binned import N, _offsets, _volume

EINVAL, EFORMAT = -1, -4
CHK = util.CHUNK
EPS = f32_toward_zero(0.01)
GARBAGE = 0xA5


def bind(lib):
    vp, u64, u32, i32, f64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double
    lib.mrcz_uncompress_compare.argtypes = [vp, vp, u64, u64, u32, u64, u64, vp, f64, f64, i32, vp]
    lib.mrcz_compare_finish.argtypes = [vp, vp, u64, u64, vp]


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    bind(s.lib)
    return s


@pytest.fixture(scope="module")
def data(oracle):
    w = _volume()
    rounded = abs_round(w, EPS)
    z8, z0, ze, zi = oracle.compress(w.tobytes(), 8), oracle.compress(w.tobytes(), 0), oracle.compress(rounded.tobytes(), 0), oracle.compress_int(w.tobytes())
    dec = lambda z, **kw: np.frombuffer(oracle.uncompress(z, **kw), np.uint32)
    return {"w": w, "b8": (z8[17:], dec(z8)), "b0": (z0[17:], dec(z0)), "eps": (ze[17:], dec(ze)), "int": (zi[17:], dec(zi, int_mode=True))}


def new_acc(nchunks):
    a = util.aligned_empty(ctypes.sizeof(ref.Compare) * max(nchunks, 1))
    a[:] = GARBAGE                                  # d_acc needs no zeroing
    return a


def records(acc, nchunks):
    return [ref.as_dict(ref.Compare.from_buffer_copy(acc[i * ctypes.sizeof(ref.Compare):].tobytes()[: ctypes.sizeof(ref.Compare)])) for i in range(nchunks)]


def step(lib, ctx, rec, orig, nfl, acc, first_chunk=0, nchunks=None, eps_abs=-1.0, eps_rel=-1.0, int_mode=False, chk=CHK, null=()):
    """one mrcz_uncompress_compare: rec = the records of chunks [first_chunk, first_chunk + nchunks), orig = the file's words"""
    if nchunks is None:
        nchunks = (nfl + CHK - 1) // CHK - first_chunk
    r = util.aligned_empty(len(rec) + 8)
    r[: len(rec)] = np.frombuffer(bytes(rec), np.uint8)
    a, b = first_chunk * CHK, min((first_chunk + nchunks) * CHK, nfl)
    o = util.aligned_empty(4 * max(b - a, 4)).view(np.uint32)
    o[: max(b - a, 0)] = orig[a:b]
    return lib.mrcz_uncompress_compare(ctx, None if "rec" in null else r.ctypes.data, len(rec), nfl, chk, first_chunk, nchunks,
                                       None if "orig" in null else o.ctypes.data, eps_abs, eps_rel, 1 if int_mode else 0,
                                       None if "acc" in null else acc.ctypes.data)


def finish(lib, ctx, acc, first_chunk, nchunks):
    t = ref.Compare()
    assert lib.mrcz_compare_finish(ctx, acc.ctypes.data, first_chunk, nchunks, ctypes.byref(t)) == 0
    return ref.as_dict(t)


def compare(sim, rec, orig, nfl=N, pieces=None, ctx=None, **kw):
    """(chunk records, total, raw accumulator bytes) of a file compared in pieces [(first_chunk, nchunks)] (default: one call)"""
    ctx = ctx or sim
    nch = (nfl + CHK - 1) // CHK
    offs = _offsets(rec, nfl)
    acc = new_acc(nch)
    for k, n in pieces or [(0, nch)]:
        rc = step(sim.lib, ctx.ctx, rec[offs[k]: offs[k + n]], orig, nfl, acc, k, n, **kw)
        assert rc == 0, sim.lib.mrcz_last_error(ctx.ctx)
    return records(acc, nch), finish(sim.lib, ctx.ctx, acc, 0, nch), acc[: nch * ctypes.sizeof(ref.Compare)].tobytes()


def check(sim, rec, orig, dec, nfl=N, eps_abs=None, eps_rel=None, **kw):
    want = ref.fold_chunks(orig[:nfl], dec[:nfl], CHK, eps_abs, eps_rel)
    got, tot, _ = compare(sim, rec, orig, nfl, eps_abs=-1.0 if eps_abs is None else eps_abs, eps_rel=-1.0 if eps_rel is None else eps_rel, **kw)
    for c, (g, w) in enumerate(zip(got, want)):
        ref.assert_matches(g, w, f"chunk {c}")
    wt = ref.total(want)
    ref.assert_matches(tot, wt, "total")
    return tot, wt


def test_b8_equals_the_numpy_fold_and_the_mask_bounds_the_relative_error(sim, data):
    rec, dec = data["b8"]
    tot, want = check(sim, rec, data["w"], dec)
    assert tot["n"] == N - 256 and tot["n_header_diff"] == 0 and tot["n_special_diff"] == 0
    assert tot["n_diff"] > 100000 and tot["max_err"] > 0 and 0 < tot["n_finite"] < tot["n"]   # NaN and Inf words are in the volume
    assert tot["first_over"] == ref.NONE and tot["n_over_abs"] == tot["n_over_rel"] == 0       # both checks off
    # the mask's own guarantee: |x - x'| < 2^(8 - 23) |x|
    tot, _ = check(sim, rec, data["w"], dec, eps_rel=2.0 ** -15)
    assert tot["n_over_rel"] == 0 and tot["first_over"] == ref.NONE
    tot, want = check(sim, rec, data["w"], dec, eps_rel=2.0 ** -17, eps_abs=1e-4)
    assert tot["n_over_rel"] == want["n_over_rel"] > 0 and tot["n_over_abs"] == want["n_over_abs"] > 0
    assert tot["first_over"] == want["first_over"] != ref.NONE


def test_lossless_container_has_no_error(sim, data):
    rec, dec = data["b0"]
    tot, _ = check(sim, rec, data["w"], dec, eps_abs=0.0, eps_rel=0.0)
    for k in ("n_diff", "n_header_diff", "n_special_diff", "n_over_abs", "n_over_rel", "max_err", "max_rel", "sum_err", "sum_abs_err", "sum_err2"):
        assert tot[k] == 0, k
    assert tot["first_over"] == ref.NONE and tot["max_err_index"] == 256      # the lowest index that attains max_err = 0


def test_absolute_bound(sim, data):
    rec, dec = data["eps"]
    eps = float(EPS)
    tot, _ = check(sim, rec, data["w"], dec, eps_abs=eps)
    assert tot["n_over_abs"] == 0 and tot["max_err"] <= eps and tot["first_over"] == ref.NONE
    tot, want = check(sim, rec, data["w"], dec, eps_abs=eps / 2)
    assert tot["n_over_abs"] == want["n_over_abs"] > 0 and tot["first_over"] == want["first_over"] != ref.NONE
    offs = _offsets(rec)
    for off in (-1.0, -1e-300, math.nan, -math.inf):                            # negative and NaN bounds switch the checks off
        acc = new_acc(3)
        assert step(sim.lib, sim.ctx, rec[offs[2]:], data["w"], N, acc, first_chunk=2, eps_abs=off, eps_rel=off) == 0
        t = records(acc, 3)[2]
        assert t["n_diff"] > 0 and t["n_over_abs"] == t["n_over_rel"] == 0 and t["first_over"] == ref.NONE


def test_cuts_do_not_change_the_bits(sim, data):
    rec, _ = data["b8"]
    kw = dict(eps_abs=1e-4, eps_rel=2.0 ** -17)
    base = compare(sim, rec, data["w"], **kw)[2]                              # the module's context: batches of two chunks
    one, three = util.SimCodec(sim.lib, max_batch_chunks=1), util.SimCodec(sim.lib, max_batch_chunks=3)
    for ctx, pieces in ((one, None), (three, None), (sim, [(0, 1), (1, 1), (2, 1)]), (three, [(2, 1), (1, 1), (0, 1)]), (sim, [(1, 2), (0, 1)])):
        assert compare(sim, rec, data["w"], pieces=pieces, ctx=ctx, **kw)[2] == base, pieces
    sim.lib.mrcz_destroy(one.ctx)
    sim.lib.mrcz_destroy(three.ctx)


def test_an_original_that_is_not_what_was_compressed(sim, data):
    rec, dec = data["b8"]
    w = data["w"].copy()
    f = w.view(np.float32)
    nan_at = int(np.flatnonzero(np.isnan(f) & (np.arange(N) > CHK))[0])       # a NaN of chunk 1 becomes a number
    num_at = int(np.flatnonzero(np.isfinite(f) & (np.arange(N) > 2 * CHK))[5])  # a number of chunk 2 becomes Inf
    w[100] ^= 0x00010000                                                       # one header word flipped
    f[nan_at] = 3.0
    f[num_at] = np.inf
    # a tie for the maximum error at two indices of chunk 0: the original 1024 below the decoded word at both, exactly
    d = dec.view(np.float32)
    ties = np.flatnonzero((np.abs(d) >= 1) & (np.abs(d) < 100) & (np.arange(N) > 5000) & (np.arange(N) < CHK))[[700, 20]]
    for i in ties:
        f[i] = d[i] - np.float32(1024.0)
        assert float(d[i]) - float(f[i]) == 1024.0
    tot, want = check(sim, rec, w, dec, eps_abs=-1.0)
    assert tot["n_header_diff"] == 1 and tot["n_special_diff"] == 2 and tot["first_over"] == nan_at
    assert tot["max_err"] == 1024.0 and tot["max_err_index"] == int(ties.min())


def test_int_mode(sim, data):
    rec, dec = data["int"]
    tot, _ = check(sim, rec, data["w"], dec, int_mode=True, eps_abs=0.5)
    assert tot["n_diff"] > 0 and tot["n_header_diff"] == 0


def test_records_of_a_later_chunk_and_a_short_last_chunk(sim, data):
    rec, dec = data["b8"]
    offs = _offsets(rec)
    want = ref.fold_chunks(data["w"], dec, CHK, 1e-4, None)
    acc = new_acc(3)
    assert step(sim.lib, sim.ctx, rec[offs[1]:], data["w"], N, acc, first_chunk=1, eps_abs=1e-4) == 0
    got = records(acc, 3)
    ref.assert_matches(got[1], want[1], "chunk 1")
    ref.assert_matches(got[2], want[2], "chunk 2")                           # N - 2 CHK = 524564 words: a short last chunk
    assert got[2]["n"] == N - 2 * CHK
    assert acc[: ctypes.sizeof(ref.Compare)].tobytes() == bytes([GARBAGE]) * ctypes.sizeof(ref.Compare)   # chunk 0's record is untouched
    ref.assert_matches(finish(sim.lib, sim.ctx, acc, 1, 2), ref.total(want[1:]), "chunks 1 and 2")


@pytest.mark.parametrize("n", [1, 100, 255, 256, 257, 259, 4099])
def test_small_files(sim, oracle, n):
    w = util.gauss_words(n, seed=n, header=False)
    z = oracle.compress(w.tobytes(), 10)
    dec = np.frombuffer(oracle.uncompress(z), np.uint32)
    other = w.copy()
    other[::7] ^= 0x00000400                       # differences in header and data words alike
    tot, _ = check(sim, z[17:], other, dec, nfl=n, eps_abs=1e-3, eps_rel=1e-4)
    assert tot["n"] == max(n - 256, 0)
    if n <= 256:
        assert tot["n_finite"] == 0 and tot["max_err_index"] == ref.NONE and tot["orig_min"] == math.inf and tot["orig_max"] == -math.inf
        assert tot["n_header_diff"] == len(range(0, n, 7))


def test_lz4_fixtures(sim):
    from golden.make_golden import lz4_cases
    try:
        for name, (raw, _) in lz4_cases().items():
            z = open(os.path.join(util.GOLDEN, name + ".zip"), "rb").read()
            fsz, chk = struct.unpack("<QI", z[:12])
            assert chk == CHK
            nfl = fsz // 4
            assert sim.set_ztypes(struct.unpack("<4b", z[13:17])) == 0
            dec = np.frombuffer(raw[: nfl * 4], np.uint32)
            tot, _ = check(sim, z[17:], dec, dec, nfl=nfl, eps_abs=0.0)
            assert tot["n_diff"] == 0 and tot["max_err"] == 0
            other = dec.copy()
            other[300::11] += 3
            tot, _ = check(sim, z[17:], other, dec, nfl=nfl, eps_abs=1e-6)
            assert tot["n_diff"] == len(range(300, nfl, 11))
    finally:
        assert sim.set_ztypes((0, 0, 0, 0)) == 0


def test_rejected_arguments(sim, data):
    rec, dec = data["b8"]
    offs = _offsets(rec)
    lib, ctx, w = sim.lib, sim.ctx, data["w"]
    acc = new_acc(3)
    clean = acc.tobytes()
    for null in ("rec", "orig", "acc"):
        assert step(lib, ctx, rec, w, N, acc, null=(null,)) == EINVAL
    assert lib.mrcz_uncompress_compare(None, None, 0, N, CHK, 0, 0, None, 0.0, 0.0, 0, acc.ctypes.data) == EINVAL
    assert step(lib, ctx, rec, w, N, acc, first_chunk=1, nchunks=3) == EINVAL       # past the file's three chunks
    assert step(lib, ctx, rec, w, N, acc, first_chunk=4, nchunks=0) == EINVAL
    assert step(lib, ctx, rec, w, N, acc, chk=0) == EFORMAT
    assert step(lib, ctx, rec, w, N, acc, chk=CHK + 1) == EFORMAT
    assert step(lib, ctx, rec, w, N, acc, first_chunk=3, nchunks=0) == 0             # nothing to do ...
    assert step(lib, ctx, rec, w, N, acc, first_chunk=0, nchunks=0, null=("rec", "orig")) == 0
    assert acc.tobytes() == clean                                                    # ... and nothing touched
    t = ref.Compare()
    assert lib.mrcz_compare_finish(ctx, None, 0, 3, ctypes.byref(t)) == EINVAL
    assert lib.mrcz_compare_finish(ctx, acc.ctypes.data, 0, 3, None) == EINVAL
    assert lib.mrcz_compare_finish(None, acc.ctypes.data, 0, 3, ctypes.byref(t)) == EINVAL
    assert lib.mrcz_compare_finish(ctx, acc.ctypes.data, 0, 0, ctypes.byref(t)) == 0 and t.n == 0 and t.first_over == ref.NONE
    o = util.aligned_empty(4 * N + 64)                                               # a misaligned original
    r = util.aligned_empty(len(rec) + 8)
    r[: len(rec)] = np.frombuffer(rec, np.uint8)
    assert lib.mrcz_uncompress_compare(ctx, r.ctypes.data, len(rec), N, CHK, 0, 3, o.ctypes.data + 4, 0.0, 0.0, 0, acc.ctypes.data) == EINVAL
    assert step(lib, ctx, rec[: offs[2]], w, N, acc) == EFORMAT                      # chunk 2's record is missing
    assert step(lib, ctx, rec[: offs[1] - 5], w, N, acc, nchunks=1) == EFORMAT       # chunk 0's record is cut
    assert step(lib, ctx, rec[: offs[2] + 9], w, N, acc) == EFORMAT                  # cut inside chunk 2's header
    bad = bytearray(rec)
    bad[offs[1] + 16 + 40: offs[1] + 16 + 60] = b"\xff" * 20                        # a damaged deflate stream
    rc = step(lib, ctx, bytes(bad), w, N, acc)
    assert rc in (0, EFORMAT)                                                        # decoded to other words, or refused
    check(sim, rec, w, dec)                                                          # the context still works after refusals


ASAN_SCRIPT = r'''
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import util, compare_ref as ref
import test_sim_compare as t
lib = ctypes.CDLL(os.environ["SIM_ASAN"])
sim = util.SimCodec(lib)
t.bind(lib)
oracle = util.load_oracle()
n = 70001                                                # one short chunk, no multiple of four (the emulator is slow under the sanitizer)
w = util.gauss_words(n, seed=8)
z = oracle.compress(w.tobytes(), 8)
dec = np.frombuffer(oracle.uncompress(z), np.uint32)
rec = z[17:]
offs = t._offsets(rec, n)
def run(rec_bytes, **kw):
    # the records in a buffer of exactly their length and the original in one of exactly its words: a read past either is caught
    r = np.frombuffer(bytes(rec_bytes), np.uint8).copy() if len(rec_bytes) else np.zeros(1, np.uint8)
    o = util.aligned_empty(4 * n).view(np.uint32); o[:] = w
    acc = t.new_acc(1)
    rc = lib.mrcz_uncompress_compare(sim.ctx, r.ctypes.data, len(rec_bytes), n, util.CHUNK, 0, 1, o.ctypes.data, 1e-4, -1.0, 0, acc.ctypes.data)
    return rc, acc
rc, acc = run(rec)
assert rc == 0
for c, (g, want) in enumerate(zip(t.records(acc, 1), ref.fold_chunks(w, dec, util.CHUNK, 1e-4, None))):
    ref.assert_matches(g, want, c)
for cut in (offs[1] - 1, offs[1] - 4097, 16, 15, 0):
    rc, _ = run(rec[:cut])
    assert rc == -4, (cut, rc)
print("COMPARE-ASAN-OK")
'''


def test_records_cut_short_never_read_past_len_under_asan(tmp_path, tmp_path_factory):
    from test_sim_fuzz import _asan_build
    so, asan_rt = _asan_build(tmp_path_factory)
    script = tmp_path / "compare_asan.py"
    script.write_text(ASAN_SCRIPT)
    env = dict(os.environ, REPO=util.ROOT, SIM_ASAN=so, LD_PRELOAD=asan_rt,
               ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1")
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert r.returncode == 0 and "COMPARE-ASAN-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr
