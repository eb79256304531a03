"""CPU-only: top-planes decode (mrcz_record_top_span, mrcz_uncompress_top, k_parse_top, k_merge_top) on the SIMT emulator build of
the product sources.  The three-chunk volume of tests/test_sim_binned.py in the -b 8, -b 0 and absolute-bound containers, all
written by the CPU oracle.  Every comparison is bit equality with oracle.uncompress(container) & mask(keep), computed with numpy:
keep 2 and 3, 32- and 16-bit output, ordinary and thinned records, any cut into batches and calls, ragged last chunks, the LZ4
fixtures and a general-distance container through the fallback kernels, dropped payloads overwritten with 0xFF (never read), a
damaged kept stream (MRCZ_EFORMAT) and every refused argument."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

import top_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero
from test_sim_binned import N, _volume
from top_ref import COMBOS, EFORMAT, EINVAL, F32, THINNED, U16

CHK = util.CHUNK
EPS = f32_toward_zero(0.01)
GARBAGE = 0xA5


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    ref.bind(s.lib)
    return s


@pytest.fixture(scope="module")
def data(oracle):
    w = _volume()
    out = {"w": w}
    for tag, z in (("b8", oracle.compress(w.tobytes(), 8)), ("b0", oracle.compress(w.tobytes(), 0)), ("eps", oracle.compress(abs_round(w, EPS).tobytes(), 0))):
        out[tag] = (z[17:], np.frombuffer(oracle.uncompress(z), np.uint32))
    return out


def top(sim, rec, nfl, keep=2, u16=False, thinned=False, first_chunk=0, nchunks=None, chk=CHK, ctx=None, out=None, null=(), flags=None, misalign=()):
    """one mrcz_uncompress_top over `rec` = the records of chunks [first_chunk, first_chunk + nchunks) in a buffer of their length:
    (rc, the output elements, consumed); elements the call does not own keep GARBAGE"""
    if nchunks is None:
        nchunks = (nfl + max(chk, 1) - 1) // max(chk, 1) - first_chunk
    nel = max(min(nchunks * chk, nfl - first_chunk * chk), 0)
    r = util.aligned_empty(len(rec) + 16)
    r[: len(rec)] = np.frombuffer(bytes(rec), np.uint8)
    own = out is None
    if own:
        out = util.aligned_empty((2 if u16 else 4) * (nel + 8))
        out[:] = GARBAGE
    cons = ctypes.c_uint64(77)
    fl = ((U16 if u16 else F32) | (THINNED if thinned else 0)) if flags is None else flags
    rp = None if "rec" in null else r.ctypes.data + (1 if "rec" in misalign else 0)
    op = None if "out" in null else out.ctypes.data + (4 if "out" in misalign else 0)
    rc = sim.lib.mrcz_uncompress_top((ctx or sim).ctx if "ctx" not in null else None, rp, len(rec), nfl, chk, first_chunk, nchunks, keep, fl, op, ctypes.byref(cons))
    el = out.view(np.uint16 if u16 else np.uint32)
    assert not own or np.all(out[(2 if u16 else 4) * nel:] == GARBAGE)         # nothing behind the call's own elements is written
    return rc, el[:nel].copy(), cons.value


def check(sim, rec, full, keep, u16, thinned, nfl=None, **kw):
    nfl = len(full) if nfl is None else nfl
    src = ref.thin(sim.lib, rec, nfl, keep, chk=kw.get("chk", CHK)) if thinned else rec
    rc, got, cons = top(sim, src, nfl, keep, u16, thinned, **kw)
    assert rc == 0, sim.lib.mrcz_last_error((kw.get("ctx") or sim).ctx)
    assert cons == len(src)
    assert np.array_equal(got, ref.expected(full, keep, u16)), (keep, u16, thinned)


@pytest.mark.parametrize("keep,u16", COMBOS)
@pytest.mark.parametrize("mode", ["b8", "b0", "eps"])
def test_every_word_equals_the_full_decode_under_the_mask(sim, data, mode, keep, u16):
    rec, full = data[mode]
    for thinned in (False, True):
        check(sim, rec, full, keep, u16, thinned)
        assert int(sim.lib.mrcz_debug_fallbacks(sim.ctx)) == 0                # oracle-written: as for the full decode
        assert int(sim.lib.mrcz_debug_chain_fallbacks(sim.ctx)) == 0


def test_thinned_records_are_the_header_and_the_tail_of_every_record(sim, data):
    for mode in ("b8", "b0"):
        rec, _ = data[mode]
        offs = ref.offsets(rec, N)
        for keep in (2, 3):
            th = ref.thin(sim.lib, rec, N, keep)
            at = 0
            for c in range(3):
                ln = ref.lengths(rec[offs[c]: offs[c] + 16])
                kept = sum(ln[4 - keep:])
                assert th[at: at + 16] == rec[offs[c]: offs[c] + 16]
                assert th[at + 16: at + 16 + kept] == rec[offs[c + 1] - kept: offs[c + 1]]
                at += 16 + kept
            assert at == len(th) < len(rec)
            assert len(rec) - len(th) == sum(sum(ref.lengths(rec[o: o + 16])[: 4 - keep]) for o in offs[:3])


def test_cuts_do_not_change_the_bits(sim, data):
    rec, full = data["b8"]
    offs = ref.offsets(rec, N)
    ctxs = {m: util.SimCodec(sim.lib, max_batch_chunks=m) for m in (1, 64)}   # the module's context: batches of two chunks
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            for m in (1, 64):
                check(sim, rec, full, keep, u16, thinned, ctx=ctxs[m])
            # one call per chunk, in reverse order, into one output buffer
            esz = 2 if u16 else 4
            out = util.aligned_empty(esz * (N + 8))
            out[:] = GARBAGE
            for c in (2, 1, 0):
                piece = rec[offs[c]: offs[c + 1]]
                src = ref.thin(sim.lib, piece, N, keep, first_chunk=c) if thinned else piece
                rc, got, cons = top(ctxs[1], src, N, keep, u16, thinned, first_chunk=c, nchunks=1, out=out[esz * c * CHK:])
                assert rc == 0 and cons == len(src)
            got = out.view(np.uint16 if u16 else np.uint32)[:N]
            assert np.array_equal(got, ref.expected(full, keep, u16)), (keep, u16, thinned)
    rc, got, _ = top(sim, rec[offs[1]:], N, 2, True, first_chunk=1)            # the records of chunks 1 and 2 alone
    assert rc == 0 and np.array_equal(got, ref.expected(full[CHK:], 2, True))
    for c in ctxs.values():
        sim.lib.mrcz_destroy(c.ctx)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 9, 255, 257, 4099, 16385, 16386, 16387, 131075])
def test_ragged_last_chunks(sim, oracle, n):
    """file lengths that are no multiple of four or eight words: the tail goes out element by element"""
    w = util.gauss_words(n, seed=n, header=False)
    z = oracle.compress(w.tobytes(), 10)
    full = np.frombuffer(oracle.uncompress(z), np.uint32)
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            check(sim, z[17:], full, keep, u16, thinned)


@pytest.mark.parametrize("chk,n", [(4099, 3 * 4099 + 17), (4096, 5 * 4096), (300, 300 * 4 + 255), (1, 7)])
def test_a_chunk_size_below_the_default(sim, oracle, chk, n):
    """chunk bases that are no multiple of four (or eight) words: stores of 16 bytes only where the address allows"""
    w = util.gauss_words(n, seed=chk, header=False)
    b = w.view(np.uint8).reshape(-1, 4)
    z = bytearray(struct.pack("<QIb4b", 4 * n, chk, 0, 0, 0, 0, 0))
    for c0 in range(0, n, chk):
        planes = [np.ascontiguousarray(b[c0: c0 + chk, j]) for j in range(4)]
        zs = [util.python_zlib_stream(p) for p in planes]
        z += util.chunk_record(planes, [s if len(p) > len(s) + 4 else None for p, s in zip(planes, zs)])
    full = np.frombuffer(oracle.uncompress(bytes(z)), np.uint32)
    assert full.tobytes() == w.tobytes()
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            check(sim, bytes(z[17:]), full, keep, u16, thinned, chk=chk)


def test_lz4_fixtures_and_general_distances_take_the_fallback_kernels(sim, oracle):
    from golden.make_golden import lz4_cases
    try:
        for name, (raw, _) in lz4_cases().items():
            z = open(os.path.join(util.GOLDEN, name + ".zip"), "rb").read()
            fsz, chk = struct.unpack("<QI", z[:12])
            assert chk == CHK
            assert sim.set_ztypes(struct.unpack("<4b", z[13:17])) == 0
            full = np.frombuffer(raw[: fsz // 4 * 4], np.uint32)
            for keep, u16 in COMBOS:
                for thinned in (False, True):
                    check(sim, z[17:], full, keep, u16, thinned)
    finally:
        assert sim.set_ztypes((0, 0, 0, 0)) == 0
    # planes deflated by the system zlib with its default strategy: matches at general distances go to the sequential decoder
    w = util.poisson_words(40000, seed=9)
    z = util.container_from_python_zlib(w, zlib.Z_DEFAULT_STRATEGY)
    full = np.frombuffer(oracle.uncompress(z), np.uint32)
    assert full.tobytes() == w.tobytes()
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            check(sim, z[17:], full, keep, u16, thinned)
            assert int(sim.lib.mrcz_debug_fallbacks(sim.ctx)) > 0
    for name in ("words5000_tail3_b8", "gauss20000_b12", "poisson40000_b0", "runs9000_b0", "words100_b0"):   # the reference's own containers
        z = open(os.path.join(util.GOLDEN, name + ".zip"), "rb").read()
        full = np.frombuffer(oracle.uncompress(z), np.uint32)
        for keep, u16 in COMBOS:
            check(sim, z[17:], full, keep, u16, True)


@pytest.mark.parametrize("mode,keep", [("b0", 2), ("b8", 2), ("b8", 3)])
def test_dropped_planes_are_never_read(sim, data, oracle, mode, keep):
    """every payload byte of the dropped planes is 0xFF, the headers stand: exact and MRCZ_OK; the full decode may fail"""
    rec, full = data[mode]
    bad = ref.poison(rec, N, keep)
    assert bad != rec and len(bad) == len(rec)
    for u16 in ((True, False) if keep == 2 else (False,)):
        check(sim, bad, full, keep, u16, False)
        assert int(sim.lib.mrcz_debug_fallbacks(sim.ctx)) == 0 and int(sim.lib.mrcz_debug_chain_fallbacks(sim.ctx)) == 0
    try:
        dec = sim.uncompress_records(bad, N)
        assert not np.array_equal(dec, full)                                  # the premise: the low planes really are gone
    except RuntimeError:
        pass


def test_a_damaged_kept_stream_is_eformat(sim, oracle):
    n = 70001
    w = util.gauss_words(n, seed=3)
    rec = bytearray(oracle.compress(w.tobytes(), 8)[17:])
    ln = np.frombuffer(bytes(rec[:16]), "<u4")
    assert not int(ln[3]) & 0x80000000, "plane 3 of Gaussian words deflates"
    p3 = 16 + sum(ref.lengths(rec[:16])[:3])
    rec[p3] = (rec[p3] & 0xF8) | 0x06                                          # BFINAL 0, BTYPE 3: no such block
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            src = ref.thin(sim.lib, bytes(rec), n, keep) if thinned else bytes(rec)
            assert top(sim, src, n, keep, u16, thinned)[0] == EFORMAT
    # the same byte in a DROPPED plane is nobody's business
    w8 = np.frombuffer(oracle.uncompress(oracle.compress(w.tobytes(), 8)), np.uint32)
    rec = bytearray(oracle.compress(w.tobytes(), 8)[17:])
    assert not int(ln[0]) & 0x80000000
    rec[16] = (rec[16] & 0xF8) | 0x06
    check(sim, bytes(rec), w8, 2, True, False)
    assert top(sim, bytes(rec), n, 3)[0] == 0                                  # plane 0 is dropped by keep 3 as well


def test_record_top_span(sim, data):
    lib = sim.lib
    for mode in ("b8", "b0", "eps"):
        rec, _ = data[mode]
        offs = ref.offsets(rec, N)
        for c in range(3):
            h = rec[offs[c]: offs[c] + 16]
            n = min(CHK, N - c * CHK)
            ln = ref.lengths(h)
            assert ref.span(lib, h, n, 2) == (0, 16 + ln[0] + ln[1], ln[2] + ln[3])
            assert ref.span(lib, h, n, 3) == (0, 16 + ln[0], ln[1] + ln[2] + ln[3])
            size = ctypes.c_uint64()
            lib.mrcz_record_size.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
            assert lib.mrcz_record_size(h, n, ctypes.byref(size)) == 0 and size.value == sum(ref.span(lib, h, n, 2)[1:])
    h = struct.pack("<4I", 10, 20, 30, 40)
    assert ref.span(lib, h, 1000, 2) == (0, 46, 70)
    for keep in (-1, 0, 1, 4, 5):
        assert ref.span(lib, h, 1000, keep)[0] == EINVAL
    sk, by = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.mrcz_record_top_span(None, 1000, 2, ctypes.byref(sk), ctypes.byref(by)) == EINVAL
    assert lib.mrcz_record_top_span(h, 1000, 2, None, ctypes.byref(by)) == EINVAL
    assert lib.mrcz_record_top_span(h, 1000, 2, ctypes.byref(sk), None) == EINVAL
    too_long = CHK + (CHK >> 3) + 1025
    for j in range(4):                                                        # impossible lengths, in a kept or a dropped plane
        ln = [10, 20, 30, 40]
        ln[j] = 999 | 0x80000000                                              # a RAW plane shorter than the chunk
        assert ref.span(lib, struct.pack("<4I", *ln), 1000, 2)[0] == EFORMAT
        ln[j] = too_long                                                      # a deflate stream longer than any plane's can be
        assert ref.span(lib, struct.pack("<4I", *ln), 1000, 3)[0] == EFORMAT
        ln[j] = 1000 | 0x80000000
        assert ref.span(lib, struct.pack("<4I", *ln), 1000, 2)[0] == 0


def test_rejected_arguments(sim, data):
    rec, full = data["b8"]
    offs = ref.offsets(rec, N)
    for kw in (dict(keep=1), dict(keep=4), dict(keep=0), dict(keep=-2), dict(keep=3, u16=True), dict(flags=2), dict(flags=8), dict(flags=U16 | 16),
               dict(flags=-1), dict(null=("out",)), dict(null=("rec",)), dict(null=("ctx",)), dict(misalign=("out",)), dict(misalign=("rec",)),
               dict(first_chunk=1, nchunks=3), dict(first_chunk=4, nchunks=0), dict(first_chunk=0, nchunks=4)):
        rc, got, cons = top(sim, rec, N, **{"nchunks": 3, **kw})
        assert rc == EINVAL, kw
        assert np.all(got.view(np.uint8) == GARBAGE), kw
    assert top(sim, rec, N, chk=0)[0] == EFORMAT
    assert top(sim, rec, N, chk=CHK + 1)[0] == EFORMAT
    for kw in (dict(first_chunk=3, nchunks=0), dict(first_chunk=0, nchunks=0), dict(first_chunk=0, nchunks=0, null=("rec",))):
        rc, got, cons = top(sim, rec, N, **kw)                                # nothing to do ...
        assert rc == 0 and cons == 0 and len(got) == 0                        # ... and nothing touched (top() checks the buffer)
    for keep in (2, 3):
        th = ref.thin(sim.lib, rec, N, keep)
        assert top(sim, rec[: offs[2]], N, keep)[0] == EFORMAT                # chunk 2's record is missing
        assert top(sim, rec[: offs[2] + 9], N, keep)[0] == EFORMAT            # cut inside chunk 2's header
        assert top(sim, rec[: len(rec) - 3], N, keep)[0] == EFORMAT           # cut inside the last kept payload
        assert top(sim, th[: len(th) - 3], N, keep, thinned=True)[0] == EFORMAT
        assert top(sim, th[: 16 + 5], N, keep, thinned=True)[0] == EFORMAT
    bad = bytearray(rec)
    bad[offs[1] + 3] |= 0x80                                                  # chunk 1, plane 0 (dropped): RAW with a length below the chunk's
    assert top(sim, bytes(bad), N, 2)[0] == EFORMAT                           # the header is read whole, and it is impossible
    check(sim, rec, full, 2, True, False)                                     # the context still works after refusals
