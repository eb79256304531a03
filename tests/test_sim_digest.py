"""CPU-only: digest decode (mrcz_uncompress_digest, mrcz_digest_words, k_crc_fold, k_crc_chunk, mrcz_digest_finish) on the SIMT
emulator build of the product sources.  The three-chunk volume of tests/test_sim_binned.py in the four containers of
tests/test_sim_compare.py (-b 8, -b 0, absolute bound, -s int), all written by the CPU oracle.  The yardstick is Python's
zlib.crc32 over the oracle's decode; every comparison is equality of 32-bit values."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import crc_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero
from crc_ref import ABS, EFORMAT, EINVAL, INT8, MASK, NONE
from test_sim_binned import N, _offsets, _volume

CHK = util.CHUNK
EPS = f32_toward_zero(0.01)
MODES = {"b8": (MASK, 8, 0.0, False), "b0": (MASK, 0, 0.0, False), "eps": (ABS, 0, float(EPS), False), "int": (INT8, 0, 0.0, True)}


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    ref.bind(s.lib)
    return s


@pytest.fixture(scope="module")
def data(oracle):
    w = _volume()
    rounded = abs_round(w, EPS)
    z8, z0, ze, zi = oracle.compress(w.tobytes(), 8), oracle.compress(w.tobytes(), 0), oracle.compress(rounded.tobytes(), 0), oracle.compress_int(w.tobytes())
    dec = lambda z, **kw: np.frombuffer(oracle.uncompress(z, **kw), np.uint32)
    return {"w": w, "b8": (z8[17:], dec(z8)), "b0": (z0[17:], dec(z0)), "eps": (ze[17:], dec(ze)), "int": (zi[17:], dec(zi, int_mode=True))}


def step(lib, ctx, rec, nfl, acc, first_chunk=0, nchunks=None, int_mode=False, chk=CHK, null=()):
    """one mrcz_uncompress_digest: rec = the records of chunks [first_chunk, first_chunk + nchunks), in a buffer of their length"""
    if nchunks is None:
        nchunks = (nfl + max(chk, 1) - 1) // max(chk, 1) - first_chunk
    r = util.aligned_empty(len(rec) + 8)
    r[: len(rec)] = np.frombuffer(bytes(rec), np.uint8)
    return lib.mrcz_uncompress_digest(ctx, None if "rec" in null else r.ctypes.data, len(rec), nfl, chk, first_chunk, nchunks,
                                      1 if int_mode else 0, None if "acc" in null else acc.ctypes.data)


def digest(sim, rec, nfl=N, pieces=None, ctx=None, chk=CHK, offs=None, **kw):
    """(chunk records, total, raw accumulator bytes) of a file digested in pieces [(first_chunk, nchunks)] (default: one call)"""
    ctx = ctx or sim
    nch = (nfl + chk - 1) // chk
    offs = offs or _offsets(rec, nfl)
    acc = ref.new_acc(nch)
    for k, n in pieces or [(0, nch)]:
        rc = step(sim.lib, ctx.ctx, rec[offs[k]: offs[k + n]], nfl, acc, k, n, chk=chk, **kw)
        assert rc == 0, sim.lib.mrcz_last_error(ctx.ctx)
    return ref.records(acc, nch), ref.finish(sim.lib, ctx.ctx, acc, 0, nch), acc[: nch * 16].tobytes()


def digest_words(sim, words, xform=NONE, bits=0, eps=0.0, first_chunk=0, chk=CHK, nfile=None, ctx=None):
    """chunk records of mrcz_digest_words over `words` = the file's words from chunk first_chunk on"""
    ctx = ctx or sim
    n = len(words)
    nch = first_chunk + (n + chk - 1) // chk
    d = util.aligned_empty(4 * max(n, 4)).view(np.uint32)
    d[:n] = words
    acc = ref.new_acc(nch)
    rc = sim.lib.mrcz_digest_words(ctx.ctx, d.ctypes.data, n, first_chunk, chk, xform, bits, eps, acc.ctypes.data)
    assert rc == 0, sim.lib.mrcz_last_error(ctx.ctx)
    return ref.records(acc, nch, first_chunk), acc


@pytest.mark.parametrize("mode", ["b8", "b0", "eps", "int"])
def test_every_chunk_and_the_file_equal_zlib_crc32_of_the_oracle_decode(sim, data, mode):
    rec, dec = data[mode]
    got, tot, _ = digest(sim, rec, int_mode=MODES[mode][3])
    assert got == ref.chunk_crcs(dec)
    assert tot == (ref.file_crc(dec), 4 * N)


@pytest.mark.parametrize("mode", ["b8", "b0", "eps", "int"])
def test_the_expected_decode_of_the_original_equals_the_digest_of_the_container(sim, data, mode):
    rec, dec = data[mode]
    xform, bits, eps, int_mode = MODES[mode]
    got, acc = digest_words(sim, data["w"], xform, bits, eps)
    assert got == ref.chunk_crcs(dec)
    assert got == digest(sim, rec, int_mode=int_mode)[0]
    assert ref.finish(sim.lib, sim.ctx, acc, 0, 3) == (ref.file_crc(dec), 4 * N)


def test_digest_words_none_is_the_crc32_of_a_plain_file(sim, data):
    w = data["w"]
    got, acc = digest_words(sim, w)
    assert got == ref.chunk_crcs(w)
    assert ref.finish(sim.lib, sim.ctx, acc, 0, 3) == (zlib.crc32(w.tobytes()), 4 * N)
    # the words of chunks 1 and 2 alone: the records of a later call of a pipeline
    later, acc2 = digest_words(sim, w[CHK:], MASK, 8, first_chunk=1)
    assert later == ref.chunk_crcs(util.erase_expected(w, 8))[1:]
    assert acc2[:16].tobytes() == bytes([ref.GARBAGE]) * 16                     # chunk 0's record is untouched


def test_cuts_do_not_change_the_bits(sim, data):
    rec, dec = data["b8"]
    base = digest(sim, rec)[2]                                                # the module's context: batches of two chunks
    ctxs = {m: util.SimCodec(sim.lib, max_batch_chunks=m) for m in (1, 3, 64)}
    cases = [(ctxs[1], None), (ctxs[3], None), (ctxs[64], None), (sim, [(0, 1), (1, 1), (2, 1)]), (ctxs[3], [(2, 1), (1, 1), (0, 1)]), (sim, [(1, 2), (0, 1)])]
    for ctx, pieces in cases:
        assert digest(sim, rec, pieces=pieces, ctx=ctx)[2] == base, pieces
    for m in (1, 3, 64):                                                      # and the compress side, cut into other batches
        assert digest_words(sim, data["w"], MASK, 8, ctx=ctxs[m])[1][:48].tobytes() == base
        sim.lib.mrcz_destroy(ctxs[m].ctx)


def test_records_of_a_later_chunk_and_a_short_last_chunk(sim, data):
    rec, dec = data["b8"]
    offs = _offsets(rec)
    want = ref.chunk_crcs(dec)
    acc = ref.new_acc(3)
    assert step(sim.lib, sim.ctx, rec[offs[1]:], N, acc, first_chunk=1) == 0
    assert ref.records(acc, 3, 1) == want[1:] and want[2][1] == 4 * (N - 2 * CHK)
    assert acc[:16].tobytes() == bytes([ref.GARBAGE]) * 16                      # chunk 0's record is untouched
    both = zlib.crc32(dec[CHK:].tobytes())
    assert ref.finish(sim.lib, sim.ctx, acc, 1, 2) == (both, 4 * (N - CHK))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 258, 259, 4099, 16385, 16386, 16387, 131075])
def test_small_files_and_last_chunks_of_4k_plus_1_to_3_words(sim, oracle, n):
    w = util.gauss_words(n, seed=n, header=False)
    z = oracle.compress(w.tobytes(), 10)
    dec = np.frombuffer(oracle.uncompress(z), np.uint32)
    got, tot, _ = digest(sim, z[17:], nfl=n)
    assert got == [(zlib.crc32(dec.tobytes()), 4 * n)] and tot == got[0]
    for xform, bits, eps, exp in ((MASK, 10, 0.0, dec), (NONE, 0, 0.0, w), (ABS, 0, float(EPS), abs_round(w, EPS))):
        assert digest_words(sim, w, xform, bits, eps)[0] == [(zlib.crc32(exp.tobytes()), 4 * n)]
    assert digest_words(sim, w, INT8)[0] == [(zlib.crc32(np.frombuffer(oracle.uncompress(oracle.compress_int(w.tobytes()), int_mode=True), np.uint32).tobytes()), 4 * n)]


@pytest.mark.parametrize("chk,n", [(4099, 3 * 4099 + 17), (4096, 5 * 4096), (300, 300 * 4 + 255), (1, 7), (CHK - 1, CHK + 5)])
def test_a_chunk_size_below_the_default(sim, oracle, chk, n):
    """containers whose header names a smaller chunk size (planes deflated by the system zlib): chunk bases that are no multiple
    of four words take the unaligned loads"""
    w = util.gauss_words(n, seed=chk, header=False)
    b = w.view(np.uint8).reshape(-1, 4)
    z = bytearray(struct.pack("<QIb4b", 4 * n, chk, 0, 0, 0, 0, 0))
    offs = []
    for c0 in range(0, n, chk):
        planes = [np.ascontiguousarray(b[c0: c0 + chk, j]) for j in range(4)]
        zs = [util.python_zlib_stream(p) for p in planes]
        offs.append(len(z) - 17)
        z += util.chunk_record(planes, [s if len(p) > len(s) + 4 else None for p, s in zip(planes, zs)])
    offs.append(len(z) - 17)
    dec = np.frombuffer(oracle.uncompress(bytes(z)), np.uint32)
    assert dec.tobytes() == w.tobytes()
    got, tot, _ = digest(sim, bytes(z[17:]), nfl=n, chk=chk, offs=offs)
    assert got == ref.chunk_crcs(dec, chk) and tot == (zlib.crc32(dec.tobytes()), 4 * n)
    assert digest_words(sim, w, MASK, 8, chk=chk)[0] == ref.chunk_crcs(util.erase_expected(w, 8), chk)
    if len(offs) > 2:                                                         # a later piece, in reverse order
        assert digest(sim, bytes(z[17:]), nfl=n, chk=chk, offs=offs, pieces=[(1, len(offs) - 2), (0, 1)])[0] == got


def test_one_flipped_bit_in_a_raw_plane_decodes_ok_and_changes_only_its_chunk(sim, oracle):
    """the premise of the feature: the container has no checksum, so the damaged file decodes with MRCZ_OK"""
    n = 2 * CHK + 70001
    w = util.gauss_words(n, seed=77)
    z = oracle.compress(w.tobytes(), 8)
    rec = bytearray(z[17:])
    offs = _offsets(bytes(rec), n)
    good = digest(sim, bytes(rec), nfl=n)
    assert good[0] == ref.chunk_crcs(np.frombuffer(oracle.uncompress(z), np.uint32))
    span = ref.raw_payload_span(bytes(rec), offs, 1, CHK)
    assert span is not None, "a -b 8 container of Gaussian words has a RAW plane"
    rec[span[1] + 12345] ^= 0x10
    acc = ref.new_acc(3)
    assert step(sim.lib, sim.ctx, bytes(rec), n, acc) == 0                        # MRCZ_OK: nobody is told
    bad = ref.records(acc, 3)
    dec_bad = np.frombuffer(oracle.uncompress(z[:17] + bytes(rec)), np.uint32)
    assert bad == ref.chunk_crcs(dec_bad)
    assert bad[1] != good[0][1] and bad[0] == good[0][0] and bad[2] == good[0][2]
    assert ref.finish(sim.lib, sim.ctx, acc, 0, 3)[0] != good[1][0]


def test_one_flipped_byte_in_a_stored_block(sim, oracle):
    """the same for the stored data of a stored deflate block (planes written by the system zlib at level 0)"""
    n = 70001
    w = util.gauss_words(n, seed=5)
    b = w.view(np.uint8).reshape(-1, 4)
    planes = [np.ascontiguousarray(b[:, j]) for j in range(4)]
    zs = [util.python_zlib_stream(p, level=0) for p in planes]                # stored blocks: 5-byte header, then the bytes
    z = util.file_header(4 * n) + util.chunk_record(planes, zs)
    assert np.frombuffer(oracle.uncompress(z), np.uint32).tobytes() == w.tobytes()
    good = digest(sim, z[17:], nfl=n)
    assert good[1] == (zlib.crc32(w.tobytes()), 4 * n)
    bad = bytearray(z)
    bad[17 + 16 + len(zs[0]) + 5 + 1000] ^= 0xff                              # byte 1000 of plane 1's first stored block
    acc = ref.new_acc(1)
    assert step(sim.lib, sim.ctx, bytes(bad[17:]), n, acc) == 0
    dec_bad = np.frombuffer(oracle.uncompress(bytes(bad)), np.uint32)
    assert int(np.count_nonzero(dec_bad != w)) == 1
    assert ref.records(acc, 1) == [(zlib.crc32(dec_bad.tobytes()), 4 * n)] != good[0]


def test_rejected_arguments(sim, data):
    rec, dec = data["b8"]
    offs = _offsets(rec)
    lib, ctx = sim.lib, sim.ctx
    acc = ref.new_acc(3)
    clean = acc.tobytes()
    for null in ("rec", "acc"):
        assert step(lib, ctx, rec, N, acc, null=(null,)) == EINVAL
    assert lib.mrcz_uncompress_digest(None, None, 0, N, CHK, 0, 0, 0, acc.ctypes.data) == EINVAL
    assert step(lib, ctx, rec, N, acc, first_chunk=1, nchunks=3) == EINVAL           # past the file's three chunks
    assert step(lib, ctx, rec, N, acc, first_chunk=4, nchunks=0) == EINVAL
    assert step(lib, ctx, rec, N, acc, chk=0) == EFORMAT
    assert step(lib, ctx, rec, N, acc, chk=CHK + 1) == EFORMAT
    assert step(lib, ctx, rec, N, acc, first_chunk=3, nchunks=0) == 0                 # nothing to do ...
    assert step(lib, ctx, rec, N, acc, first_chunk=0, nchunks=0, null=("rec",)) == 0
    w = util.aligned_empty(4 * 1024).view(np.uint32)
    assert lib.mrcz_digest_words(ctx, None, 0, 0, CHK, NONE, 0, 0.0, acc.ctypes.data) == 0
    assert acc.tobytes() == clean                                                    # ... and nothing touched
    assert lib.mrcz_digest_words(ctx, None, 1024, 0, CHK, NONE, 0, 0.0, acc.ctypes.data) == EINVAL
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, CHK, NONE, 0, 0.0, None) == EINVAL
    assert lib.mrcz_digest_words(None, w.ctypes.data, 1024, 0, CHK, NONE, 0, 0.0, acc.ctypes.data) == EINVAL
    assert lib.mrcz_digest_words(ctx, w.ctypes.data + 4, 1000, 0, CHK, NONE, 0, 0.0, acc.ctypes.data) == EINVAL   # misaligned
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, CHK, 4, 0, 0.0, acc.ctypes.data) == EINVAL          # unknown transform
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, CHK, MASK, 33, 0.0, acc.ctypes.data) == EINVAL
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, CHK, ABS, 0, 0.0, acc.ctypes.data) == EINVAL
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, 0, NONE, 0, 0.0, acc.ctypes.data) == EINVAL
    assert lib.mrcz_digest_words(ctx, w.ctypes.data, 1024, 0, CHK + 1, NONE, 0, 0.0, acc.ctypes.data) == EINVAL
    assert acc.tobytes() == clean
    t = ref.Digest()
    assert lib.mrcz_digest_finish(ctx, None, 0, 3, ctypes.byref(t)) == EINVAL
    assert lib.mrcz_digest_finish(ctx, acc.ctypes.data, 0, 3, None) == EINVAL
    assert lib.mrcz_digest_finish(None, acc.ctypes.data, 0, 3, ctypes.byref(t)) == EINVAL
    t.crc32, t.nbytes = 5, 5
    assert lib.mrcz_digest_finish(ctx, acc.ctypes.data, 0, 0, ctypes.byref(t)) == 0 and (t.crc32, t.reserved, t.nbytes) == (0, 0, 0)
    assert step(lib, ctx, rec[: offs[2]], N, acc) == EFORMAT                         # chunk 2's record is missing
    assert step(lib, ctx, rec[: offs[1] - 5], N, acc, nchunks=1) == EFORMAT          # chunk 0's record is cut
    assert step(lib, ctx, rec[: offs[2] + 9], N, acc) == EFORMAT                     # cut inside chunk 2's header
    assert step(lib, ctx, rec[: len(rec) - 3], N, acc) == EFORMAT                    # cut inside the last chunk's payload
    assert digest(sim, rec)[0] == ref.chunk_crcs(dec)                                # the context still works after refusals
