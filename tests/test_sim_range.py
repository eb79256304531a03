"""CPU-only: range decode (mrcz_uncompress_range, mrcz_records_index) on the SIMT emulator build of the product sources.
Windows of multi-chunk files must equal the same words of the whole-file decode: the exempt header words, windows at every
alignment, across chunk and batch boundaries, records that start at a later chunk, and the arguments that are refused."""
import ctypes

import numpy as np
import pytest

import util

EINVAL, EFORMAT = -1, -4
CHK = util.CHUNK
N = 2 * CHK + 4097          # three chunks, the last one short; batches of two chunks


def _volume(n=N):
    w = np.zeros(n, np.uint32)
    w[:256] = util.kat_words(256)
    for c in range((n + CHK - 1) // CHK):       # a noisy stretch per chunk so that the records differ
        a = c * CHK + 300 * (c + 1)
        m = min(3000, n - a)
        w[a: a + m] = util.gauss_words(3000, seed=30 + c, header=False)[:m]
    w[CHK - 2000: CHK + 2000] = util.gauss_words(4000, seed=77, header=False)  # noise across the chunk boundary
    w[n - 1500:] = util.gauss_words(1500, seed=78, header=False)               # and up to the file's last word
    return w


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    s.lib.mrcz_record_size.argtypes = [vp, u32, ctypes.POINTER(u64)]
    s.lib.mrcz_records_index.argtypes = [vp, u64, u64, u32, ctypes.POINTER(u64)]
    s.lib.mrcz_uncompress_range.argtypes = [vp, vp, u64, u64, u32, u64, u64, u64, vp, i32, ctypes.POINTER(u64)]
    return s


def _range(sim, rec, nfile, w0, w1, first_chunk=0, int_mode=False, chk=CHK):
    r = util.aligned_empty(len(rec) + 8)
    r[:len(rec)] = np.frombuffer(rec, np.uint8)
    out = util.aligned_empty(4 * max(w1 - w0, 1)).view(np.uint32)
    cons = ctypes.c_uint64()
    rc = sim.lib.mrcz_uncompress_range(sim.ctx, r.ctypes.data, len(rec), nfile, chk, first_chunk, w0, w1, out.ctypes.data,
                                       1 if int_mode else 0, ctypes.byref(cons))
    return rc, out[:max(w1 - w0, 0)].copy(), cons.value


def _index(sim, rec, nfile, chk=CHK):
    nch = (nfile + chk - 1) // chk
    offs = (ctypes.c_uint64 * (nch + 1))()
    rc = sim.lib.mrcz_records_index(rec, len(rec), nfile, chk, offs)
    return rc, list(offs)


def _py_index(rec, nfile, chk=CHK):
    offs, off = [], 0
    for c in range((nfile + chk - 1) // chk):
        offs.append(off)
        h = np.frombuffer(rec[off: off + 16], "<u4")
        off += 16 + int(sum(int(x) & 0x7fffffff for x in h))
    return offs + [off]


def _windows(n):
    return [
        (0, 256), (3, 200), (255, 256),                 # inside the exempt header words
        (250, 262), (100, 5000), (256, 4099),           # straddling word 256
        (4097, 4097 + 8190), (8194, 8194 + 5), (12291, 30001), (1, 2),  # w0 % 4 = 1, 2, 3, 1; one word
        (777, 778), (CHK - 1, CHK),                     # one word
        (CHK - 3001, CHK + 2999), (CHK - 1, CHK + 1),   # across the chunk boundary
        (2 * CHK - 5, 2 * CHK + 7),                     # across the batch boundary (batches of two chunks)
        (0, n),                                         # the whole file
        (n - 1, n), (n - 5003, n), (CHK + 17, n),       # ending at the file's last word
    ]


@pytest.mark.parametrize("mode", [0, 8, 23, "int"])
def test_windows_equal_the_whole_decode(sim, mode):
    w = _volume()
    int_mode = mode == "int"
    rec = sim.compress_records(w, 0 if int_mode else mode, int_mode=int_mode)
    full = sim.uncompress_records(rec, N, int_mode=int_mode)
    if int_mode:
        assert np.array_equal(full, util.int_mode_expected(w))
    else:
        assert np.array_equal(full, util.erase_expected(w, mode))
    offs = _py_index(rec, N)
    for w0, w1 in _windows(N):
        rc, got, cons = _range(sim, rec, N, w0, w1, int_mode=int_mode)
        assert rc == 0, (w0, w1, sim.lib.mrcz_last_error(sim.ctx))
        assert np.array_equal(got, full[w0:w1]), (mode, w0, w1, np.flatnonzero(got != full[w0:w1])[:8])
        assert cons == offs[(w1 + CHK - 1) // CHK], (w0, w1)  # nothing past the window's last record consumed


def test_records_of_later_chunks_decode_alone(sim):
    w = _volume()
    rec = sim.compress_records(w, 8)
    full = util.erase_expected(w, 8)
    offs = _py_index(rec, N)
    for c in (1, 2):
        tail = rec[offs[c]:]
        for w0, w1 in ((c * CHK, c * CHK + 1), (c * CHK + 3, min(N, c * CHK + 9001)), (N - 7, N)):
            rc, got, cons = _range(sim, tail, N, w0, w1, first_chunk=c)
            assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
            assert np.array_equal(got, full[w0:w1]), (c, w0, w1)
    # only the records of chunk 1: chunk 1 decodes, chunk 2 is refused (the records end before it)
    one = rec[offs[1]:offs[2]]
    rc, got, _ = _range(sim, one, N, CHK + 5, 2 * CHK)
    assert rc == EFORMAT                                 # read as the records of chunks 0 and 1, they end before chunk 1's
    rc, got, _ = _range(sim, one, N, CHK + 5, 2 * CHK, first_chunk=1)
    assert rc == 0 and np.array_equal(got, full[CHK + 5: 2 * CHK])
    rc, _, _ = _range(sim, one, N, CHK + 5, 2 * CHK + 1, first_chunk=1)
    assert rc == EFORMAT
    # records of chunks 0 and 1 walked past, chunk 2 decoded (first_chunk before the window)
    rc, got, _ = _range(sim, rec, N, 2 * CHK + 10, N)
    assert rc == 0 and np.array_equal(got, full[2 * CHK + 10:])


def test_int_mode_header_words_in_a_later_batch_start(sim):
    # int mode: header words stay as they are only in chunk 0 of the file, not at the start of a later batch
    w = _volume()
    rec = sim.compress_records(w, 0, int_mode=True)
    exp = util.int_mode_expected(w)
    offs = _py_index(rec, N)
    rc, got, _ = _range(sim, rec[offs[2]:], N, 2 * CHK, 2 * CHK + 300, first_chunk=2, int_mode=True)
    assert rc == 0 and np.array_equal(got, exp[2 * CHK: 2 * CHK + 300])


def test_single_small_chunk(sim):
    # one chunk smaller than CHUNK_SIZE (chk = nfloats, as the reference writes small files)
    n = 70001
    w = util.gauss_words(n, seed=5)
    rec = sim.compress_records(w, 12)
    exp = util.erase_expected(w, 12)
    for w0, w1 in ((0, n), (5, 9), (255, 258), (4095, 8193), (n - 3, n)):
        rc, got, _ = _range(sim, rec, n, w0, w1, chk=n)
        assert rc == 0 and np.array_equal(got, exp[w0:w1]), (w0, w1)


def test_records_index_matches_a_walk_of_the_headers(sim):
    w = _volume()
    rec = sim.compress_records(w, 23)
    rc, offs = _index(sim, rec, N)
    assert rc == 0 and offs == _py_index(rec, N) and offs[-1] == len(rec)
    rc, _ = _index(sim, rec[:-1], N)
    assert rc == EFORMAT
    rc, _ = _index(sim, rec[: offs[2] + 15], N)          # cut inside the last chunk header
    assert rc == EFORMAT
    size = ctypes.c_uint64()
    assert sim.lib.mrcz_record_size(rec, CHK, ctypes.byref(size)) == 0 and size.value == offs[1]
    bad = bytearray(rec[:16])
    bad[3] = 0x7f                                         # a deflate payload longer than any plane of a chunk
    assert sim.lib.mrcz_record_size(bytes(bad), CHK, ctypes.byref(size)) == EFORMAT
    bad[3] = 0x80; bad[0] = bad[1] = bad[2] = 0           # a RAW plane shorter than the chunk
    assert sim.lib.mrcz_record_size(bytes(bad), CHK, ctypes.byref(size)) == EFORMAT


def test_rejected_arguments(sim):
    n = 20000
    w = util.gauss_words(n, seed=9)
    rec = sim.compress_records(w, 8)
    assert _range(sim, rec, n, 5, 5, chk=n)[0] == EINVAL          # empty
    assert _range(sim, rec, n, 9, 5, chk=n)[0] == EINVAL          # reversed
    assert _range(sim, rec, n, 0, n + 1, chk=n)[0] == EINVAL      # past the file
    assert _range(sim, rec, n, 0, 10, chk=0)[0] == EFORMAT        # no chunk size
    assert _range(sim, rec, n, 0, 10, first_chunk=1, chk=n)[0] == EINVAL  # records begin after the window
    assert _range(sim, rec[:-3], n, 0, 10, chk=n)[0] == EFORMAT   # records end inside the window's chunk
    assert _range(sim, rec[:10], n, 0, 10, chk=n)[0] == EFORMAT   # inside the chunk header
    # a window that is fine after refusals (the context is still usable)
    rc, got, _ = _range(sim, rec, n, 10, 20, chk=n)
    assert rc == 0 and np.array_equal(got, util.erase_expected(w, 8)[10:20])
