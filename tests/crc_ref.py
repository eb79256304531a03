"""The yardstick of the digest tests: Python's zlib.crc32 over the words a container decodes to, per chunk and for the file, and the
bindings and small helpers the digest test files share."""
import ctypes
import zlib

import numpy as np

import util

NONE, MASK, INT8, ABS = 0, 1, 2, 3          # MRCZ_DIGEST_*
EINVAL, EFORMAT = -1, -4
GARBAGE = 0xA5


class Digest(ctypes.Structure):
    """mrcz_digest_t"""
    _fields_ = [("crc32", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("nbytes", ctypes.c_uint64)]


def bind(lib):
    vp, u64, u32, i32, f32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
    lib.mrcz_crc32_combine.restype = u32
    lib.mrcz_crc32_combine.argtypes = [u32, u32, u64]
    lib.mrcz_uncompress_digest.argtypes = [vp, vp, u64, u64, u32, u64, u64, i32, vp]
    lib.mrcz_digest_words.argtypes = [vp, vp, u64, u64, u32, i32, i32, f32, vp]
    lib.mrcz_digest_words_async.argtypes = [vp, vp, u64, u64, u32, i32, i32, f32, vp]
    lib.mrcz_digest_finish.argtypes = [vp, vp, u64, u64, vp]


def chunk_crcs(decoded, chk=util.CHUNK):
    """[(zlib.crc32, bytes)] of every chunk of the decoded words"""
    b = np.ascontiguousarray(decoded).view(np.uint8).tobytes()
    return [(zlib.crc32(b[a: a + 4 * chk]), len(b[a: a + 4 * chk])) for a in range(0, len(b), 4 * chk)]


def file_crc(decoded):
    return zlib.crc32(np.ascontiguousarray(decoded).view(np.uint8).tobytes())


def new_acc(nchunks):
    a = util.aligned_empty(ctypes.sizeof(Digest) * max(nchunks, 1))
    a[:] = GARBAGE                                  # d_acc needs no zeroing
    return a


def records(acc, nchunks, first_chunk=0):
    """[(crc32, nbytes)] of records first_chunk .. nchunks - 1; the reserved word must be 0"""
    out = []
    for i in range(first_chunk, nchunks):
        d = Digest.from_buffer_copy(acc[i * 16: i * 16 + 16].tobytes())
        assert d.reserved == 0
        out.append((d.crc32, d.nbytes))
    return out


def finish(lib, ctx, acc, first_chunk, nchunks):
    t = Digest()
    assert lib.mrcz_digest_finish(ctx, acc.ctypes.data, first_chunk, nchunks, ctypes.byref(t)) == 0
    assert t.reserved == 0
    return t.crc32, t.nbytes


def raw_payload_span(rec, offs, c, nwords):
    """(plane, start, end) of a RAW payload of chunk c, offsets into rec: the plane is found by the RAW bit of the chunk header"""
    import struct
    lens = struct.unpack("<4I", rec[offs[c]: offs[c] + 16])
    pos = offs[c] + 16
    for j, l in enumerate(lens):
        n = l & 0x7fffffff
        if l & 0x80000000:
            assert n == nwords
            return j, pos, pos + n
        pos += n
    return None
