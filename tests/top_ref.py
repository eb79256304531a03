"""Shared by the top-planes decode tests (emulator, host tools, GPU): the numpy yardstick full_decode & mask(keep), the ctypes
prototypes of mrcz_record_top_span / mrcz_uncompress_top, thinned records built from mrcz_record_top_span, and containers whose
dropped payloads are overwritten."""
import ctypes

import numpy as np

import util

CHK = util.CHUNK
EINVAL, EFORMAT = -1, -4
F32, U16, THINNED = 0, 1, 4          # MRCZ_TOP_*
COMBOS = [(2, True), (2, False), (3, False)]          # (keep, 16-bit output)


def mask(keep: int) -> np.uint32:
    return np.uint32((0xFFFFFFFF << (8 * (4 - keep))) & 0xFFFFFFFF)


def expected(full: np.ndarray, keep: int, u16: bool = False) -> np.ndarray:
    """what top decode must return for the words `full` of the full decode"""
    m = full.astype(np.uint32) & mask(keep)
    return (m >> np.uint32(16)).astype(np.uint16) if u16 else m


def bind(lib):
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.mrcz_record_top_span.restype = i32
    lib.mrcz_record_top_span.argtypes = [vp, u32, i32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_uncompress_top.restype = i32
    lib.mrcz_uncompress_top.argtypes = [vp, vp, u64, u64, u32, u64, u64, i32, i32, vp, ctypes.POINTER(u64)]
    return lib


def span(lib, header16: bytes, n: int, keep: int):
    """(rc, skip, bytes) of mrcz_record_top_span"""
    sk, by = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xBEEF)
    rc = lib.mrcz_record_top_span(bytes(header16), n, keep, ctypes.byref(sk), ctypes.byref(by))
    return rc, sk.value, by.value


def lengths(header16) -> list:
    return [int(x) & 0x7fffffff for x in np.frombuffer(bytes(header16), "<u4")]


def offsets(rec, nfl: int, chk: int = CHK) -> list:
    """byte offset of every chunk record inside `rec` (records of a whole file), and of the end of the last"""
    offs, off = [], 0
    for _ in range((nfl + chk - 1) // chk):
        offs.append(off)
        off += 16 + sum(lengths(rec[off: off + 16]))
    return offs + [off]


def thin(lib, rec, nfl: int, keep: int, first_chunk: int = 0, chk: int = CHK) -> bytes:
    """the thinned records of `rec` = the ordinary records of chunks first_chunk, first_chunk + 1, ... of a file of nfl words:
    per record its 16-byte header, then bytes [skip, skip + bytes) of the record as mrcz_record_top_span gives them"""
    out, off, c = bytearray(), 0, first_chunk
    while off < len(rec):
        n = min(chk, nfl - c * chk)
        rc, sk, by = span(lib, rec[off: off + 16], n, keep)
        assert rc == 0
        out += rec[off: off + 16] + rec[off + sk: off + sk + by]
        off += sk + by
        c += 1
    assert off == len(rec)
    return bytes(out)


def poison(rec, nfl: int, keep: int, chk: int = CHK, byte: int = 0xFF) -> bytes:
    """`rec` with every payload byte of the dropped planes overwritten; the headers and the kept payloads are left alone"""
    out = bytearray(rec)
    for c, off in enumerate(offsets(rec, nfl, chk)[:-1]):
        dropped = sum(lengths(rec[off: off + 16])[: 4 - keep])
        out[off + 16: off + 16 + dropped] = bytes([byte]) * dropped
    return bytes(out)


def kept_share(rec, nfl: int, keep: int, chk: int = CHK) -> float:
    """kept payload bytes over record bytes"""
    kept = sum(sum(lengths(rec[off: off + 16])[4 - keep:]) for off in offsets(rec, nfl, chk)[:-1])
    return kept / len(rec)
