"""Inputs shared by test_gpu_cleared_planes.py and its emulator twin test_sim_cleared_planes.py: byte planes that the mask or the
"-s int" quantiser clears.  The host knows them before the first launch (cleared_planes, mrcz_api.hip), and for their tiles past
the file header k_tile_summary stores nothing and k_histogram / k_emit load nothing (tile_cleared, mrcz_tile.h): the workspace
keeps whatever an earlier call left there, and the records must not depend on it.

A case is (name, words, setting, first_chunk): setting = a mask level or "int", first_chunk = 0 (the chunk starts a file: its
first 256 words keep all their bits) or 1.  The expectation is the CPU oracle's: for a file-start chunk the record of
compress(words), for any other chunk the second record of compress(concat(zeros(CHUNK), words)) -- the oracle has no other way
to code a chunk without the header exemption (bench.py's parity_check does the same).  Every buffer is pre-filled with
emit_whole_words_cases.PATTERN, and what a case is meant to reach is asserted from the oracle's bytes."""
import functools

import numpy as np

import emit_mixed_cases as mixed
import probe_ref as pr
import util

CHK = util.CHUNK
TILE = 4096                 # plane positions per tile (mrcz_common.h)
RAW = 0x80000000            # bit 31 of a payload length in the chunk header: the plane is stored RAW


def noise(n: int) -> np.ndarray:
    """N(10, 3^2) floats, no header"""
    return util.gauss_words(n, seed=1000 + n, header=False)


def file_start(n: int) -> np.ndarray:
    """the first 256 words are arbitrary bits: plane 0 of tile 0 has literals that no mask touches"""
    w = noise(n)
    k = min(n, 256)
    w[:k] = util.kat_words(256)[:k]
    return w


def run_from_header(n: int) -> np.ndarray:
    """header words 200..255 with a zero low byte: plane 0's run of zeros starts inside the loaded tile 0 and extends over the
    cleared tiles behind it (TileInfo::B / F)"""
    w = file_start(n)
    w[199] |= 0x5a
    w[200:256] &= 0xFFFFFF00
    return w


# ------------------------------------------------------------------ the cases
# 1: not a file's first chunk, b = 8, plane 0 cleared in every tile.  13 / 14: the last RAW and the first static zero plane;
#    258..260: one match of maximal length and a remainder of 0, 1, 2; 4096 / 4097: a tile edge; 32768 / 32769: a segment edge
NONFIRST_N = (1, 13, 14, 258, 259, 260, 4095, 4096, 4097, 32768, 32769)
# 2: a file's first chunk, b = 8: tile 0 is loaded, at 4097 and 8197 the tiles behind it are cleared
FILESTART_N = (255, 256, 257, 300, 4096, 4097, 8197)
# 3: other mask levels, not a first chunk: 12 = plane 0 cleared and plane 1 half masked, 16 / 24 / 32 = two, three, four planes
#    cleared, 0 and 7 = none (the controls)
LEVELS = (0, 7, 12, 16, 24, 32)
LEVEL_N = 4097
# 4: "-s int": planes 1..3 cleared past the header
INT_FILESTART_N = (256, 257, 4097)
INT_NONFIRST_N = 4097
# 5: every case family again behind a call that left 0xA5 in every plane row
STALE_N = (13, 14, 4097)
STALE_WORD = 0xA5A5A5A5


def _case(name, words, setting, first_chunk):
    return (name, words, setting, first_chunk)


def nonfirst(n):
    return _case(f"nonfirst-b8-{n}", noise(n), 8, 1)


def filestart(n):
    return _case(f"filestart-b8-{n}", file_start(n), 8, 0)


def filestart_run():
    return _case("filestart-b8-run-from-header", run_from_header(8197), 8, 0)


def level(bits, n=LEVEL_N):
    return _case(f"nonfirst-b{bits}-{n}", noise(n), bits, 1)


def int_filestart(n):
    return _case(f"int-filestart-{n}", util.int_mode_words(n), "int", 0)


def int_nonfirst(n=INT_NONFIRST_N):
    return _case(f"int-nonfirst-{n}", util.int_mode_words(n), "int", 1)


def stale_cases(n):
    """cases 1-4 at one size"""
    return ([nonfirst(n), filestart(n)] + [level(b, n) for b in LEVELS if b != 8]
            + [_case(f"int-filestart-{n}", _int_words(n), "int", 0), _case(f"int-nonfirst-{n}", _int_words(n), "int", 1)])


def _int_words(n):
    """util.int_mode_words needs room for its specials: below that, noise around the int8 range"""
    return util.int_mode_words(n) if n >= 300 else (noise(n).view(np.float32) * np.float32(9.0)).view(np.uint32).copy()


def stale_words(n: int) -> np.ndarray:
    return np.full(n, STALE_WORD, np.uint32)


# 6 (GPU only): a file-start chunk and a later one in one grid
def two_chunk_words():
    w = util.gauss_words(CHK + 4097, seed=4097, header=False)
    w[:256] = util.kat_words(256)
    return w, 8


# ------------------------------------------------------------------ the oracle's answer
_cache = {}


def expected(oracle, case):
    """(record bytes, per-plane sums) of the case's chunk"""
    name, words, setting, first_chunk = case
    if name not in _cache:
        src = np.concatenate([np.zeros(CHK, np.uint32), words]) if first_chunk else words
        z = oracle.compress_int(src.tobytes()) if setting == "int" else oracle.compress(src, setting)
        offs = pr.record_offsets(z, len(src))
        assert len(offs) == first_chunk + 2
        _cache[name] = (z[offs[first_chunk]:], pr.plane_sums(z, len(src), first_chunk=first_chunk))
    return _cache[name]


def plane_lengths(record: bytes):
    return [int(x) for x in np.frombuffer(record[:16], "<u4")]


def plane0_blocks(record: bytes):
    """plane 0's blocks without the empty stored block of the full flush"""
    lens = plane_lengths(record)
    assert not lens[0] & RAW
    blocks = mixed.walk_blocks(record[16: 16 + lens[0]])
    assert blocks[-1][:2] == (0, 0)
    return blocks[:-1]


def check_raw_edge(n: int, record: bytes):
    """13 zero bytes are the last plane that goes out RAW, 14 the first that is one static block"""
    lens = plane_lengths(record)
    if n <= 13:
        assert lens[0] == (RAW | n), (n, hex(lens[0]))
    else:
        blocks = plane0_blocks(record)
        assert len(blocks) == 1, (n, [b[:2] for b in blocks])       # (a static block while it is short, a dynamic one later)
        if n == 14:
            assert blocks[0][0] == 1, blocks[0][:2]
        if n in (258, 259, 260):       # a literal, then one match of 257, 258, 258 bytes, and at 260 one more literal
            assert blocks[0][1] == {258: 2, 259: 2, 260: 3}[n], (n, blocks[0][1])


def check_run_from_header(words: np.ndarray):
    p0 = (words & np.uint32(0xff)).astype(np.uint8)
    p0[256:] = 0                        # b = 8
    assert p0[199] != 0 and not p0[200:].any() and len(p0) > 2 * TILE
