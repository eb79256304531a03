"""CPU-only, no emulator: the host arithmetic of digest decode.  mrcz_crc32_combine of the product library against zlib.crc32 of
the joined bytes, and the text sidecar's writer and parser."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import crc_ref as ref
import util

LIB = os.path.join(util.ROOT, "datacompressionfloat_amd", "lib", "libmrcz_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import sys
        sys.path.insert(0, util.ROOT)
        import __graft_entry__ as g
        g.build()
    l = ctypes.CDLL(LIB)
    ref.bind(l)
    return l


def test_combine_equals_crc32_of_the_joined_bytes(lib):
    rng = np.random.default_rng(11)
    pieces = [b"", b"\x00", b"a", bytes(rng.integers(0, 256, 100003, dtype=np.uint8)), bytes(rng.integers(0, 256, 393221, dtype=np.uint8)),
              bytes(rng.integers(0, 256, 4 * util.CHUNK, dtype=np.uint8))]            # a full chunk's 25,165,824 bytes
    crcs = [zlib.crc32(p) for p in pieces]
    for a, ca in zip(pieces, crcs):
        for b, cb in zip(pieces, crcs):
            assert lib.mrcz_crc32_combine(ca, cb, len(b)) == zlib.crc32(b, ca), (len(a), len(b))   # zlib.crc32(b, crc(a)) = crc(a + b)
    assert zlib.crc32(pieces[3] + pieces[4]) == lib.mrcz_crc32_combine(crcs[3], crcs[4], len(pieces[4]))


def test_combine_over_a_length_above_2_to_the_32(lib):
    a = b"the bytes in front"
    n = (1 << 32) + 12345
    zeros = bytes(1 << 26)
    cb, cab, left = 0, zlib.crc32(a), n
    while left:                                          # B = n zero bytes, its crc32 taken in pieces: no 4 GiB buffer
        k = min(left, len(zeros))
        cb = zlib.crc32(zeros[:k], cb)
        cab = zlib.crc32(zeros[:k], cab)
        left -= k
    assert lib.mrcz_crc32_combine(zlib.crc32(a), cb, n) == cab
    assert lib.mrcz_crc32_combine(zlib.crc32(a), cb, n & 0xFFFFFFFF) != cab           # the count is 64 bits wide


def test_sidecar_round_trip_and_refusals():
    from datacompressionfloat_amd import MrczError, format_sidecar, parse_sidecar
    crcs = [0, 0xFFFFFFFF, 0x0000BEEF]
    text = format_sidecar(2 * util.CHUNK + 5, util.CHUNK, "int", 0x00C0FFEE, crcs)
    assert text == f"mrcz-digest crc32 1\nwords {2 * util.CHUNK + 5} chunk {util.CHUNK} chunks 3 mode int\nfile 00c0ffee\n0 00000000\n1 ffffffff\n2 0000beef\n"
    sc = parse_sidecar(text)
    assert sc == {"words": 2 * util.CHUNK + 5, "chunk": util.CHUNK, "chunks": 3, "mode": "int", "file": 0x00C0FFEE, "crcs": crcs}
    assert parse_sidecar(text.encode()) == sc
    assert parse_sidecar(format_sidecar(0, util.CHUNK, "float", 0, []))["crcs"] == []
    lines = text.split("\n")
    bad = ["", "mrcz-digest crc32 2\n" + "\n".join(lines[1:]), "\n".join(lines[:-2]) + "\n", text + "3 00000000\n", text.replace("00c0ffee", "00C0FFEE"),
           text.replace("1 ffffffff", "2 ffffffff"), text.replace("chunks 3", "chunks 4"), text.replace("mode int", "mode half"),
           text.replace("file 00c0ffee", "file c0ffee"), text.replace("words ", "words -"), text.replace(f"chunk {util.CHUNK}", "chunk 0"), b"\xff\xfe" + text.encode()]
    for t in bad:
        with pytest.raises(MrczError):
            parse_sidecar(t)
    with pytest.raises(MrczError):
        format_sidecar(4, 4, "half", 0, [0])
