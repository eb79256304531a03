"""GPU: decoder conformance on an MI355X.  The hand-built catalogue of tests/inflate_catalogue.py at GPU sizes (blocks that span
16 KiB windows), the whole system-zlib parameter sweep, full 6 Mi-byte planes, the per-stream limits of the block-parallel
decoder as shipped (MAXCAND 1024 candidates, MAXSEG 2048 segments), and range / box decode over foreign containers.  For any
stream that zlib inflates to exactly the plane, the words must be zlib's; where the header of mrcz_inflate_par.hip predicts the
decode class, last_chain_fallbacks() / last_fallbacks() must say the same.  Every stream here is valid (zlib accepts it):
corrupted and malformed input is exercised on the emulator only."""
import functools
import zlib

import numpy as np
import pytest

import inflate_catalogue as ic
import util

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ic.hand_cases()] + [c.name for c in ic.mutation_catchers()]


@functools.lru_cache(maxsize=1)
def _big_catalogue():
    return {c.name: c for c in ic.hand_cases(big=True) + ic.mutation_catchers(big=True)}


@pytest.fixture(scope="module")
def codec():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    assert torch.cuda.is_available()
    c = MrcZipCodec(0, max_batch_chunks=8)
    yield c
    c.close()


def _decode(codec, c):
    back = np.frombuffer(codec.unzip_bytes(c.container), np.uint32)
    bad = np.flatnonzero(back != c.words)
    assert not len(bad), (c.name, len(bad), bad[:8])
    exp = c.expected_fallbacks()
    got = (codec.last_chain_fallbacks(), codec.last_fallbacks())
    if exp is not None:
        assert got == exp, (c.name, c.classes)
    return back, got


@pytest.mark.parametrize("name", NAMES)
def test_hand_built_streams(codec, name):
    _decode(codec, _big_catalogue()[name])


def test_python_zlib_full_sweep(codec):
    """level {0,1,6,9} x strategy {default, filtered, Huffman only, RLE, fixed} x memLevel {1,8,9} x window {9,15} x flush
    {full, finish, sync every 4 KiB, partial every 4 KiB}, four combinations per chunk, the input kinds in turn"""
    combos = list(ic.sweep_combos())
    assert len(combos) == 480
    classes = {}
    for c in ic.sweep_cases(combos, 65536, every=4096):
        _, got = _decode(codec, c)
        classes[got] = classes.get(got, 0) + 1
    print("sweep: containers per (chain, sequential) fall-backs", sorted(classes.items()))
    assert len(classes) > 1


@pytest.mark.parametrize("combos", [
    [(6, "rle", 9, 15, "full"), (6, "rle", 9, 15, "finish"), (1, "default", 8, 15, "finish"), (9, "huffman", 9, 15, "full")],
    [(0, "default", 9, 15, "full"), (6, "fixed", 1, 9, "full"), (9, "filtered", 8, 15, "sync"), (6, "rle", 1, 15, "partial")],
], ids=["a", "b"])
def test_python_zlib_full_planes(codec, combos):
    for c in ic.sweep_cases(combos, util.CHUNK, every=1 << 20):
        _decode(codec, c)


def _cliff_plane(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 6, n) * 0x11).astype(np.uint8)


@pytest.mark.parametrize("every,what", [(4096, "more than 1024 blocks"), (2048, "more than 2048 blocks and segments")])
def test_cliffs_at_the_shipped_limits(codec, every, what):
    """Z_RLE with Z_SYNC_FLUSH every few KiB on full 6 Mi-byte planes: a dynamic block and an empty stored block per piece,
    3072 / 6144 blocks per stream -- past MAXCAND (1024) and, in the second case, past MAXSEG (2048) too.  (With at most 1024
    blocks a 6 MiB plane cannot reach 2048 segments: a segment is one 16 KiB window of a block.)  Each stream must come back
    byte-exact through the chain fall-back."""
    n = util.CHUNK
    planes = [_cliff_plane(n, j) for j in range(4)]
    streams = [util.python_zlib_stream(p, 6, zlib.Z_RLE, 9, 15, "sync", every) for p in planes]
    c = ic.case(f"cliff_{every}", [ic.chunk(planes, streams, ["chain"] * 4)])
    _decode(codec, c)
    assert codec.last_chain_fallbacks() == 4 and codec.last_fallbacks() == 0, what




@pytest.mark.parametrize("name", ["static_with_data", "distance_codes_11_to_15_bits", "d1_after_empty_blocks",
                                  "pair_at_every_bit_residue", "stored_run_129_then_dynamic"])
def test_range_and_boxes_over_foreign_containers(codec, name):
    import torch
    from datacompressionfloat_amd._lib import MrczBoxGeom
    c = _big_catalogue()[name]
    full, _ = _decode(codec, c)
    n = len(full)
    for w0, w1 in ((0, n), (1, 258), (n // 3, min(n, n // 3 + 100001)), (n - 5, n)):
        got = np.frombuffer(codec.unzip_range(c.container, w0, w1), np.uint32)
        assert np.array_equal(got, full[w0:w1]), (name, w0, w1)
        assert (codec.last_chain_fallbacks(), codec.last_fallbacks()) == c.expected_fallbacks()
    d0, nx, ny = 7, 64, 32
    nz = (n - d0) // (nx * ny)
    bx, by, bz = 9, 6, 3
    origins = np.array([(0, 0, 0), (nx - bx, ny - by, nz - bz), (20, 7, nz // 2), (-4, 30, 1), (60, -2, nz - 2)], np.int32)
    g = MrczBoxGeom(d0, nx, ny, nz, bx, by, bz, 0xDEADBEEF)
    rec = torch.frombuffer(bytearray(c.records), dtype=torch.uint8).to(codec.device)
    out, dec = codec.uncompress_boxes_device(rec, n, g, origins)
    got = out.cpu().numpy().view(np.uint32)
    vol = np.pad(full[d0: d0 + nz * nx * ny].reshape(nz, ny, nx), ((bz, bz), (by, by), (bx, bx)), constant_values=np.uint32(0xDEADBEEF))
    for i, (x, y, z) in enumerate(origins.tolist()):
        assert np.array_equal(got[i], vol[z + bz: z + 2 * bz, y + by: y + 2 * by, x + bx: x + 2 * bx]), (name, i)
    assert dec == 1
    assert (codec.last_chain_fallbacks(), codec.last_fallbacks()) == c.expected_fallbacks()


def test_mixed_chunks(codec):
    for tail in (70001, util.CHUNK - 1):
        c = ic.mixed_container(tail)
        _decode(codec, c)
        assert (codec.last_chain_fallbacks(), codec.last_fallbacks()) == (4, 2)


def test_chain_fallbacks_latched_across_compress(codec):
    c = _big_catalogue()["static_with_data"]
    _decode(codec, c)
    assert codec.last_chain_fallbacks() == 1
    w = util.gauss_words(20000)
    codec.zip_bytes(w.tobytes(), 8)
    assert codec.last_chain_fallbacks() == 1 and codec.last_fallbacks() == 0
