"""Inputs shared by test_gpu_compress_path.py and its emulator twin test_sim_compress_path.py: the small kernels between the
histograms and the emit pass of the compressor.

  k_block_reduce   sums a block's pair rows with several waves once the block has more than eight pairs;
  k_huffman        numbers the trees of a lane itself (no prefix kernel in front of it);
  k_huffman_hdr    counts, beside the headers, every pair's bits under its block's dynamic code and under the static code;
  k_stream_layout  picks one of the two by the block's type and scans the pairs' bit offsets.

Every expectation is the CPU oracle's container, every buffer is pre-filled with emit_whole_words_cases.PATTERN, and what a
case is meant to reach (how many pairs a block has, which type it gets) is asserted from the oracle's bytes and from the
plane, so that a case cannot silently stop covering it."""
import numpy as np

import emit_mixed_cases as mixed
import emit_whole_words_cases as whole
import util

SEG = 32768                 # plane positions per segment (mrcz_common.h)
BLK_SYMS = mixed.BLK_SYMS
BR_ROWS = 8                 # pair rows one wave of k_block_reduce sums per round (mrcz_compress.hip)


def coded_blocks(stream: bytes):
    """the blocks of a plane's stream without the empty stored block of the full flush"""
    blocks = mixed.walk_blocks(stream)
    assert blocks[-1][:2] == (0, 0)
    return blocks[:-1]


def segments_of(nbytes: int) -> int:
    return (nbytes + SEG - 1) // SEG


# ------------------------------------------------------------------ constant planes over many pairs
# n words of 10.0f at b = 0: every plane is one dynamic block over all its segments
CONSTANT_N = {262144: 8,        # exactly eight rows: one wave, no partial rows
              262145: 9,        # eight segments and one word: the ninth row is the second wave's only one
              294912: 9,        # nine full segments
              1081345: 34}      # 33 segments and a word: every wave has rows, the last group is ragged


def constant_words(n: int) -> np.ndarray:
    return np.full(n, 0x41200000, np.uint32)


def check_constant(n: int, container: bytes):
    assert segments_of(n) == CONSTANT_N[n]
    for plane in range(4):
        blocks = coded_blocks(mixed.plane_stream(container, plane))
        assert len(blocks) == 1 and blocks[0][0] == 2, (n, plane, [b[:2] for b in blocks])
        assert 1000 < blocks[0][1] <= 4200, blocks[0][1]          # 1018 symbols (262144) ... 4193 (1081345)


# ------------------------------------------------------------------ a sparse plane: many match lengths in the rows
SPARSE_BYTES = 40 * SEG + 777


def sparse_plane() -> np.ndarray:
    """0x33 everywhere but for one byte of 0x80..0x8f about every 3000 positions: one dynamic block over 41 pairs whose rows
    hold many different length codes (the runs between two marks are cut into matches of 258 and a remainder)"""
    rng = np.random.default_rng(41)
    p = np.full(SPARSE_BYTES, 0x33, np.uint8)
    pos = np.cumsum(rng.integers(2000, 4000, SPARSE_BYTES // 2000))
    pos = pos[pos < SPARSE_BYTES - 1]
    p[pos] = (0x80 + rng.integers(0, 16, len(pos))).astype(np.uint8)
    return p


def check_sparse(container: bytes):
    blocks = coded_blocks(mixed.plane_stream(container, mixed.PLANE))
    assert len(blocks) == 1 and blocks[0][0] == 2, [b[:2] for b in blocks]
    assert segments_of(SPARSE_BYTES) == 41 and 5000 < blocks[0][1] < BLK_SYMS
    ll = blocks[0][2]
    assert sum(1 for l in ll[257:] if l) >= 12, "few length codes in use"


# ------------------------------------------------------------------ a static block cut by a segment boundary
def static_cut_plane():
    """emit_mixed_cases.boundary_plane("static") -- a dynamic block of 32767 symbols, then a static one of 55 symbols in 75
    bytes -- behind runs of 0xF0 / 0xF1 of at most 258 bytes, as many as it takes for the second block to start 8..60
    positions before a multiple of 32768: the static block then lies in two segments, and the first of them holds pairs of
    both blocks.  Returns (plane, first position of the static block)."""
    body = mixed.boundary_plane("dynamic")
    tail = mixed.boundary_plane("static")
    S, _ = mixed.symbol_starts(body)
    starts = np.flatnonzero(S)
    cut0 = int(starts[BLK_SYMS])
    assert np.array_equal(tail[:cut0], body[:cut0])
    tail = tail[cut0:]
    assert len(tail) == 75
    for front in range(0, 20000):
        full, rem = divmod(front, 258)
        nsym = 2 * full + (rem if rem <= 3 else 2)        # a run of 4..258 bytes is a literal and a match
        cut = front + int(starts[BLK_SYMS - nsym])
        if 8 <= (-cut) % SEG <= 60:
            break
    else:
        raise AssertionError("no front puts the block boundary in front of a segment boundary")
    runs = [np.full(258, 0xF0 + (k & 1), np.uint8) for k in range(full)] + [np.full(rem, 0xF0 + (full & 1), np.uint8)]
    plane = np.concatenate(runs + [body[:cut - front], tail])
    return plane, cut


def check_static_cut(plane: np.ndarray, cut: int, container: bytes):
    S, _ = mixed.symbol_starts(plane)
    starts = np.flatnonzero(S)
    assert int(starts[BLK_SYMS]) == cut and len(starts) == BLK_SYMS + 55
    assert cut // SEG + 1 == (len(plane) - 1) // SEG, "the static block does not cross a segment boundary"
    blocks = coded_blocks(mixed.plane_stream(container, mixed.PLANE))
    assert [b[:2] for b in blocks] == [(2, BLK_SYMS), (1, 55)], [b[:2] for b in blocks]


# ------------------------------------------------------------------ inputs of the whole-word tests that still belong
KEPT = ("random200k_b0",                   # stored blocks (bit count 0) beside coded pairs, RAW planes
        "gauss300k_b0", "gauss300k_b8", "gauss300k_b12")      # nine blocks of two or three pairs


def kept(name: str):
    return whole.SMALL[name]()


# ------------------------------------------------------------------ GPU only
def constant_chunk_plus():
    """a whole chunk of 10.0f and 1000 words more, b = 0: one block over all 192 segments, and a second chunk of one tile"""
    return constant_words(util.CHUNK + 1000), 0


TWO_LANE_CHUNKS = 8       # mrcz_api.hip: a batch of >= 8 chunks runs as two lanes


def two_lane_words():
    """the smallest two-lane batch at b = 8: plane 0 of every chunk is masked to zero, one block of 192 pairs, and each lane
    numbers the trees of its own streams"""
    return util.gauss_words((TWO_LANE_CHUNKS - 1) * util.CHUNK + 1000, seed=1234), 8
