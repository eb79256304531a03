"""Inputs shared by test_gpu_decision_edges.py and its emulator twin test_sim_decision_edges.py: planes that sit exactly on the
integer comparisons that fix the compressor's output.  All but the last are made in k_stream_layout (mrcz_compress.hip):

  block type   stored iff stored_len + 4 <= opt_lenb && stored_ok, else static iff static_lenb == opt_lenb (byte counts, after
               static_lenb <= opt_lenb folded the minimum into opt_lenb), else dynamic;
  stored_ok    start >= 32768 * (slides the encoder's window made before the block was flushed), SURVEY App. B.4;
  RAW          a plane is COMPRESSED iff n > min(zlen, CHK) + 4 (zip.c:170-177);
  full block   nsym == nblk * 32767: whether the last block was flushed inside the loop or after it.

An off-by-one in any of them changes the container only for inputs that sit on the tie, so every family below is built to sit
there, and asserts that it does from the CPU oracle alone (stream_info below, Oracle.deflate, the chunk headers of the oracle's
container): a case cannot silently stop covering its edge.  The planes come from fixed numpy seeds; where a seed's draws are
what puts a plane on its edge, the expected difference stands beside it and is asserted.

A case is the words of one compress call at bits = 0: the planes under test in some of the four byte lanes, zero elsewhere.
check_case() is the one check both twins run for it."""
import ctypes
import functools

import numpy as np

import emit_whole_words_cases as whole
import probe_ref as pr
import util

CHK = util.CHUNK
BLK_SYMS = 32767
MAXBLK = 194                # blocks of one stream at most (mrcz_common.h)


# ------------------------------------------------------------------ the two block tables
# (bound here, not in util.py: every test imports util.py, and these two functions are this file's alone)
class OracleStreamInfo(ctypes.Structure):
    """mrcz_oracle_stream_info_t"""
    _fields_ = [("nsym", ctypes.c_uint32), ("nblocks", ctypes.c_uint32), ("nmatch", ctypes.c_uint32)]


class OracleBlockInfo(ctypes.Structure):
    """mrcz_oracle_block_info_t"""
    _fields_ = [("start", ctypes.c_uint32), ("end", ctypes.c_uint32), ("btype", ctypes.c_uint32), ("stored_ok", ctypes.c_uint32),
                ("bits", ctypes.c_uint64), ("opt_len", ctypes.c_uint32), ("static_len", ctypes.c_uint32)]


class BlockInfo(ctypes.Structure):
    """mrcz_block_info_t (include/mrcz_hip.h)"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("start", "end", "btype", "opt_len", "static_len", "bitpos")]


def stream_info(oracle, plane: np.ndarray):
    """mrcz_oracle_stream_info of one plane: (nsym, nblocks, nmatch, blocks), blocks = one dict per block of the stream with
    the fields of mrcz_oracle_block_info_t (start, end, btype, stored_ok, bits, opt_len, static_len)"""
    f = oracle.lib.mrcz_oracle_stream_info
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    si = OracleStreamInfo()
    cap = len(plane) // BLK_SYMS + 2           # a block holds 32767 symbols, a symbol at least one byte
    blocks = (OracleBlockInfo * cap)()
    rc = f(plane.ctypes.data, len(plane), ctypes.byref(si), blocks, cap)
    if rc != 0 or si.nblocks > cap:
        raise RuntimeError("oracle stream_info failed")
    return int(si.nsym), int(si.nblocks), int(si.nmatch), [
        {k: int(getattr(blocks[b], k)) for k, _ in OracleBlockInfo._fields_} for b in range(si.nblocks)]


def debug_blocks(lib, ctx, stream: int):
    """mrcz_debug_blocks: the block table of stream 4 * chunk + plane of the last compress call of the context, one dict per
    block.  `lib` is the emulator's library or the GPU's: the C ABI is the same."""
    lib.mrcz_debug_blocks.restype = ctypes.c_int
    lib.mrcz_debug_blocks.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(BlockInfo), ctypes.c_uint32]
    blocks = (BlockInfo * MAXBLK)()
    nb = lib.mrcz_debug_blocks(ctx, stream, blocks, MAXBLK)
    if nb < 0 or nb > MAXBLK:
        raise RuntimeError(f"mrcz_debug_blocks({stream}) returned {nb}")
    return [{k: int(getattr(blocks[b], k)) for k, _ in BlockInfo._fields_} for b in range(nb)]


class Backend:
    """what a twin gives check_case: the codec under test behind four calls"""

    def compress_prefilled(self, words):
        """-> (the whole buffer, pre-filled with whole.PATTERN, after the call; out_len; plane_bytes)"""
        raise NotImplementedError

    def blocks(self, stream):
        """debug_blocks (below) of one stream of that call"""
        raise NotImplementedError

    def probe(self, words):
        """mrcz_probe_chunks(MASK, bits 0) -> (out_len, plane_bytes)"""
        raise NotImplementedError

    def decode(self, records, nwords):
        """-> (decoded words, last_fallbacks())"""
        raise NotImplementedError


def words_of(planes: dict, n: int) -> np.ndarray:
    """n words whose byte lane j is planes[j]; the lanes not named are zero"""
    b = np.zeros((n, 4), np.uint8)
    for j, p in planes.items():
        assert len(p) == n, (j, len(p), n)
        b[:, j] = p
    return b.reshape(-1).view(np.uint32)


def planes_of(words: np.ndarray, chunk: int = 0):
    b = words.view(np.uint8).reshape(-1, 4)[chunk * CHK: (chunk + 1) * CHK]
    return [np.ascontiguousarray(b[:, j]) for j in range(4)]


def chunk_headers(z: bytes, nwords: int):
    """per chunk of a container the four (is RAW, payload length)"""
    out = []
    for off in pr.record_offsets(z, nwords)[:-1]:
        out.append([(bool(int(x) >> 31), int(x) & 0x7fffffff) for x in np.frombuffer(z[off: off + 16], "<u4")])
    return out


def lenb(bits: int) -> int:
    return (bits + 3 + 7) >> 3


def stored_diff(b: dict) -> int:
    """stored_len + 4 - opt_lenb of an oracle block: stored iff <= 0 and stored_ok"""
    return b["end"] - b["start"] + 4 - min(lenb(b["opt_len"]), lenb(b["static_len"]))


def raw_diff(oracle, plane) -> int:
    """n - (len + 4) of a plane: COMPRESSED iff > 0"""
    return len(plane) - (min(len(oracle.deflate(plane)), CHK) + 4)


def noise(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


def five_runs(nruns: int, lead: int = 0) -> np.ndarray:
    """`lead` single bytes, each different from its neighbours, then runs of five bytes: a literal and a match of four each"""
    return np.concatenate([(0xe0 + (np.arange(lead) & 1)).astype(np.uint8), np.repeat((0x30 + np.arange(nruns) % 9).astype(np.uint8), 5)])


def check_case(be: Backend, oracle, words: np.ndarray, name, max_batch_chunks: int = 2):
    """The per-case check: container and plane sums, the block table of every stream, the probe's sizes, and the decode of the
    oracle's container.  Returns the oracle's container."""
    n = len(words)
    nch = (n + CHK - 1) // CHK
    assert nch <= max_batch_chunks, "mrcz_debug_blocks shows the last batch of a call only"
    z = oracle.compress(words, 0, threads=nch if nch > 1 else 0)
    got, olen, sums = be.compress_prefilled(words)
    whole.check(got, olen, z[17:], name)
    assert sums == pr.plane_sums(z, n), name
    for c in range(nch):
        for j, plane in enumerate(planes_of(words, c)):
            _, nblocks, _, want = stream_info(oracle, plane)
            have = be.blocks(4 * c + j)
            assert len(have) == nblocks == len(want), (name, c, j, len(have), nblocks)
            bit = 0
            for k, (h, w) in enumerate(zip(have, want)):
                for f in ("start", "end", "btype", "opt_len", "static_len"):
                    assert h[f] == w[f], (name, "chunk", c, "plane", j, "block", k, f, h, w)
                assert h["bitpos"] == bit, (name, "chunk", c, "plane", j, "block", k, "bitpos", h["bitpos"], bit)
                bit += w["bits"]
    assert be.probe(words) == (olen, sums), name
    dec, fallbacks = be.decode(z[17:], n)
    assert np.array_equal(dec, words), name
    assert fallbacks == 0, (name, fallbacks)
    return z


# ------------------------------------------------------------------ A: the RAW threshold on small planes
A0_N = range(1, 41)                  # all-zero planes of n bytes
A1_N = range(30, 81)                 # the first n of A1_SOURCE
A0_EDGE = {12: -1, 13: 0, 14: 1}     # n -> n - (len + 4)
A1_EDGE = {48: -1, 49: 0, 50: -1, 51: 0, 52: 0, 53: 1, 54: 1}
A_SIM = (1, 4, 12, 13, 14, 30, 40, 49, 50, 51, 52, 53, 54, 80)      # the emulator's share of 1 ... 80


def a1_source():
    return np.random.default_rng(1).integers(0, 16, 400).astype(np.uint8)


def a_members(n: int) -> dict:
    """lane -> plane of case A-n: the A1 member in lane 0 where n has one, the A0 member in lane 2 (and, being zero, in every
    lane not taken); n = 30 ... 40 has both"""
    m = {}
    if n in A1_N:
        m[0] = a1_source()[:n]
    if n in A0_N:
        m[2] = np.zeros(n, np.uint8)
    return m


def a_case(oracle, n: int, behind_full_chunk: bool = False) -> np.ndarray:
    m = a_members(n)
    words = words_of(m, n)
    diffs = a_diffs(oracle, n)
    if n in A0_EDGE:
        assert diffs[2] == A0_EDGE[n], (n, diffs)
    if n in A1_EDGE:
        assert diffs[0] == A1_EDGE[n], (n, diffs)
    if behind_full_chunk:
        words = np.concatenate([np.full(CHK, 0x41200000, np.uint32), words])
    return words


def a_diffs(oracle, n: int) -> dict:
    return {j: raw_diff(oracle, p) for j, p in a_members(n).items()}


def check_a_headers(oracle, n: int, z: bytes, chunk: int = 0):
    """the oracle's chunk header says RAW exactly where n <= len + 4"""
    hdr = chunk_headers(z, chunk * CHK + n)[chunk]
    for j, d in a_diffs(oracle, n).items():
        assert hdr[j][0] == (d <= 0), (n, j, d, hdr[j])
        assert hdr[j][1] == (n if d <= 0 else n - d - 4), (n, j, d, hdr[j])


def a_conditions(oracle):
    diffs = [d for n in range(1, 81) for d in a_diffs(oracle, n).values()]
    assert 0 in diffs and 1 in diffs and -1 in diffs, sorted(set(diffs))
    for n in (13, 14, 52, 53):                      # one tie and one n == len + 5 in each of A0 and A1, through the container
        check_a_headers(oracle, n, oracle.compress(a_case(oracle, n), 0))


# ------------------------------------------------------------------ B: stored_len + 4 against opt_lenb
B_BYTES = 20000
# t -> stored_len + 4 - opt_lenb of the plane base[:t] + low[t:]: the twelve t around the sign change (bisected on the oracle)
B_T = {11453: 1, 11454: 0, 11455: 0, 11456: 1, 11458: 1, 11459: 0, 11460: 1, 11469: 1, 11470: 0, 11502: 0, 11503: -1, 11504: -1}
B_CASES = {k: sorted(B_T)[k::3] for k in range(3)}          # four members a call, one a lane


def b_plane(t: int) -> np.ndarray:
    """uniform over 256 values up to t, over 200 behind: the later t, the closer to incompressible"""
    base = np.random.default_rng(11).integers(0, 256, B_BYTES).astype(np.uint8)
    low = np.random.default_rng(12).integers(0, 200, B_BYTES).astype(np.uint8)
    return np.concatenate([base[:t], low[t:]])


def b_block(oracle, t: int) -> dict:
    _, nblocks, _, blocks = stream_info(oracle, b_plane(t))
    assert nblocks == 1
    b = blocks[0]
    assert stored_diff(b) == B_T[t], (t, stored_diff(b), B_T[t])
    assert b["stored_ok"] == 1 and (b["btype"] == 0) == (B_T[t] <= 0), (t, b)
    return b


def b_case(oracle, k: int) -> np.ndarray:
    for t in B_CASES[k]:
        b_block(oracle, t)
    return words_of({j: b_plane(t) for j, t in enumerate(B_CASES[k])}, B_BYTES)


def b_conditions(oracle):
    blocks = [b_block(oracle, t) for t in B_T]
    assert any(stored_diff(b) == 0 and b["stored_ok"] and b["btype"] == 0 for b in blocks)
    assert any(stored_diff(b) == 1 and b["btype"] != 0 for b in blocks)
    assert any(stored_diff(b) == -1 and b["btype"] == 0 for b in blocks)
    assert sorted(t for ts in B_CASES.values() for t in ts) == sorted(B_T)


# ------------------------------------------------------------------ C: static against dynamic, in bytes
# (seed, n): the first n of default_rng(seed).integers(0, 5, 1500) * 29.  TIE: static_lenb == opt_lenb although static_len >
# opt_len in bits (static); NEXT: static_lenb == opt_lenb + 1 (dynamic).  Found by a search over seeds 0 ... 39, n = 20 ... 1200.
TIE, NEXT = "tie", "next"
C_CASES = {
    "24": {0: (17, 24, TIE), 1: (1, 24, NEXT), 2: (19, 24, TIE), 3: (3, 24, NEXT)},
    "25": {0: (13, 25, TIE), 1: (17, 25, NEXT), 2: (1, 25, NEXT)},
    "26": {2: (13, 26, TIE)},
    "27": {2: (0, 27, TIE), 0: (13, 27, NEXT)},
    "28": {2: (12, 28, TIE), 0: (0, 28, NEXT)},
    "29": {2: (5, 29, TIE), 0: (12, 29, NEXT)},
    "30": {2: (9, 30, TIE), 0: (5, 30, NEXT)},
    # the same behind a full block of five-byte runs: these planes are COMPRESSED, so the choice is in the container's bits too
    # (the planes above are shorter than their streams and stored RAW: there it shows in the block table alone)
    "25-second-block": {2: (13, 25, TIE), 0: (17, 25, NEXT)},
}
C_FRONT_SYMS = BLK_SYMS


def c_member(seed: int, n: int) -> np.ndarray:
    return (np.random.default_rng(seed).integers(0, 5, 1500) * 29).astype(np.uint8)[:n]


def c_kind(b: dict):
    s, o = lenb(b["static_len"]), lenb(b["opt_len"])
    if s == o and b["static_len"] > b["opt_len"]:
        return TIE
    return NEXT if s == o + 1 else None


def c_case(oracle, name: str) -> np.ndarray:
    front = five_runs((C_FRONT_SYMS - 1) // 2, lead=1) if name.endswith("second-block") else np.zeros(0, np.uint8)
    planes = {}
    for j, (seed, n, kind) in C_CASES[name].items():
        alone = stream_info(oracle, c_member(seed, n))[3]
        assert len(alone) == 1 and c_kind(alone[0]) == kind and alone[0]["btype"] == (1 if kind == TIE else 2), (name, j, alone)
        planes[j] = np.concatenate([front, c_member(seed, n)])
        if len(front):
            nsym, nblocks, _, blocks = stream_info(oracle, planes[j])
            assert nblocks == 2 and blocks[0]["end"] == len(front) and nsym > BLK_SYMS, (name, j, nsym, nblocks)
            assert all(blocks[1][f] == alone[0][f] for f in ("btype", "opt_len", "static_len")), (name, j, blocks[1], alone[0])
            assert raw_diff(oracle, planes[j]) > 0
    return words_of(planes, len(next(iter(planes.values()))))


def c_conditions(oracle):
    kinds = [kind for name, lanes in C_CASES.items() if not name.endswith("second-block") for _, _, kind in lanes.values()]
    assert kinds.count(TIE) >= 3 and kinds.count(NEXT) >= 3
    for name in C_CASES:
        c_case(oracle, name)


# ------------------------------------------------------------------ G: the window slides
# the final block of a plane of n bytes is flushed after every slide, and slide k happens once n >= 65274 + 32768 (k - 1):
# stored_ok of the final block flips where its start lies below 32768 k.  98301 | 98302 is the other kind of flip: the first
# byte of a new final block.
G_PAIRS = ((65273, 65274), (98041, 98042), (98301, 98302), (130809, 130810))
G_BYTES = 131072


@functools.lru_cache(maxsize=None)
def g_noise(seed: int) -> np.ndarray:
    p = noise(seed, G_BYTES)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def g_runs_late() -> np.ndarray:
    """a first block of noise alone, so the second starts at 32767 as in a noise plane, then noise with a five-byte run every
    8000 positions (more, and the final block would no longer be stored where it may be): symbols and positions diverge, and
    the run over 65268 ... 65279 makes a match, not a literal, step to position 65274"""
    p = noise(8, G_BYTES)
    for a in range(36000, 65000, 8000):
        p[a: a + 5] = 0xEE
    p[65268: 65280] = 0xEE
    p.setflags(write=False)
    return p


G_RUNS_FRONT = (10967, 10900)        # literals, five-byte runs: 32767 symbols over 65467 positions


@functools.lru_cache(maxsize=None)
def g_runs_front() -> np.ndarray:
    """a first block that spans 65467 positions (noise, then five-byte runs), then noise: at 98042 and 130810 the final block
    is one block earlier than in a noise plane, and a new block starts at 98235, not at 98302"""
    lit, runs = G_RUNS_FRONT
    p = np.concatenate([noise(9, lit), five_runs(runs), noise(10, 140000 - lit - 5 * runs)])
    p.setflags(write=False)
    return p


def g_runs_front_pair(oracle):
    """the lengths at which the third block of g_runs_front() gets its first byte"""
    blocks = stream_info(oracle, g_runs_front())[3]
    assert 65274 < blocks[0]["end"] < 65536 and blocks[1]["end"] == blocks[0]["end"] + BLK_SYMS, blocks[:2]
    return blocks[1]["end"], blocks[1]["end"] + 1


G_START_ON_SLIDE = "start-on-slide"
G_START_ON_SLIDE_BYTES = 98100       # two slides (>= 98042), the third block still the last (< 98304)


@functools.lru_cache(maxsize=None)
def g_start_on_slide() -> np.ndarray:
    """noise with one run of four bytes (a literal and a match of three) in the first block: two full blocks span 65536
    positions, and the third starts exactly where the window stands after its second slide: start == 32768 * 2, the tie of
    stored_ok itself"""
    p = noise(13, G_BYTES)
    p[1000: 1004] = 0xEE
    p.setflags(write=False)
    return p


def g_names(oracle=None):
    return [str(n) for pair in G_PAIRS for n in pair] + ["runs-new-block-0", "runs-new-block-1", G_START_ON_SLIDE]


def g_members(oracle, name: str):
    """(n, lane -> source plane) of case G-name"""
    if name == G_START_ON_SLIDE:
        n = G_START_ON_SLIDE_BYTES
        blocks = stream_info(oracle, g_start_on_slide()[:n])[3]
        assert len(blocks) == 3 and blocks[2]["start"] == 65536 and (blocks[2]["btype"], blocks[2]["stored_ok"]) == (0, 1), blocks
        # that the window has slid twice at this length: the noise plane's last block starts two positions earlier and is
        # not allowed to be stored
        other = stream_info(oracle, g_noise(3)[:n])[3]
        assert len(other) == 3 and other[2]["start"] == 65534 and other[2]["stored_ok"] == 0, other
        return n, {0: g_noise(3), 2: g_start_on_slide()}
    if name.startswith("runs-new-block"):
        return g_runs_front_pair(oracle)[int(name[-1])], {0: g_noise(3), 2: g_runs_front()}
    n = int(name)
    third = g_runs_late() if n < 70000 else g_noise(5) if n in G_PAIRS[2] else g_runs_front()
    return n, {0: g_noise(3), 1: g_noise(4), 2: third}


def g_final(oracle, plane) -> tuple:
    nsym, nblocks, _, blocks = stream_info(oracle, plane)
    return blocks[-1]["btype"], blocks[-1]["stored_ok"], nblocks, nsym


def g_case(oracle, name: str) -> np.ndarray:
    n, src = g_members(oracle, name)
    return words_of({j: p[:n] for j, p in src.items()}, n)


def g_conditions(oracle):
    pairs = [(str(a), str(b)) for a, b in G_PAIRS] + [("runs-new-block-0", "runs-new-block-1")]
    for a, b in pairs:
        (na, sa), (nb, sb) = g_members(oracle, a), g_members(oracle, b)
        assert nb == na + 1 and sorted(sa) == sorted(sb)
        for j in sa:
            if a.startswith("runs") and j == 0:
                continue                                       # noise beside the plane with runs: on no edge at this length
            fa, fb = g_final(oracle, sa[j][:na]), g_final(oracle, sb[j][:nb])
            assert fa[:2] != fb[:2], (a, b, j, fa, fb)
            if na in (65273, 98041, 130809):                   # a slide: stored and allowed, then not allowed
                assert fa[:2] == (0, 1) and fb[1] == 0 and fa[2] == fb[2], (a, j, fa, fb)
            else:                                              # a new block of one literal
                assert fb[2] == fa[2] + 1 and fb[:2] == (1, 1) and fa[3] == fa[2] * BLK_SYMS, (a, j, fa, fb)
    g_members(oracle, G_START_ON_SLIDE)
    # the planes with runs are where symbols and positions diverge
    assert g_final(oracle, g_runs_late()[:65274])[3] <= 65274 - 4 * 3 - 4
    assert g_final(oracle, g_runs_front()[:98042])[2] == 2 and g_final(oracle, g_noise(3)[:98042])[2] == 3
    assert g_final(oracle, g_runs_front()[:130810])[2] == 3 and g_final(oracle, g_noise(3)[:130810])[2] == 4


# ------------------------------------------------------------------ F: the block boundary, counted in symbols
# name -> (nsym, leading literals).  Five-byte runs are a literal and a match each; with an odd number of literals in front
# the last symbol of every full block is a match.
F_CASES = {"32766": (32766, 0), "32767-match-last": (32767, 1), "32768": (32768, 0), "65534": (65534, 0),
           "65535-match-last": (65535, 1)}
F_STORED_FULL = "65534-stored-full"
F_STORED_FULL_FRONT = (11095, 10836)    # literals, five-byte runs: 32767 symbols over 65275 positions


def f_stored_full_plane() -> np.ndarray:
    """A first block of 65275 positions and a second of 32767 noise literals: 98042 bytes, two full blocks, and the window's
    second slide falls on position 98042 itself, behind the flush of the second block.  A block flushed inside the loop sees
    one slide and may be stored (65275 >= 32768); had it been taken for a partial last block, flushed after the loop, it would
    see two and could not (65275 < 65536)."""
    lit, runs = F_STORED_FULL_FRONT
    return np.concatenate([noise(9, lit), five_runs(runs), noise(12, BLK_SYMS)])


def f_plane(name: str) -> np.ndarray:
    if name == F_STORED_FULL:
        return f_stored_full_plane()
    nsym, lead = F_CASES[name]
    assert (nsym - lead) % 2 == 0
    return five_runs((nsym - lead) // 2, lead)


def f_names():
    return list(F_CASES) + [F_STORED_FULL]


def f_case(oracle, name: str) -> np.ndarray:
    plane = f_plane(name)
    nsym, nblocks, nmatch, blocks = stream_info(oracle, plane)
    if name == F_STORED_FULL:
        assert (nsym, nblocks, len(plane)) == (2 * BLK_SYMS, 2, 65274 + 32768), (nsym, nblocks, len(plane))
        assert 32768 <= blocks[1]["start"] < 65536 and (blocks[1]["btype"], blocks[1]["stored_ok"]) == (0, 1), blocks[1]
        # one byte less and the same block is the partial last one: flushed after the loop, before that slide, stored too;
        # one byte more and it is followed by a block of one literal
        assert g_final(oracle, plane[:-1])[:3] == (0, 1, 2)
        return words_of({2: plane, 0: five_runs(len(plane) // 5 + 1)[:len(plane)]}, len(plane))
    want, lead = F_CASES[name]
    assert nsym == want and nmatch == (want - lead) // 2, (name, nsym, nmatch)
    assert nblocks == (want + BLK_SYMS - 1) // BLK_SYMS, (name, nblocks)
    if want % BLK_SYMS == 1:
        assert blocks[-1]["end"] - blocks[-1]["start"] in (1, 4) and blocks[-1]["btype"] == 1, blocks[-1]      # one symbol
    if lead & 1:                                                # the first block ends with a match of four
        assert plane[blocks[0]["end"] - 1] == plane[blocks[0]["end"] - 5] != plane[blocks[0]["end"] - 6]
    return words_of({2: plane}, len(plane))


def f_conditions(oracle):
    for name in f_names():
        f_case(oracle, name)
    assert sorted(v[0] for v in F_CASES.values()) == [32766, 32767, 32768, 65534, 65535]
    assert sum(1 for v in F_CASES.values() if v[1] & 1 and v[0] >= BLK_SYMS) >= 2      # a full block that ends with a match


# ------------------------------------------------------------------ D: a full-size chunk at the RAW threshold (GPU only)
# m -> zlen - CHK of a 6291456-byte noise plane whose last m bytes are zero (bisected on the oracle: zlen crosses CHK - 5 at
# m = 7756).  COMPRESSED iff CHK > min(zlen, CHK) + 4: -5 and below.  m = 0: zlen above CHK, the cap.
D_M = {7757: -6, 7756: -5, 7755: -4, 7752: -1, 7751: 0, 0: None}
D_LANE = 2


@functools.lru_cache(maxsize=None)
def d_noise() -> np.ndarray:
    p = np.random.default_rng(1).integers(0, 256, CHK).astype(np.uint8)
    p.setflags(write=False)
    return p


def d_plane(m: int) -> np.ndarray:
    p = d_noise().copy()
    if m:
        p[CHK - m:] = 0
    return p


def d_case(oracle, m: int) -> np.ndarray:
    """the member's words; its zlen - CHK is asserted by d_check_header from the container the check builds anyway"""
    return words_of({D_LANE: d_plane(m)}, CHK)


def d_check_header(oracle, m: int, z: bytes):
    plane = d_plane(m)
    zlen = len(oracle.deflate(plane))
    if D_M[m] is None:
        assert zlen > CHK, (m, zlen)
    else:
        assert zlen - CHK == D_M[m], (m, zlen - CHK, D_M[m])
    raw, paylen = chunk_headers(z, CHK)[0][D_LANE]
    assert raw == (zlen - CHK >= -4), (m, zlen - CHK, raw)
    assert paylen == (CHK if raw else zlen)


def d_conditions():
    diffs = [d for d in D_M.values() if d is not None]
    assert sorted(diffs) == [-6, -5, -4, -1, 0] and None in D_M.values()


# ------------------------------------------------------------------ E: SURVEY App. C-1 (GPU only)
E_TAIL = 1000


@functools.lru_cache(maxsize=None)
def e_words() -> np.ndarray:
    """A full-size incompressible chunk, a compressible one, and a short incompressible one in one file.  This is the shape of
    SURVEY App. C-1, where the reference binary itself diverges: its encoder state carries over from the chunk that hit the
    output cap.  This codec and the oracle deliberately code every chunk with fresh state, so the reference binary must not be
    consulted for this input; the oracle's container round-trips through the oracle."""
    w = np.concatenate([whole.random_words(CHK, 31), np.full(CHK, 0x41200000, np.uint32), whole.random_words(E_TAIL, 32)])
    w.setflags(write=False)
    return w


def e_check_headers(oracle, z: bytes):
    w = e_words()
    hdr = chunk_headers(z, len(w))
    assert [[raw for raw, _ in c] for c in hdr] == [[True] * 4, [False] * 4, [True] * 4], hdr
    assert oracle.uncompress(z) == w.tobytes()
