"""Inputs shared by test_gpu_emit_mixed.py and its emulator twin test_sim_emit_mixed.py: planes in which runs and literals
are mixed, which is the path of k_emit that reads a match's bits from the block's length table and appends two symbols at a
time.  One byte plane of the words carries the pattern, the other three are constant.  Every expectation is the oracle's
container; what a case is meant to reach (a block type, a code length, a lane's symbol count) is asserted from the oracle's
bytes or from the plane with the helpers below, so that a case cannot silently stop covering it.

Buffers are pre-filled with emit_whole_words_cases.PATTERN, as in the whole-word tests."""
import struct

import numpy as np

PLANE = 2                    # the byte plane that carries the pattern
CONST = 0x41000041           # the other planes' bytes
RUN_VALUES = np.arange(0x10, 0x30, dtype=np.uint8)      # bytes of the runs ...
SEP_VALUES = np.arange(0x80, 0x87, dtype=np.uint8)      # ... and of the single bytes between them (disjoint)


def words_of(plane: np.ndarray) -> np.ndarray:
    return (np.uint32(CONST & ~(0xff << (8 * PLANE))) | (plane.astype(np.uint32) << np.uint32(8 * PLANE))).astype(np.uint32)


def plane_stream(container: bytes, plane: int = PLANE, chunk: int = 0) -> bytes:
    """the payload of one plane of one chunk record of a container (17-byte file header, then per chunk 4 lengths + payloads)"""
    off = 17
    for _ in range(chunk):
        off += 16 + sum(x & 0x7fffffff for x in struct.unpack("<4I", container[off: off + 16]))
    lens = struct.unpack("<4I", container[off: off + 16])
    assert not lens[plane] & 0x80000000, "the plane was stored RAW"
    a = off + 16 + sum(x & 0x7fffffff for x in lens[:plane])
    return container[a: a + lens[plane]]


# ------------------------------------------------------------------ the symbols of a plane (SURVEY App. B.2 closed form)
def symbol_starts(plane: np.ndarray):
    """(S, M): positions that start a symbol / a match of the Z_RLE parse.  In a maximal run [s, t), d = p - s, f = t - p:
    d == 0 literal; m = (d - 1) % 258: m == 0 -> match of min(258, f) if f >= 3, else literal; m == 1 -> literal iff f == 1."""
    n = len(plane)
    E = np.ones(n, bool)
    E[1:] = plane[1:] != plane[:-1]
    idx = np.arange(n)
    s = np.maximum.accumulate(np.where(E, idx, 0))
    nxt = np.where(E, idx, n)
    t = np.minimum.accumulate(np.append(nxt[1:], n)[::-1])[::-1]
    d, f = idx - s, t - idx
    m = (d - 1) % 258
    S = (d == 0) | ((d > 0) & (m == 0)) | ((d > 0) & (m == 1) & (f == 1))
    M = (d > 0) & (m == 0) & (f >= 3)
    return S, M


def quarter_counts(S: np.ndarray) -> np.ndarray:
    """symbol starts per 16-position quarter, as [tile, lane, quarter] (the plane padded to whole tiles)"""
    pad = (-len(S)) % 4096
    return np.append(S, np.zeros(pad, bool)).reshape(-1, 64, 4, 16).sum(axis=3)


# ------------------------------------------------------------------ a raw-deflate block walker
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DEXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
_CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _table(lengths):
    """decode table of a canonical code: index = the next maxlen bits of the stream (LSB first) -> (symbol, length)"""
    maxlen = max(lengths)
    count = [0] * (maxlen + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (maxlen + 2)
    for b in range(1, maxlen + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    tab = [None] * (1 << maxlen)
    for sym, l in enumerate(lengths):
        if l:
            c, r = nxt[l], 0
            nxt[l] += 1
            for _ in range(l):
                r, c = (r << 1) | (c & 1), c >> 1
            for k in range(r, 1 << maxlen, 1 << l):
                tab[k] = (sym, l)
    return tab, maxlen


def walk_blocks(z: bytes):
    """The blocks of a raw deflate stream up to its end (the reference ends a stream with Z_FULL_FLUSH: an empty stored
    block, not BFINAL): a list of (btype, symbols without END_BLOCK | stored bytes, literal/length code lengths or None)."""
    buf = bytes(z) + b"\0" * 8
    pos, out, nbits = 0, [], 8 * len(z)

    def bits(n):
        nonlocal pos
        v = (int.from_bytes(buf[pos >> 3: (pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(tab, maxlen):
        nonlocal pos
        s, l = tab[(int.from_bytes(buf[pos >> 3: (pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << maxlen) - 1)]
        pos += l
        return s

    while pos + 3 <= nbits:
        final, btype = bits(1), bits(2)
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            assert n ^ nn == 0xffff
            pos += 8 * n
            out.append((0, n, None))
        else:
            if btype == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CLORD[i]] = bits(3)
                ctab, cmax = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = sym(ctab, cmax)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    elif s == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                ll, dl = lens[:hlit], lens[hlit:]
            ltab, lmax = _table(ll)
            dtab, dmax = _table(dl) if any(dl) else (None, 0)
            nsym = 0
            while True:
                s = sym(ltab, lmax)
                if s == 256:
                    break
                nsym += 1
                if s > 256:
                    pos += _LEXTRA[s - 257]
                    d = sym(dtab, dmax)
                    pos += _DEXTRA[d]
            out.append((btype, nsym, list(ll) + [0] * (286 - len(ll))))
        if final:
            break
    return out


# ------------------------------------------------------------------ cases 1 and 2: run lengths, alignment
def run_set(shuffled: bool, shift: int = 0) -> np.ndarray:
    """runs of every length 1..600 (ascending, or shuffled with a fixed seed), single distinct bytes between them, behind
    `shift` bytes that are all different from their neighbours.  Lengths 1 and 2 have no match; 3..10 and every extra-bits
    class; 259, 260, 261 and longer split into matches of 258 and a remainder, which is one or two literals for some."""
    lens = np.arange(1, 601)
    if shuffled:
        lens = np.random.default_rng(20240611).permutation(lens)
    parts = [(0xc0 + (np.arange(shift) & 1)).astype(np.uint8)]
    for k, l in enumerate(lens.tolist()):
        parts.append(np.full(l, RUN_VALUES[k % len(RUN_VALUES)], np.uint8))
        parts.append(SEP_VALUES[k % len(SEP_VALUES): k % len(SEP_VALUES) + 1])
    return np.concatenate(parts)


SHIFTS = (0, 1, 15, 16, 17, 63)


# ------------------------------------------------------------------ case 3: pairing
def pairing_plane() -> np.ndarray:
    """Literals everywhere (16 symbols in every quarter of every lane), except:
    tile 1, quarter 1: lanes 3 / 5 / 7 / 9 hold 0 / 1 / 2 / 3 symbols there (a run from the quarter before covers the rest);
    tile 2, quarter 2: lane 20 alone has a match, every other lane of the wave 16 literals (where the literal path of a
    quarter and the mixed one meet)."""
    rng = np.random.default_rng(77)
    p = rng.integers(0, 200, 4 * 4096).astype(np.uint8)
    same = np.flatnonzero(p[1:] == p[:-1]) + 1
    while len(same):
        p[same] = (p[same] + 1) % 200
        same = np.flatnonzero(p[1:] == p[:-1]) + 1
    t1 = 4096
    a = t1 + 64 * 3
    p[a + 10: a + 40] = 250                               # literal at 10, match 11..39: nothing starts in 16..31
    a = t1 + 64 * 5
    p[a + 10: a + 31] = 251; p[a + 31: a + 41] = 252      # one symbol (the literal at 31)
    a = t1 + 64 * 7
    p[a + 10: a + 30] = 251; p[a + 30: a + 45] = 252      # two: the literal at 30 and its match at 31
    a = t1 + 64 * 9
    p[a + 10: a + 29] = 251; p[a + 29] = 253; p[a + 30: a + 45] = 252   # three
    a = 2 * 4096 + 64 * 20
    p[a + 36: a + 40] = 254                               # literal at 36, match of 3 at 37
    return p


def check_pairing_plane(p: np.ndarray):
    S, M = symbol_starts(p)
    c = quarter_counts(S)
    assert [int(c[1, l, 1]) for l in (3, 5, 7, 9)] == [0, 1, 2, 3] and int(c[1, 4, 1]) == 16
    m = quarter_counts(M)
    assert int(m[2, 20, 2]) == 1 and int(m[2, :, 2].sum()) == 1 and int((c[2, :, 2] == 16).sum()) == 63


# ------------------------------------------------------------------ case 4: block boundary
BLK_SYMS = 32767


def boundary_plane(second: str) -> np.ndarray:
    """Short runs (1..6 bytes of eight values), more than 32767 symbols; the last symbol of the first block is a match, so
    the block changes inside a tile and inside a run.  `second`: "dynamic" = a second block of the same kind, "static" = a
    few more symbols, all different, "stored" = noise behind the boundary."""
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 7, 30000)
    vals = rng.integers(0, 8, 30000)
    vals[1:][vals[1:] == vals[:-1]] += 8                  # most equal neighbours are told apart; the rest merge into longer runs
    body = np.repeat(vals.astype(np.uint8), lens)
    for lead in range(64):                                # single literals in front shift the symbol numbering
        p = np.concatenate([(0xe0 + (np.arange(lead) & 1)).astype(np.uint8), body])
        S, M = symbol_starts(p)
        starts = np.flatnonzero(S)
        if len(starts) > BLK_SYMS + 40 and M[starts[BLK_SYMS - 1]] and starts[BLK_SYMS - 1] % 4096 not in (0, 4095):
            break
    else:
        raise AssertionError("no lead puts a match at the block boundary")
    cut = int(starts[BLK_SYMS])                           # first position of the second block
    if second == "dynamic":
        return p
    if second == "static":  # many different bytes once each (a dynamic header would cost more than it saves) and a few short runs
        tail = [np.array([20 + 3 * k], np.uint8) for k in range(45)]
        for k in range(5):
            tail.insert(8 * k + 3, np.full(4 + k, 200 + k, np.uint8))
        return np.concatenate([p[:cut]] + tail)
    assert second == "stored"
    noise = np.random.default_rng(9).integers(0, 256, 3000).astype(np.uint8)
    while noise[0] == p[cut - 1]:
        noise[0] += 1
    return np.concatenate([p[:cut], noise])


BOUNDARY_TYPES = {"dynamic": [2, 2], "static": [2, 1], "stored": [2, 0]}


def check_boundary(plane: np.ndarray, stream: bytes, second: str):
    blocks = [b for b in walk_blocks(stream)]
    assert [b[0] for b in blocks[:2]] == BOUNDARY_TYPES[second], [b[:2] for b in blocks]
    assert blocks[0][1] == BLK_SYMS
    S, M = symbol_starts(plane)
    assert M[np.flatnonzero(S)[BLK_SYMS - 1]], "the first block does not end with a match"


# ------------------------------------------------------------------ case 5: long codes
def long_code_plane():
    """One block whose literal/length counts grow a little faster than Fibonacci numbers (c[k] = c[k-1] + c[k-2] + 1: the
    Huffman tree is one chain, deeper than 15, which zlib then limits to 15 bits).  The rare symbols are END_BLOCK, two run
    bytes and the length codes of their runs (131..194 bytes: five extra bits), so a run's literal and its match take about
    15 + (15 + 5 + 1) bits; most runs start on a quarter's first position, where the two are appended as one pair."""
    counts = [1, 1]                                       # END_BLOCK, length code 281
    while len(counts) < 19:
        counts.append(counts[-1] + counts[-2] + 1)        # 3 = byte 0xf0, 5 = length code 282, 9 = byte 0xf1, then the fillers
    left = dict(zip(range(100, 114), counts[5:]))         # filler literals: byte value -> how many are still to place
    order, prev = [], -1
    while left:
        v = max((k for k in left if k != prev), key=lambda k: left[k])
        order.append(v)
        left[v] -= 1
        if not left[v]:
            del left[v]
        prev = v
        if len(left) == 1 and next(iter(left)) == prev:
            break                                         # (the most frequent byte cannot follow itself: the rest is dropped)
    f0, f1 = 0xf0, 0xf1
    todo = [(f0, 140), (f1, 170), (f0, 1), (f1, 170), (f1, 1), (f1, 170), (f0, 1), (f1, 1), (f1, 170), (f1, 1), (f1, 170), (f1, 1)]
    out, k, gap, pos = [], 0, len(order) // (len(todo) + 1), 0
    for i, v in enumerate(order):
        if k < len(todo) and i >= (k + 1) * gap and (todo[k][1] == 1 or pos % 16 == (1 if k == 5 else 0)):
            out.append(np.full(todo[k][1], todo[k][0], np.uint8))
            pos += todo[k][1]
            k += 1
        out.append(np.array([v], np.uint8))
        pos += 1
    assert k == len(todo)
    return np.concatenate(out)


def check_long_codes(plane: np.ndarray, stream: bytes):
    """the block is dynamic, holds 15-bit codes, and some quarter's first two symbols are a literal and a match of more than
    32 bits together"""
    btype, nsym, ll = walk_blocks(stream)[0]
    assert btype == 2 and max(ll) == 15
    S, M = symbol_starts(plane)
    wide = 0
    for p in np.flatnonzero(M).tolist():
        if p % 16 == 1 and S[p - 1]:
            t = p
            while t < len(plane) and plane[t] == plane[p]:
                t += 1
            code = 257 + max(i for i, b in enumerate(_LBASE) if b <= min(t - p, 258))
            assert _LEXTRA[code - 257] == 5
            wide += ll[plane[p - 1]] + ll[code] + 5 + 1 > 32
    assert wide > 0
