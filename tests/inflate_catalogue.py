"""Decoder conformance catalogue: containers whose plane streams are hand-built raw DEFLATE (tests/deflate_writer.py) or come
from the system zlib with other parameters than the reference's, each with the words it must decode to.  Built at test time
from fixed seeds; every stream is inflated by zlib here and must give exactly its plane, so a writer bug cannot pass.

Each stream carries the decode class that the header comment of csrc/mrcz_inflate_par.hip predicts for it:
  "par"    the block chain closes in parallel (k_scan_candidates / k_blk_count / k_chain): counts in neither fall-back;
  "chain"  the chain does not close and k_inflate_par decodes the stream block after block: +1 chain fall-back;
  "seq"    k_inflate_par hands the stream to the sequential k_inflate (general distances, tokens past MAXTOK):
           +1 chain fall-back and +1 (sequential) fall-back;
  "raw"    a RAW plane: no stream at all;
  None     not predicted (only the bytes are checked).
The candidate pattern is a dynamic block with BFINAL 0 and HDIST field 1 (what zlib Z_RLE writes); the block at payload bit 0
is always tried, whatever its header.  Stored blocks are sized by k_chain itself (BFINAL 0 only)."""
import zlib
from dataclasses import dataclass, field

import numpy as np

import util
from deflate_writer import DIST_BASE, DeflateWriter, canonical_codes, cat, expand, inflate_raw, lits, static_lengths, toks

RLE_DIST = [1, 1]   # zlib's distance code when every match has distance 1: two 1-bit codes (HDIST field 1)
COUNTED = {"par": (0, 0), "chain": (1, 0), "seq": (1, 1), "raw": (0, 0)}


@dataclass
class Case:
    name: str
    records: bytes                    # the chunk records (no 17-byte file header)
    words: np.ndarray                 # what they decode to
    classes: list = field(default_factory=list)   # per stream (chunk-major), see above

    @property
    def container(self) -> bytes:
        return util.file_header(4 * len(self.words)) + self.records

    def expected_fallbacks(self):
        """(chain fall-backs, sequential fall-backs) the classes predict, or None where a class is not predicted"""
        if any(c is None for c in self.classes):
            return None
        return tuple(sum(COUNTED[c][i] for c in self.classes) for i in (0, 1))


class Plane:
    """one plane stream written block by block, with the bytes it decodes to"""

    def __init__(self):
        self.w = DeflateWriter()
        self.out = bytearray()

    def _grow(self, t):
        self.out += expand(t, bytes(self.out[-32768:]))

    def stored(self, data, final=False, pad=0):
        self.w.stored(data, final, pad)
        self.out += bytes(data)
        return self

    def static(self, t, final=False):
        self.w.static(t, final)
        self._grow(t)
        return self

    def dynamic(self, t, final=False, **kw):
        self.w.dynamic(t, final=final, **kw)
        self._grow(t)
        return self

    def rle(self, t, final=False, **kw):
        """a dynamic block shaped as zlib Z_RLE writes it (only distance-1 matches, two 1-bit distance codes)"""
        kw.setdefault("dist_lengths", RLE_DIST)
        return self.dynamic(t, final=final, **kw)

    @property
    def nbit(self):
        return self.w.nbit

    def finish(self):
        z = self.w.getvalue()
        return z, np.frombuffer(bytes(self.out), np.uint8)


def checked(z, plane):
    """the reference's inflater must give exactly the plane"""
    got = inflate_raw(z)
    assert got is not None and got == bytes(plane), ("zlib disagrees with the writer", None if got is None else len(got), len(plane))
    return z


def filler(n, j, seed):
    """content of the planes a case does not care about (stored RAW)"""
    rng = np.random.default_rng(seed * 4 + j)
    return rng.integers(0, 256, n, dtype=np.uint8)


def chunk(planes, streams, classes):
    for p, z in zip(planes, streams):
        if z is not None:
            checked(z, p)
    return util.chunk_record(planes, streams), planes, list(classes)


def case(name, chunks):
    recs, words, classes = bytearray(), [], []
    for k, (rec, planes, cls) in enumerate(chunks):
        assert len(planes[0]) == util.CHUNK or (k == len(chunks) - 1 and 0 < len(planes[0]) <= util.CHUNK), name
        recs += rec
        words.append(np.stack(planes, axis=1).reshape(-1).view(np.uint32))
        classes += cls
    return Case(name, bytes(recs), np.concatenate(words), classes)


def one_stream(name, plane: Plane, klass, j=1, seed=0):
    """a one-chunk case whose plane j is the hand-built stream, the other planes RAW"""
    z, p = plane.finish()
    n = len(p)
    planes = [filler(n, k, seed) if k != j else p for k in range(4)]
    streams = [z if k == j else None for k in range(4)]
    classes = [klass if k == j else "raw" for k in range(4)]
    return case(name, [chunk(planes, streams, classes)])


def skew_lengths(syms, n=286):
    """a complete code in which the listed symbols get lengths 1, 2, ..., k-1, k-1 (the last two share the longest)"""
    ll = np.zeros(n, np.int64)
    k = len(syms)
    for i, s in enumerate(syms):
        ll[s] = min(i + 1, k - 1)
    return ll


LL1 = np.zeros(286, np.int64)
LL1[[0x11, 256, 0x22, 257]] = [1, 2, 3, 3]    # a literal of 1 bit, one of 3 bits, a distance-1 match of length 3 in 4 bits


def padded_block(q, residue, modulus, nbytes=None):
    """append a block of the candidate pattern after which the stream stands at bit `residue` mod `modulus` (and that
    produces exactly `nbytes` bytes, if given): a literals of 1 bit, b of 3 bits, c distance-1 matches of 4 bits"""
    probe = DeflateWriter()
    probe.dynamic(toks(), litlen_lengths=LL1, dist_lengths=RLE_DIST)   # header and END_BLOCK
    base = q.nbit + probe.nbit
    for c in range(8):
        for b in range(8):
            a = (residue - base - 3 * b - 4 * c) % modulus if nbytes is None else nbytes - b - 3 * c
            if a >= 1 and (base + a + 3 * b + 4 * c) % modulus == residue % modulus:
                q.rle(cat(lits(b"\x11" * a + b"\x22" * b), toks(*[(3, 1)] * c)), litlen_lengths=LL1)
                assert q.nbit % modulus == residue % modulus
                return q
    raise AssertionError("no padding block")


def mixed_tokens(rng, n, alpha=16, p_match=0.15, maxlen=258):
    """literals from a small alphabet and distance-1 matches (what an RLE coder leaves); the first token is a literal"""
    out_l, out_d = [int(rng.integers(0, alpha))], [0]
    for _ in range(n - 1):
        if rng.random() < p_match:
            out_l.append(int(rng.integers(3, maxlen + 1)))
            out_d.append(1)
        else:
            out_l.append(int(rng.integers(0, alpha)) * 7 % 256)
            out_d.append(0)
    return np.array(out_l, np.int64), np.array(out_d, np.int64)


# ---------------------------------------------------------------------------------------------------------- hand-built cases
def hand_cases(big=False):
    """the hand-built catalogue; `big` scales the blocks up for the GPU (windows of 16 KiB, pieces of 256 bits)"""
    S = 16 if big else 1
    rng = np.random.default_rng(2024)
    cs = []

    def body(n, alpha=16, p=0.15):
        return mixed_tokens(rng, n * S, alpha, p)

    # ---- block types and boundaries
    cs.append(one_stream("sync_marker_first_and_between",
                         Plane().stored(b"").rle(body(300)).stored(b"").stored(b"").rle(body(200)).stored(b""), "par"))
    cs.append(one_stream("stored_1_and_65535",
                         Plane().stored(b"\x9a").rle(body(100)).stored(filler(65535, 0, 5).tobytes()).rle(body(100)).stored(b"\x01")
                         .stored(b""), "par"))
    for nrun in (1, 63, 64, 65, 129):
        p = Plane().rle(body(50))
        blen = 37 * S
        for i in range(nrun):
            p.stored(filler(blen, i, 7 + nrun).tobytes())
        cs.append(one_stream(f"stored_run_{nrun}_then_dynamic", p.rle(body(80)).stored(b""), "par"))
    p = Plane()
    for i in range(70):
        p.stored(filler(41 if i != 33 else 40, i, 9).tobytes())
    cs.append(one_stream("stored_run_broken_by_one_length", p.rle(body(60)).stored(b""), "par"))
    p = Plane().rle(body(120))
    for i in range(66):
        p.stored(filler(29, i, 10).tobytes(), pad=0x1f if i % 2 else 0x15)
    cs.append(one_stream("stored_pad_bits_set", p.stored(b"", pad=0x1f).rle(body(60)).stored(b"", pad=0x1f), "par"))
    cs.append(one_stream("static_empty_between_dynamic",
                         Plane().rle(body(200)).static(toks()).rle(body(200)).static(toks()).stored(b""), "chain"))
    cs.append(one_stream("static_with_data",
                         Plane().rle(body(150)).static(body(300)).rle(body(100)).static(cat(lits(b"Q"), toks((258, 1), (3, 1)))).stored(b""),
                         "chain"))
    cs.append(one_stream("static_first_block", Plane().static(body(300)).stored(b""), "par"))
    cs.append(one_stream("dynamic_empty_rle_shaped", Plane().rle(body(150)).rle(toks()).rle(toks()).rle(body(150)).stored(b""), "par"))
    cs.append(one_stream("dynamic_empty_no_distance_code",
                         Plane().rle(body(150)).dynamic(toks(), dist_lengths=[0]).rle(body(150)).stored(b""), "chain"))
    cs.append(one_stream("finish_bfinal_dynamic_last", Plane().rle(body(200)).rle(body(200)).rle(body(200), final=True), "chain"))
    cs.append(one_stream("finish_bfinal_single_block", Plane().rle(body(400), final=True), "par"))
    cs.append(one_stream("finish_bfinal_stored_last", Plane().rle(body(200)).stored(filler(300, 0, 3).tobytes(), final=True), "chain"))
    cs.append(one_stream("full_flush_marker_last", Plane().rle(body(200)).rle(body(200)).stored(b""), "par"))

    # ---- distance-1 replication across blocks that produce no literal
    lastlit = cat(body(200), lits(b"\xa7"))
    d1 = toks(*([(258, 1)] * (4 * S) + [(3, 1)] * 5))
    cs.append(one_stream("d1_after_empty_blocks",
                         Plane().rle(lastlit).stored(b"").rle(toks()).rle(toks(*[(258, 1)] * (3 * S))).rle(toks(*[(3, 1)] * 9)).rle(d1)
                         .rle(body(100)).stored(b""), "par"))
    cs.append(one_stream("d1_source_is_last_byte_of_a_stored_block",
                         Plane().rle(body(100)).stored(filler(500, 1, 4).tobytes() + b"\x5c").rle(toks()).stored(b"")
                         .rle(toks(*[(258, 1)] * (3 * S))).rle(toks(*[(3, 1)] * 7)).rle(body(100)).stored(b""), "par"))
    cs.append(one_stream("d1_lead_then_literals",
                         Plane().rle(lastlit).rle(cat(toks((258, 1), (200, 1)), body(150))).rle(cat(toks((5, 1)), body(150))).stored(b""),
                         "par"))

    # ---- headers outside the candidate pattern (second block: only the block at bit 0 is tried whatever its header)
    lt = cat(body(200), toks((30, 1)), body(100))
    cs.append(one_stream("hdist_0_second_block", Plane().rle(body(150)).dynamic(lt, dist_lengths=[1]).rle(body(100)).stored(b""), "chain"))
    cs.append(one_stream("hdist_0_first_block", Plane().dynamic(lt, dist_lengths=[1]).rle(body(100)).stored(b""), "par"))
    cs.append(one_stream("hdist_29_second_block", Plane().rle(body(150)).dynamic(lt, dist_lengths=RLE_DIST, hdist=30).rle(body(100))
                         .stored(b""), "chain"))
    cs.append(one_stream("hlit_257_and_286", Plane().rle(lits(rng.integers(0, 256, 300 * S, dtype=np.uint8)))
                         .rle(lt, hlit=286).rle(cat(lits(b"z"), lits(rng.integers(0, 9, 200, dtype=np.uint8)))).stored(b""), "par"))
    ll5 = np.zeros(286, np.int64)
    ll5[:255] = 8
    ll5[256] = 8
    t5 = lits(rng.integers(0, 255, 400 * S, dtype=np.uint8))
    cs.append(one_stream("hclen_5_second_block", Plane().rle(body(100)).dynamic(t5, litlen_lengths=ll5, dist_lengths=[0]).rle(body(100))
                         .stored(b""), "chain"))
    cs.append(one_stream("hclen_19_and_plain_lengths", Plane().rle(body(200), hclen="full").rle(body(200), clen_style="plain")
                         .rle(body(200), clen_style="plain", hclen="full").stored(b""), "par"))

    # ---- code lengths and tokens at the kernel's limits
    lsyms = [7 * i % 256 for i in range(1, 14)]
    llong = skew_lengths([256, 285, 257] + lsyms)                 # literals of 4..15 bits
    assert {13, 14, 15} <= set(llong[lsyms].tolist())
    seq = rng.permutation(np.repeat(np.array(lsyms), 3 * S))
    tl = cat(lits(seq.astype(np.uint8)), toks((258, 1), (3, 1)), lits(np.array(lsyms[::-1], np.uint8)), toks((3, 1)))
    cs.append(one_stream("literal_codes_13_to_15_bits", Plane().rle(body(50)).rle(tl, litlen_lengths=llong).rle(tl, litlen_lengths=llong)
                         .stored(b""), "par"))
    t_d1 = cat(body(300, p=0.0), toks(*[(258, 1)] * 40), body(100))
    # distance 1 (symbol 0) with a code of DBITS bits and longer.  Open finding: at the GPU's size (a 44 KB block, the length
    # code of 258 at 8 bits, END_BLOCK at 13) the 10-bit case goes to the sequential decoder on the GPU and on the emulator
    # alike, although no token is longer than 18 bits; the bytes are exact, the class is left unpredicted there.
    for dbits, klass in ((10, None if big else "par"), (11, "seq"), (15, "seq")):
        dlong = skew_lengths(list(range(1, dbits + 1)) + [0], 30)
        assert dlong[0] == dbits
        cs.append(one_stream(f"distance1_code_{dbits}_bits_first_block", Plane().dynamic(t_d1, dist_lengths=dlong).stored(b""), klass))
    dgen = skew_lengths([0, 1] + list(range(16, 30)), 30)          # distance codes of 3..15 bits, general distances
    assert set(dgen[24:30].tolist()) == {11, 12, 13, 14, 15}
    hist = body(300, alpha=200, p=0.0)
    far = [(20, DIST_BASE[k] + k) for k in range(16, 30)]
    src = cat(hist, lits(filler(32768, 2, 1)), toks(*far, (258, 32768), (258, 1), (40, 2), (255, 2)))
    cs.append(one_stream("distance_codes_11_to_15_bits", Plane().rle(body(60)).dynamic(src, dist_lengths=dgen).stored(b""), "seq"))
    cs.append(one_stream("general_distances_first_block", Plane().dynamic(cat(lits(b"abcdefgh"), toks((258, 8), (100, 3), (3, 2)), lits(b"z")))
                         .stored(b""), "seq"))
    for bits, klass in ((24, "par"), (25, "seq")):
        # literal/length symbol 284 (5 extra bits) has a 15-bit code, distance 1 a code of bits - 20: the token of a match of
        # length 227..257 at distance 1 is exactly `bits` long
        ll = skew_lengths([0x41, 256, 0x42, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x4b, 0x4c, 0x4d, 285, 284])
        assert ll[284] == 15
        dl = skew_lengths([1, 2, 3, 4, 5, 6][: bits - 20] + [0], 30)
        assert dl[0] == bits - 20
        tt = cat(lits(b"AB" * 20), toks((227, 1), (257, 1), (240, 1), (258, 1)), lits(b"CDEFGHIJKLM"), toks((230, 1)), lits(b"A"))
        cs.append(one_stream(f"distance1_token_{bits}_bits", Plane().dynamic(tt, litlen_lengths=ll, dist_lengths=dl).stored(b""), klass))
    cs.append(one_stream("overlapping_copies", Plane().rle(body(100)).dynamic(cat(lits(b"xyz01"), toks((258, 5), (100, 3), (4, 2)),
                                                                               lits(b"q"), toks((258, 1))), dist_lengths=None)
                         .stored(b""), "seq"))

    # ---- bit alignment: the same pair of blocks behind a first block of every length mod 256 bits (the pair's header, and
    # tokens that straddle the 256-bit lane pieces, at every offset; at the GPU's size the blocks span 16 KiB windows too)
    pair = (mixed_tokens(rng, 30 * S, 40, 0.2), mixed_tokens(rng, 23 * S, 200, 0.1))
    p = Plane()
    for r in range(256):
        padded_block(p, r, 256)
        p.rle(pair[0]).rle(pair[1])
    cs.append(one_stream("pair_at_every_bit_residue", p.stored(b""), "par", j=2))

    # ---- END_BLOCK on the payload's last byte, the next plane's payload right behind it (four planes of one length whose
    # streams all end on a byte boundary, no sync marker)
    qs = [Plane().rle(body(150 + 40 * t)) for t in range(4)]
    target = max(len(q.out) for q in qs) + 30
    for q in qs:
        padded_block(q, 0, 8, nbytes=target - len(q.out))
    fin = [q.finish() for q in qs]
    cs.append(case("end_block_on_last_byte_next_payload_behind", [chunk([x[1] for x in fin], [x[0] for x in fin], ["par"] * 4)]))
    return cs


def mutation_catchers(big=False):
    """minimal streams for single mistakes of k_chain's speculation (each one decodes right only if the check it aims at holds)"""
    cs = []
    # A byte-aligned STATIC block behind a run of stored blocks of length L, whose bits 8..39 read as LEN = L, NLEN = ~L: only
    # the stored-run speculation's BTYPE test ((h0 & 7) == 0) keeps it from being copied as a stored block.
    sl, _ = static_lengths()
    table = {(int(l), int(c)): sym for sym, (l, c) in enumerate(zip(sl, canonical_codes(sl)))}

    def literals_of(bits):
        """bits 3..39 parsed as fixed literal/length codes: the literals, if they are all literals (the last code may run past
        bit 39: it is completed to some literal)"""
        pos, syms = 3, []
        while pos < 40:
            v, l = 0, 0
            while (l, v) not in table and pos + l < 40:
                v = (v << 1) | ((bits >> (pos + l)) & 1)
                l += 1
            if (l, v) not in table:      # a prefix cut at bit 40
                done = [sym for (cl, cv), sym in table.items() if sym < 256 and cl > l and cv >> (cl - l) == v]
                return syms + done[:1] if done else None
            if table[(l, v)] >= 256:
                return None
            syms.append(table[(l, v)])
            pos += l
        return syms
    found = None
    for L in range(64, 4000):
        for h in range(32):
            t = [L & 255, L >> 8, (L ^ 0xffff) & 255, (L ^ 0xffff) >> 8]
            syms = literals_of(2 | h << 3 | sum(t[k] << (8 + 8 * k) for k in range(4)))
            if syms:
                found = L, syms
                break
        if found:
            break
    L, syms = found
    p = Plane()
    p.stored(filler(L, 0, 21).tobytes()).stored(filler(L, 1, 21).tobytes())
    p.static(cat(lits(bytes(syms)), lits(bytes([200 + k % 50 for k in range(L - len(syms))]))))  # 9-bit codes: longer than L + 5 bytes
    z, plane = p.finish()
    assert z[2 * (L + 5)] & 7 == 2
    assert (z[2 * (L + 5) + 1] | z[2 * (L + 5) + 2] << 8) == L and (z[2 * (L + 5) + 3] | z[2 * (L + 5) + 4] << 8) == L ^ 0xffff
    cs.append(one_stream("static_block_looking_like_a_stored_run", p, "chain"))
    return cs


# ---------------------------------------------------------------------------------------------------------- python-zlib sweep
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}
FLUSH_MODES = ("full", "finish", "sync", "partial")


def sweep_plane(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "lowent":
        return (rng.integers(0, 4, n) * 0x41).astype(np.uint8)
    if kind == "fib":
        fib = [1, 1]
        while len(fib) < 20:
            fib.append(fib[-1] + fib[-2])
        p = np.array(fib[::-1], np.float64)
        return rng.choice(np.arange(20, dtype=np.uint8) * 13, n, p=p / p.sum())
    # long repeats: runs, and copies of earlier stretches
    out = np.repeat(rng.integers(0, 256, n // 500 + 1, dtype=np.uint8), 500)[:n].copy()
    for a in range(0, n - 2000, 3000):
        out[a + 1000: a + 1600] = out[a: a + 600]
    return out


def sweep_combos():
    for level in (0, 1, 6, 9):
        for strat in STRATEGIES:
            for mem in (1, 8, 9):
                for wb in (9, 15):
                    for fl in FLUSH_MODES:
                        yield level, strat, mem, wb, fl


def sweep_stream(plane, level, strat, mem, wb, fl, every):
    if fl in ("sync", "partial"):
        return util.python_zlib_stream(plane, level, STRATEGIES[strat], mem, wb, fl, every)
    return util.python_zlib_stream(plane, level, STRATEGIES[strat], mem, wb, fl)


def sweep_cases(combos, n, every):
    """four combinations per chunk (one per plane), the input kinds in turn; predicted class only where the header says:
    Z_RLE at level >= 1 with the reference's flush leaves distance-1 blocks of the candidate pattern"""
    kinds = ("random", "lowent", "fib", "repeats")
    combos = list(combos)
    out = []
    for c0 in range(0, len(combos), 4):
        group = combos[c0: c0 + 4]
        while len(group) < 4:
            group.append(group[0])
        planes, streams, classes = [], [], []
        for j, (level, strat, mem, wb, fl) in enumerate(group):
            p = sweep_plane(kinds[(c0 // 4 + j) % 4], n, seed=c0 + j)
            z = sweep_stream(p, level, strat, mem, wb, fl, every)
            planes.append(p)
            streams.append(checked(z, p))
            classes.append(None)
        name = "zlib_" + "_".join(f"{l}{s[:3]}m{m}w{w}{f[:2]}" for l, s, m, w, f in group)
        out.append(case(name, [chunk(planes, streams, classes)]))
    return out


# ---------------------------------------------------------------------------------------------------------- mixed chunks
def mixed_container(short_tail):
    """two chunks (the second one short) whose planes fall into every decode class: parallel, chain fall-back, sequential, RAW"""
    n0, n1 = util.CHUNK, short_tail
    rng = np.random.default_rng(99)

    def plane(n, seed):
        p = np.zeros(n, np.uint8)
        r = np.random.default_rng(seed)
        for a in r.integers(0, n - 3000, 6):
            p[a: a + 2000] = r.integers(0, 8, 2000, dtype=np.uint8) * 3
        return p

    def par(p):
        return util.python_zlib_stream(p, 6, zlib.Z_RLE, 9, 15, "full")

    def chain(p):   # Z_PARTIAL_FLUSH leaves empty static blocks: distance-1 matches only, but the chain does not close
        return util.python_zlib_stream(p, 6, zlib.Z_RLE, 9, 15, "partial", every=65536)

    def seq(p):
        return util.python_zlib_stream(p, 6, zlib.Z_DEFAULT_STRATEGY, 9, 15, "full")

    ch = []
    for n, order, seed in ((n0, ("par", "chain", "seq", "raw"), 1), (n1, ("raw", "seq", "par", "chain"), 2)):
        planes, streams = [], []
        for j, k in enumerate(order):
            p = plane(n, seed * 10 + j) if k != "raw" else rng.integers(0, 256, n, dtype=np.uint8)
            if k == "seq":
                p[n // 2: n // 2 + 700] = p[100: 800] = np.arange(700) % 251  # a repeat at a general distance
            planes.append(p)
            streams.append({"par": par, "chain": chain, "seq": seq, "raw": lambda _p: None}[k](p))
        ch.append(chunk(planes, streams, order))
    return case(f"mixed_chunks_tail{short_tail}", ch)
