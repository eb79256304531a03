"""A small raw-DEFLATE writer (RFC 1951) for decoder conformance tests: stored, static and dynamic blocks with every header
field under the caller's control.  Pure Python + numpy; meant to be obviously right rather than fast or small.

A token array pair (L, D) describes a block's contents: D == 0 is the literal byte L, D > 0 a match of length L (3..258) at
distance D (1..32768).  `toks(...)` and `lits(...)` build them.  END_BLOCK is added by the block writers.  Nothing here is
trusted on its own: tests inflate every stream with zlib (`inflate_raw`) and compare with the intended bytes."""
import heapq
import zlib

import numpy as np

# RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 for k in range(2, 28)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
END_BLOCK = 256

_LSYM = np.zeros(259, np.int64)      # match length -> length symbol 257..285
for _i, _b in enumerate(LEN_BASE):
    _LSYM[_b:] = 257 + _i
_LSYM[258] = 285                     # 258 has a code of its own (284 + 31 would say 258 too, zlib never writes that)


def static_lengths():
    """RFC 1951 3.2.6: the fixed literal/length and distance code lengths"""
    ll = np.zeros(288, np.int64)
    ll[0:144], ll[144:256], ll[256:280], ll[280:288] = 8, 9, 7, 8
    return ll, np.full(30, 5, np.int64)


def toks(*items):
    """tokens from ints (literals) and (length, distance) tuples"""
    L = np.array([t[0] if isinstance(t, tuple) else t for t in items], np.int64)
    D = np.array([t[1] if isinstance(t, tuple) else 0 for t in items], np.int64)
    return L, D


def lits(data):
    b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.astype(np.uint8)
    return b.astype(np.int64), np.zeros(len(b), np.int64)


def cat(*ts):
    return np.concatenate([t[0] for t in ts]), np.concatenate([t[1] for t in ts])


def expand(tokens, history=b""):
    """the bytes a token array produces after `history` (the slow, plain LZ77 definition)"""
    out = bytearray(history)
    for l, d in zip(tokens[0].tolist(), tokens[1].tolist()):
        if d == 0:
            out.append(l)
        else:
            assert 3 <= l <= 258 and 1 <= d <= len(out), (l, d, len(out))
            for _ in range(l):
                out.append(out[-d])
    return bytes(out[len(history):])


def symbols(tokens):
    """(length symbol or literal, its extra value, extra bits, distance symbol or -1, its extra value, extra bits)"""
    L, D = tokens
    m = D > 0
    ls = np.where(m, _LSYM[np.clip(L, 0, 258)], L)
    lb = np.asarray(LEN_BASE + [0], np.int64)[np.clip(ls - 257, 0, 28)]
    lx = np.where(m, np.asarray(LEN_EXTRA + [0], np.int64)[np.clip(ls - 257, 0, 28)], 0)
    lv = np.where(m, L - lb, 0)
    ds = np.where(m, np.searchsorted(np.asarray(DIST_BASE), D, side="right") - 1, -1)
    dx = np.where(m, np.asarray(DIST_EXTRA)[np.clip(ds, 0, 29)], 0)
    dv = np.where(m, D - np.asarray(DIST_BASE)[np.clip(ds, 0, 29)], 0)
    assert not m.any() or (L[m].min() >= 3 and L[m].max() <= 258 and D[m].max() <= 32768)
    return ls, lv, lx, ds, dv, dx


def canonical_codes(lengths):
    """RFC 1951 3.2.2: code of every symbol (MSB-first value) for the given lengths"""
    lengths = np.asarray(lengths, np.int64)
    bl_count = np.bincount(lengths, minlength=16)
    bl_count[0] = 0
    code, next_code = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl_count[b - 1]) << 1
        next_code[b] = code
    codes = np.zeros(len(lengths), np.int64)
    for s, l in enumerate(lengths.tolist()):
        if l:
            codes[s] = next_code[l]
            next_code[l] += 1
    return codes


def _rev(v, n):
    r = 0
    for _ in range(n):
        r, v = (r << 1) | (v & 1), v >> 1
    return r


def reversed_codes(lengths):
    """codes as they go on the wire: a Huffman code is sent MSB first, the bit writer is LSB first"""
    c = canonical_codes(lengths)
    return np.array([_rev(int(v), int(l)) for v, l in zip(c, lengths)], np.int64)


def kraft(lengths):
    from fractions import Fraction
    return sum(Fraction(1, 1 << int(l)) for l in lengths if l)


def limited_lengths(freqs, limit, min_symbols=2):
    """Huffman code lengths of `freqs`, at most `limit` bits: halve the frequencies until the tree is shallow enough.
    At least `min_symbols` symbols get a code (a complete code needs two); the result is always a complete code."""
    f = np.asarray(freqs, np.int64).copy()
    nz = np.flatnonzero(f)
    for s in range(len(f)):
        if len(nz) >= min_symbols:
            break
        if f[s] == 0:
            f[s] = 1
            nz = np.flatnonzero(f)
    while True:
        heap = [(int(f[s]), i, [s]) for i, s in enumerate(nz)]
        heapq.heapify(heap)
        depth = np.zeros(len(f), np.int64)
        k = len(heap)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], k, a[2] + b[2]))
            k += 1
        if depth.max() <= limit:
            assert kraft(depth) == 1
            return depth
        f[nz] = np.maximum((f[nz] + 1) // 2, 1)


class BitWriter:
    """LSB-first bit packer.  Fields are collected as (value, nbits) arrays and packed once."""

    def __init__(self):
        self.vals, self.nbits = [], []
        self.nbit = 0

    def put(self, v, n):
        v, n = np.atleast_1d(np.asarray(v, np.int64)), np.atleast_1d(np.asarray(n, np.int64))
        n = np.broadcast_to(n, v.shape)
        assert (n >= 0).all() and (n <= 32).all() and ((v >> n) == 0).all(), "field does not fit"
        self.vals.append(v)
        self.nbits.append(n.copy())
        self.nbit += int(n.sum())

    def align(self, pad=0):
        """to the next byte boundary; the pad bits carry `pad` (RFC 1951 says they are ignored)"""
        k = -self.nbit % 8
        if k:
            self.put(pad & ((1 << k) - 1), k)

    def getvalue(self):
        if not self.vals:
            return b""
        v, n = np.concatenate(self.vals), np.concatenate(self.nbits)
        keep = n > 0
        v, n = v[keep], n[keep]
        idx = np.arange(32)
        bits = ((v[:, None] >> idx) & 1).astype(np.uint8)
        bits = bits[idx[None, :] < n[:, None]]
        return np.packbits(bits, bitorder="little").tobytes()


class DeflateWriter:
    """One raw-DEFLATE stream, block by block.  getvalue() pads the last byte with zero bits."""

    def __init__(self):
        self.bw = BitWriter()

    @property
    def nbit(self):
        return self.bw.nbit

    def stored(self, data, final=False, pad=0):
        data = bytes(data)
        assert len(data) <= 65535
        self.bw.put(1 if final else 0, 1)
        self.bw.put(0, 2)
        self.bw.align(pad)
        n = len(data)
        self.bw.put(n, 16)
        self.bw.put(n ^ 0xffff, 16)
        if n:
            self.bw.put(np.frombuffer(data, np.uint8).astype(np.int64), 8)

    def _body(self, tokens, ll, dl):
        ls, lv, lx, ds, dv, dx = symbols(tokens)
        lc, dc = reversed_codes(ll), reversed_codes(dl)
        assert (ll[ls] > 0).all(), "a literal/length symbol without a code"
        m = ds >= 0
        assert (dl[ds[m]] > 0).all(), "a distance symbol without a code"
        n = len(ls)
        v = np.zeros((n, 4), np.int64)
        b = np.zeros((n, 4), np.int64)
        v[:, 0], b[:, 0] = lc[ls], ll[ls]
        v[:, 1], b[:, 1] = lv, lx
        v[m, 2], b[m, 2] = dc[ds[m]], dl[ds[m]]
        v[:, 3], b[:, 3] = dv, dx
        self.bw.put(v.reshape(-1), b.reshape(-1))
        self.bw.put(int(lc[END_BLOCK]), int(ll[END_BLOCK]))

    def static(self, tokens, final=False):
        self.bw.put(1 if final else 0, 1)
        self.bw.put(1, 2)
        ll, dl = static_lengths()
        self._body(tokens, ll, dl)

    def dynamic(self, tokens, litlen_lengths=None, dist_lengths=None, final=False, clen_style="rle", hclen="trim",
                hlit=None, hdist=None, limit=15):
        """A dynamic block.  Code lengths are given, or derived from the tokens' frequencies (at most `limit` bits).
        clen_style "rle" writes the code-length sequence with the 16/17/18 repeat codes, "plain" without them.  hclen "trim"
        drops trailing zero code-length-code lengths (down to 4), "full" sends all 19.  hlit / hdist force the number of codes
        sent (the lengths behind the used ones are zero)."""
        ls, _, _, ds, _, _ = symbols(tokens)
        if litlen_lengths is None:
            f = np.bincount(ls, minlength=286)[:286]
            f[END_BLOCK] += 1
            litlen_lengths = limited_lengths(f, limit)
        if dist_lengths is None:
            f = np.bincount(ds[ds >= 0], minlength=30)[:30] if (ds >= 0).any() else np.zeros(30, np.int64)
            dist_lengths = limited_lengths(f, limit) if (ds >= 0).any() else np.zeros(30, np.int64)
        ll = np.zeros(286, np.int64)
        ll[:len(litlen_lengths)] = litlen_lengths
        dl = np.zeros(30, np.int64)
        dl[:len(dist_lengths)] = dist_lengths
        nl = hlit if hlit is not None else max(257, int(np.flatnonzero(ll).max()) + 1)
        nd = hdist if hdist is not None else max(1, int(np.flatnonzero(dl).max()) + 1 if dl.any() else 1)
        assert 257 <= nl <= 286 and 1 <= nd <= 30 and not ll[nl:].any() and not dl[nd:].any()
        seq = np.concatenate([ll[:nl], dl[:nd]]).tolist()
        # the code-length sequence: (symbol, extra value, extra bits)
        cl = []
        i = 0
        while i < len(seq):
            v = seq[i]
            r = 1
            while i + r < len(seq) and seq[i + r] == v:
                r += 1
            if clen_style == "rle" and v == 0 and r >= 3:
                k = min(r, 138)
                cl.append((17, k - 3, 3) if k <= 10 else (18, k - 11, 7))
                i += k
            elif clen_style == "rle" and v != 0 and r >= 4:
                cl.append((v, 0, 0))
                k = min(r - 1, 6)
                cl.append((16, k - 3, 2))
                i += 1 + k
            else:
                cl.append((v, 0, 0))
                i += 1
        f = np.bincount([c[0] for c in cl], minlength=19)
        bl = limited_lengths(f, 7)
        order = [int(bl[s]) for s in CLEN_ORDER]
        nc = 19
        if hclen == "trim":
            while nc > 4 and order[nc - 1] == 0:
                nc -= 1
        self.bw.put(1 if final else 0, 1)
        self.bw.put(2, 2)
        self.bw.put(nl - 257, 5)
        self.bw.put(nd - 1, 5)
        self.bw.put(nc - 4, 4)
        self.bw.put(np.asarray(order[:nc], np.int64), 3)
        blc = reversed_codes(bl)
        for s, xv, xb in cl:
            self.bw.put(int(blc[s]), int(bl[s]))
            if xb:
                self.bw.put(xv, xb)
        self._body(tokens, ll, dl)
        return ll, dl

    def raw_bits(self, v, n):
        self.bw.put(v, n)

    def getvalue(self):
        return self.bw.getvalue()


def inflate_raw(z):
    """zlib's raw inflate (the reference's decoder, zip.c: inflate(Z_FINISH)) -> bytes, or None if zlib refuses the stream"""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(bytes(z)) + d.flush()
    except zlib.error:
        return None
