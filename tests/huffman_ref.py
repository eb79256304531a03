"""A plain statement of the part of zlib's trees.c that turns a block's symbol counts into its dynamic header: build_tree
(pqdownheap, smaller() on (freq, depth), the force-two-codes rule), gen_bitlen with its repair of over-long codes, gen_codes,
scan_tree / send_tree as the symbol-by-symbol state machine (max_count, min_count, prevlen) and send_all_trees.  Pure Python,
written from trees.c and RFC 1951 and from nothing in csrc/: it is what huffman_edge_cases.py measures every input with, and
test_sim_huffman_edges.py pins it by re-encoding every dynamic header the oracle writes for the catalogue.

Also here: the names of the classes a run of equal code lengths falls into (run_class, group_facts), which is how the catalogue
says what an input reaches."""

L_CODES, D_CODES, BL_CODES = 286, 30, 19
END_BLOCK, REP_3_6, REPZ_3_10, REPZ_11_138 = 256, 16, 17, 18
BL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EXTRA_LBITS = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
EXTRA_BLBITS = (0,) * 16 + (2, 3, 7)
BASE_LENGTH = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
STATIC_LLEN = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8


class Tree:
    """what build_tree leaves: lens (after gen_bitlen), codes (bit-reversed, as sent), depth (the leaves' depth in the Huffman
    tree before any length is cut), nheap (heap entries before the first merge, forced ones included), forced (symbols the
    force-two-codes rule added), max_code, overflow (gen_bitlen's counter: 0 = no repair), repair_rounds (passes of its
    do ... while), order (the nodes as zlib removes them)"""


def build_tree(freq, elems: int, max_length: int) -> Tree:
    freq = list(freq) + [0] * (elems + 1)
    depth = [0] * (2 * elems + 1)
    dad = [0] * (2 * elems + 1)
    heap = [0]                                            # 1-based, as in zlib
    max_code = -1
    for n in range(elems):
        if freq[n]:
            heap.append(n)
            max_code = n
    t = Tree()
    t.forced = []
    while len(heap) - 1 < 2:
        if max_code < 2:
            max_code += 1
            node = max_code
        else:
            node = 0
        heap.append(node)
        freq[node] = 1
        t.forced.append(node)
    t.nheap = len(heap) - 1
    t.max_code = max_code

    def smaller(n, m):
        return freq[n] < freq[m] or (freq[n] == freq[m] and depth[n] <= depth[m])

    def pqdownheap(k):
        heap_len = len(heap) - 1
        v = heap[k]
        j = k << 1
        while j <= heap_len:
            if j < heap_len and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k = j
            j <<= 1
        heap[k] = v

    for n in range((len(heap) - 1) // 2, 0, -1):
        pqdownheap(n)
    order = []                                            # zlib's heap[heap_max ...] read from the top of the array downwards
    node = elems
    while True:
        n = heap[1]
        heap[1] = heap[-1]
        heap.pop()
        pqdownheap(1)
        m = heap[1]
        order += [n, m]
        freq[node] = freq[n] + freq[m]
        depth[node] = max(depth[n], depth[m]) + 1
        dad[n] = dad[m] = node
        heap[1] = node
        node += 1
        pqdownheap(1)
        if len(heap) - 1 < 2:
            break
    root = heap[1]
    t.order = order + [root]

    # gen_bitlen
    lens = [0] * (2 * elems + 1)
    true_depth = [0] * (2 * elems + 1)
    bl_count = [0] * (max_length + 2)
    overflow = 0
    for n in reversed(order):
        true_depth[n] = true_depth[dad[n]] + 1
        bits = lens[dad[n]] + 1
        if bits > max_length:
            bits = max_length
            overflow += 1
        lens[n] = bits
        if n > max_code:
            continue
        bl_count[bits] += 1
    t.overflow = overflow
    t.repair_rounds = 0
    if overflow:
        while True:
            bits = max_length - 1
            while bl_count[bits] == 0:
                bits -= 1
            bl_count[bits] -= 1
            bl_count[bits + 1] += 2
            bl_count[max_length] -= 1
            overflow -= 2
            t.repair_rounds += 1
            if overflow <= 0:
                break
        h = 0
        for bits in range(max_length, 0, -1):
            n = bl_count[bits]
            while n:
                m = order[h]
                h += 1
                if m > max_code:
                    continue
                lens[m] = bits
                n -= 1
    t.lens = [lens[n] if n <= max_code and freq[n] else 0 for n in range(elems)]
    t.depth = [true_depth[n] if t.lens[n] else 0 for n in range(elems)]
    t.freq = freq[:elems]

    # gen_codes
    next_code, code = [0] * (max_length + 2), 0
    for bits in range(1, max_length + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    t.codes = [0] * elems
    for n in range(max_code + 1):
        l = t.lens[n]
        if l:
            t.codes[n] = int(format(next_code[l], "0%db" % l)[::-1], 2)
            next_code[l] += 1
    return t


def scan_tree(lens, max_code: int):
    """zlib's scan_tree and send_tree, which are one loop: the bit-length symbols of lens[0 ... max_code] as a list of
    (symbol, value of its extra bits), and the 19 counts"""
    lens = list(lens[: max_code + 1]) + [0xffff]          # the guard
    out = []
    prevlen, nextlen, count = -1, lens[0], 0
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for n in range(max_code + 1):
        curlen, nextlen = nextlen, lens[n + 1]
        count += 1
        if count < max_count and curlen == nextlen:
            continue
        elif count < min_count:
            out += [(curlen, 0)] * count
        elif curlen != 0:
            if curlen != prevlen:
                out.append((curlen, 0))
                count -= 1
            out.append((REP_3_6, count - 3))
        elif count <= 10:
            out.append((REPZ_3_10, count - 3))
        else:
            out.append((REPZ_11_138, count - 11))
        count, prevlen = 0, curlen
        if nextlen == 0:
            max_count, min_count = 138, 3
        elif curlen == nextlen:
            max_count, min_count = 6, 3
        else:
            max_count, min_count = 7, 4
    counts = [0] * BL_CODES
    for s, _ in out:
        counts[s] += 1
    return out, counts


class Header:
    """what send_all_trees writes behind the three bits of the block header: value / nbits (LSB first), and hlit, hdist,
    hclen as counts, the bit-length tree (bl) and the symbol sequences (lsyms, dsyms)"""


def dynamic_header(ll_lens, d_lens) -> Header:
    h = Header()
    lmax = max(n for n in range(L_CODES) if ll_lens[n])
    dmax = max([n for n in range(len(d_lens)) if d_lens[n]] + [0])
    h.hlit, h.hdist = lmax + 1, dmax + 1
    h.lsyms, lc = scan_tree(ll_lens, lmax)
    h.dsyms, dc = scan_tree(d_lens, dmax)
    h.bl_freq = [a + b for a, b in zip(lc, dc)]
    h.bl = build_tree(h.bl_freq, BL_CODES, 7)
    max_blindex = BL_CODES - 1
    while max_blindex >= 3 and h.bl.lens[BL_ORDER[max_blindex]] == 0:
        max_blindex -= 1
    h.hclen = max_blindex + 1
    value, nbits = 0, 0

    def put(v, n):
        nonlocal value, nbits
        value |= v << nbits
        nbits += n

    put(h.hlit - 257, 5)
    put(h.hdist - 1, 5)
    put(h.hclen - 4, 4)
    for rank in range(h.hclen):
        put(h.bl.lens[BL_ORDER[rank]], 3)
    for s, x in h.lsyms + h.dsyms:
        put(h.bl.codes[s], h.bl.lens[s])
        put(x, EXTRA_BLBITS[s])
    h.value, h.nbits = value, nbits
    return h


def block_costs(ll_freq, nmatch: int):
    """(opt_len, static_len) of a block in bits, as zlib has them when it chooses the block type; the literal/length tree,
    the distance tree and the header on the way.  ll_freq holds END_BLOCK's 1; every match has distance 1."""
    lt = build_tree(ll_freq, L_CODES, 15)
    dt = build_tree([nmatch] + [0] * (D_CODES - 1), D_CODES, 15)
    hdr = dynamic_header(lt.lens, dt.lens)
    opt = sum(f * (lt.lens[n] + (EXTRA_LBITS[n - 257] if n > 256 else 0)) for n, f in enumerate(ll_freq))
    opt += nmatch * dt.lens[0] + hdr.nbits
    static = sum(f * (STATIC_LLEN[n] + (EXTRA_LBITS[n - 257] if n > 256 else 0)) for n, f in enumerate(ll_freq)) + 5 * nmatch
    return opt, static, lt, dt, hdr


# ------------------------------------------------------------------ the classes of a run of equal code lengths
def runs_of(lens, max_code: int):
    """maximal runs of equal lengths in lens[0 ... max_code]: (first symbol, length of the run, the code length)"""
    out, a = [], 0
    for n in range(1, max_code + 2):
        if n == max_code + 1 or lens[n] != lens[a]:
            out.append((a, n - a, lens[a]))
            a = n
    return out


def zero_rest_class(r: int) -> str:
    return str(r) if r < 3 else "3..10" if r <= 10 else "11..137"


def run_class(R: int, L: int):
    """zero run: ("z", min(R // 138, 1), class of R % 138);  non-zero run: ("n", h, full, r)"""
    if L == 0:
        return ("z", min(R // 138, 1), zero_rest_class(R % 138))
    h = min(R, 7)
    return ("n", h, min((R - h) // 6, 2), (R - h) % 6)


def group_facts(first: int, R: int):
    """what the position of a run means to a scan that takes the symbols 64 at a time"""
    facts = set()
    if first % 64 == 63:
        facts.add("starts-63")
    if first % 64 == 0:
        facts.add("starts-0")
    crossed = (first + R) // 64 - first // 64      # boundaries between the run's start and the next run's start
    if crossed:
        facts.add("crosses-%s" % (crossed if crossed < 3 else ">=3"))
    return facts
