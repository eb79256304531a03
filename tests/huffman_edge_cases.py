"""Inputs shared by test_gpu_huffman_edges.py and its emulator twin test_sim_huffman_edges.py: blocks whose symbol counts put
the Huffman builder (mrcz_huffman.hip) on its edges -- the number of used literal/length symbols, every class of run in the
code-length sequence that scan_tree / send_tree distinguish, the size and depth of the bit-length tree, every HLIT, and
literal/length chains deeper than 15.

A case is one chunk at mask level 0: byte lane LANE holds the plane under test (one or two blocks), the other lanes noise of the
same length, which is stored RAW.  Code lengths are steered with dyadic counts (a symbol counted 2^(Lmax - l) times gets length
l exactly when the counts, END_BLOCK's 1 included, sum to 2^Lmax), which lengths are zero by the byte values used, and no byte
equals its successor unless a match is wanted.

What a case reaches is never taken from the codec: block_facts() reads it from the oracle's stream (stream_info, walk_blocks)
and from huffman_ref.py, the plain statement of trees.c, which the same function pins against the oracle on the way (the
block's opt_len and static_len, its code lengths and the bits of its dynamic header).  Every family has a *_conditions(oracle)
that asserts its cases sit where they are meant to, block type included; reached() is the union over the catalogue that
REQUIRED is compared with.

Not reachable, and so not in REQUIRED: HCLEN below 18 (the distance tree's two lengths are bit-length symbol 1, next to last
in the order the lengths are sent), and for the same reason zlib's force-two-codes rule in the bit-length tree (symbol 1
always has a count and so has whatever the literal/length tree's lengths are coded with).  A literal/length tree of one symbol
does not exist either: a block holds a symbol besides END_BLOCK.  The rule does fire in the distance tree of every block."""
import functools
import heapq

import numpy as np

import decision_edge_cases as edges
import emit_mixed_cases as mixed
import huffman_ref as ref

LANE = 1
BLK_SYMS = edges.BLK_SYMS


def words_of(plane: np.ndarray, seed: int = 5) -> np.ndarray:
    n = len(plane)
    return edges.words_of({j: plane if j == LANE else edges.noise(seed + j, n) for j in range(4)}, n)


# ------------------------------------------------------------------ planes from symbol counts
def length_code(m: int) -> int:
    return 257 + max(k for k, b in enumerate(ref.BASE_LENGTH) if b <= m)


def build_plane(lit: dict, codes: dict = None) -> np.ndarray:
    """A plane with lit[b] literals of byte b and codes[c] matches of length code c (each of the code's base length).  A match
    is a run of 1 + length equal bytes whose first byte is one of the literals counted in lit; no two neighbours in the plane
    hold the same byte."""
    left = dict(lit)
    items = {b: [] for b in lit}                            # byte -> lengths of its pieces, 1 = a single literal
    cap = [(-c, b) for b, c in lit.items()]
    heapq.heapify(cap)
    for c, cnt in sorted((codes or {}).items(), key=lambda kv: -kv[1]):
        for _ in range(cnt):
            k, b = heapq.heappop(cap)                       # the byte with most literals left carries the run
            assert k < 0, "more matches than literals"
            items[b].append(1 + ref.BASE_LENGTH[c - 257])
            left[b] -= 1
            heapq.heappush(cap, (k + 1, b))
    for b, c in left.items():
        items[b] = [1] * c + items[b]                       # runs are popped first
    order = spread({b: len(v) for b, v in items.items()})
    return np.repeat(np.array(order, np.uint8), [items[b].pop() for b in order])


def spread(counts: dict) -> list:
    """every key counts[key] times, no two equal neighbours: always the key with most left that is not the last one"""
    todo = [(-c, k) for k, c in counts.items() if c]
    heapq.heapify(todo)
    out = []
    while todo:
        c, k = heapq.heappop(todo)
        if out and k == out[-1]:
            assert todo, "%r would follow itself" % (k,)
            c2, k2 = heapq.heappop(todo)
            heapq.heappush(todo, (c, k))
            c, k = c2, k2
        out.append(k)
        if c + 1 < 0:
            heapq.heappush(todo, (c + 1, k))
    return out


def counts_for(lens: dict, lmax: int, fillers=()):
    """(lit, codes) that give symbol s the code length lens[s] and END_BLOCK lmax: 2^(lmax - l) each.  What the lengths leave
    of the Kraft sum goes to the `fillers`, one symbol for every bit of it."""
    lens = dict(lens)
    unit = lambda l: 1 << (lmax - l)
    rest = (1 << lmax) - 1 - sum(unit(l) for l in lens.values())
    assert rest >= 0, rest
    fillers = list(fillers)
    for bit in range(lmax - 1, -1, -1):
        if rest >> bit & 1:
            s = fillers.pop(0)
            assert s not in lens
            lens[s] = lmax - bit
    lit = {s: unit(l) for s, l in lens.items() if s < 256}
    codes = {s: unit(l) for s, l in lens.items() if s > 256}
    return lit, codes, lens


def dyadic_plane(lens: dict, lmax: int, fillers=()) -> np.ndarray:
    lit, codes, _ = counts_for(lens, lmax, fillers)
    return build_plane(lit, codes)


# ------------------------------------------------------------------ what the oracle and the statement say about a plane
def symbol_counts(plane: np.ndarray):
    """per block of the Z_RLE parse the literal/length counts, END_BLOCK's 1 included, and the matches"""
    edge = np.flatnonzero(np.append(True, plane[1:] != plane[:-1]))
    runlen = np.diff(np.append(edge, len(plane)))
    syms = []
    for b, l in zip(plane[edge].tolist(), runlen.tolist()):
        syms.append(b)
        l -= 1
        while l >= 3:
            m = min(l, 258)
            syms.append(length_code(m))
            l -= m
        syms += [b] * l
    out = []
    for a in range(0, len(syms), BLK_SYMS):
        f = np.bincount(syms[a: a + BLK_SYMS], minlength=ref.L_CODES).tolist()
        f[256] = 1
        out.append((f, sum(f[257:])))
    return out


def _bits_at(z: bytes, pos: int, n: int) -> int:
    return (int.from_bytes(z, "little") >> pos) & ((1 << n) - 1)


@functools.lru_cache(maxsize=None)
def _facts(oracle, key):
    plane = plane_of(key)
    nsym, nblocks, nmatch, blocks = edges.stream_info(oracle, plane)
    counts = symbol_counts(plane)
    assert len(counts) == nblocks and sum(sum(f) - 1 for f, _ in counts) == nsym and sum(m for _, m in counts) == nmatch, key
    z = oracle.deflate(plane)
    walked = mixed.walk_blocks(z)
    out, bit = [], 0
    for k, (b, (f, nm)) in enumerate(zip(blocks, counts)):
        opt, static, lt, dt, hdr = ref.block_costs(f, nm)
        assert (opt, static) == (b["opt_len"], b["static_len"]), (key, k, opt, static, b)        # the statement, pinned
        assert dt.lens[:2] == [1, 1] and dt.nheap == 2 and len(dt.forced) == (1 if nm else 2), (key, k, dt.lens)
        assert walked[k][0] == b["btype"], (key, k, walked[k][0], b)
        if b["btype"] == 2:
            assert walked[k][2] == lt.lens, (key, k, "code lengths")
            again = ref.dynamic_header(walked[k][2], dt.lens)
            assert _bits_at(z, bit + 3, again.nbits) == again.value, (key, k, "header bits")
            assert _bits_at(z, bit, 3) >> 1 == 2
        runs = ref.runs_of(lt.lens, lt.max_code)
        out.append({
            "btype": b["btype"], "n": lt.nheap, "lens": lt.lens, "hlit": hdr.hlit, "hclen": hdr.hclen,
            "runs": [(ref.run_class(R, L), "start" if a == 0 else "zero" if lt.lens[a - 1] == 0 else "nonzero", a, R) for a, R, L in runs],
            "groups": set().union(*[ref.group_facts(a, R) for a, R, _ in runs]),
            "bl_n": hdr.bl.nheap, "bl_forced": len(hdr.bl.forced), "bl_depth": max(hdr.bl.depth), "bl_rounds": hdr.bl.repair_rounds,
            "ll_depth": max(lt.depth), "ll_rounds": lt.repair_rounds, "ll_long": [s for s in range(ref.L_CODES) if lt.depth[s] > 15],
            "distinct": len(set(f) - {0}), "nsym": sum(f) - 1,
        })
        bit += b["bits"]
    return out


def block_facts(oracle, family: str, name: str):
    """one dict per block of the case's plane"""
    return _facts(oracle, (family, name))


def case_block(oracle, family, name):
    """the block a case is about: the last of its plane"""
    return block_facts(oracle, family, name)[-1]


# ------------------------------------------------------------------ T: the number of used literal/length symbols
T_N = (2, 3, 4, 15, 16, 17, 31, 32, 33, 143, 144, 145, 285, 286)
ALL_MATCH = 100             # matches of 258 in the all-match block
# the block type the oracle chooses (T alone may be static: a few symbols, or every symbol once, do not pay for a header)
T_STATIC = ("3-inc", "4-inc")       # and every "eq"


def t_symbols(n: int, kind: str):
    """the n - 1 symbols besides END_BLOCK, rarest first.  Length codes come first: a match costs the plane up to 259 bytes."""
    nl = min(n - 1, 256)
    bytes_ = list(range(nl)) if kind == "eq" else list(range(255, 255 - nl, -1))
    return list(range(285, 285 - (n - 1 - nl), -1)) + bytes_


def t_plane(name: str) -> np.ndarray:
    n, kind = name.split("-")
    n = int(n)
    if (n, kind) == (2, "inc"):
        # 32766 literals and the literal that heads the constant region fill a block; the next holds its matches of 258 alone
        return np.concatenate([(0x20 + (np.arange(BLK_SYMS - 1) % 3)).astype(np.uint8), np.full(1 + 258 * ALL_MATCH, 0x77, np.uint8)])
    syms = t_symbols(n, kind)
    if kind == "eq":
        f = {s: 1 for s in syms}                            # END_BLOCK's count: every comparison of the heap is a tie
    elif n <= 256:
        f = {s: 2 + i for i, s in enumerate(syms)}          # all different, END_BLOCK's 1 the least
    else:
        f = {s: 2 + i // 2 for i, s in enumerate(syms)}     # (1 + 2 + ... + 286 symbols are more than a block holds: pairs)
    return build_plane({s: c for s, c in f.items() if s < 256}, {s: c for s, c in f.items() if s > 256})


def t_names():
    return ["%d-%s" % (n, kind) for n in T_N for kind in ("eq", "inc")]


def t_conditions(oracle):
    for name in t_names():
        n, kind = name.split("-")
        blocks = block_facts(oracle, "T", name)
        b = blocks[-1]
        assert b["n"] == int(n), (name, b["n"])
        assert len(blocks) == (2 if name == "2-inc" else 1)
        if kind == "eq":
            assert b["nsym"] == int(n) - 1, (name, b["nsym"])
        elif int(n) <= 256 and name != "2-inc":
            assert b["distinct"] == int(n), (name, b["distinct"])     # no two used symbols are counted the same
        assert b["btype"] == (1 if kind == "eq" or name in T_STATIC else 2), (name, b["btype"])
    b = case_block(oracle, "T", "2-inc")
    assert b["btype"] == 2 and [s for s, l in enumerate(b["lens"]) if l] == [256, 285] and b["nsym"] == ALL_MATCH
    assert ("z", 1, "11..137") in [r[0] for r in b["runs"]] and b["runs"][0][3] == 256
    assert "crosses->=3" in b["groups"] and b["bl_n"] == 2 and b["bl_forced"] == 0
    assert all(l for l in case_block(oracle, "T", "286-inc")["lens"])


# ------------------------------------------------------------------ Z: runs of zero lengths
Z_LEAD = (138, 139, 140, 141, 148, 149)
Z_INNER_A = (1, 2, 3, 10, 11, 137)


def z_plane(name: str) -> np.ndarray:
    if name.startswith("lead-"):
        R = int(name[5:])
        if R == 255:
            return np.full(1 + 258 * 40, 0xff, np.uint8)
        return build_plane({R: 200, R + 2: 100, R + 3: 50, R + 5: 50})
    used = {"inner-a": np.cumsum([0] + [g + 1 for g in Z_INNER_A]).tolist(),      # 0 2 5 9 20 32 170
            "inner-b": [10, 149, 151],                                           # 138 zeros between two literals
            "starts-63": [62, 70, 72],
            "crosses-3": [60, 200, 203]}[name]
    return build_plane({b: 40 * (1 + i % 3) for i, b in enumerate(used)})


def z_names():
    return ["lead-%d" % R for R in Z_LEAD + (255,)] + ["inner-a", "inner-b", "starts-63", "crosses-3"]


def z_conditions(oracle):
    def zero_runs(name):
        b = case_block(oracle, "Z", name)
        assert b["btype"] == 2, (name, b["btype"])
        return [(a, R) for c, _, a, R in b["runs"] if c[0] == "z"]
    for R in Z_LEAD + (255,):
        assert zero_runs("lead-%d" % R)[0] == (0, R), R
    inner = zero_runs("inner-a")
    assert [R for a, R in inner if 0 < a < 171] == list(Z_INNER_A), inner
    assert (11, 138) in zero_runs("inner-b")
    assert (63, 7) in zero_runs("starts-63")
    a, R = zero_runs("crosses-3")[1]
    assert (a, R) == (61, 139) and ref.group_facts(a, R) == {"crosses->=3"}


# ------------------------------------------------------------------ N: runs of equal non-zero lengths
N_RUNS = tuple(range(1, 31))
N_LMAX, N_A, N_B = 10, 9, 10
N_FILLERS = tuple(range(233, 256, 2))
N_ROOM = 230


def n_layouts():
    """name -> code lengths of the bytes: for every R a zero, R lengths A, one B, R lengths A, packed into as many planes as
    it takes"""
    out, cur = {}, []
    for R in N_RUNS:
        piece = [0] + [N_A] * R + [N_B] + [N_A] * R
        if len(cur) + len(piece) > N_ROOM:
            out["runs-%d" % len(out)] = cur
            cur = []
        cur = cur + piece
    out["runs-%d" % len(out)] = cur
    return out


def n_plane(name: str) -> np.ndarray:
    if name == "all-256":          # every byte nine bits; the other half of the code space: length codes 257 ... 267 and END_BLOCK
        lens = {b: 9 for b in range(256)}
        lens.update({257 + k: 2 + k for k in range(11)})
        return dyadic_plane(lens, 12)
    if name == "ends-285":
        return dyadic_plane({10: 2, 20: 2, 30: 3, 40: 4, 283: 6, 284: 6, 285: 6}, 8, fillers=(50, 52, 54))
    lens = {b: l for b, l in enumerate(n_layouts()[name]) if l}
    return dyadic_plane(lens, N_LMAX, fillers=N_FILLERS)


def n_names():
    return list(n_layouts()) + ["all-256", "ends-285"]


def n_conditions(oracle):
    seen = set()
    for name, layout in n_layouts().items():
        b = case_block(oracle, "N", name)
        assert b["btype"] == 2 and b["lens"][:len(layout)] == layout, (name, b["btype"])
        seen |= {(R, behind) for c, behind, a, R in b["runs"] if c[0] == "n" and a < len(layout)}
    assert seen >= {(R, behind) for R in N_RUNS for behind in ("zero", "nonzero")}, seen
    b = case_block(oracle, "N", "all-256")
    assert b["btype"] == 2 and b["runs"][0][2:] == (0, 256) and b["runs"][0][0][0] == "n" and "crosses->=3" in b["groups"]
    assert ref.group_facts(0, 256) == {"starts-0", "crosses->=3"}
    b = case_block(oracle, "N", "ends-285")
    assert b["btype"] == 2 and b["runs"][-1][2:] == (283, 3) and b["hlit"] == 286


# ------------------------------------------------------------------ B: the bit-length tree
def b_plane(name: str) -> np.ndarray:
    if name in ("19-symbols", "18-symbols"):
        # a zero; five times 3 (a literal and a REP16); three zeros (REPZ17) or two (literals); 2; 4 ... 15; zeros (REPZ18)
        lens = {b: 3 for b in range(1, 6)}
        first = 9 if name == "19-symbols" else 8
        lens[first] = 2
        lens.update({first + 1 + k: 4 + k for k in range(12)})
        return dyadic_plane(lens, 15)
    per_length, lmax, _, _ = B_DEPTH[name]
    assert sum(c << (lmax - l) for l, c in per_length.items()) == 1 << lmax
    per_length = {l: c - (l == lmax) for l, c in per_length.items()}       # END_BLOCK is one of the longest
    return dyadic_plane(dict(enumerate(spread(per_length))), lmax)


# name -> (how many symbols have each code length, Lmax, the bit-length tree's depth before any repair, passes of the repair's
# do ... while).  The bit-length symbols' counts are then 1 (REPZ18, the zeros behind the last byte), 2 (symbol 1, the distance
# tree), 3, 5, 8, 13, ...: a chain.  Found by a search with huffman_ref.py alone: every assignment of distinct lengths 2 ... 15
# to the counts 3, 5, 8, 13, 21, 34 (, 55 (, 89 | 90)) whose Kraft sum is exactly 1, the lengths spread over the bytes with no
# two equal neighbours (so that no REP16 takes counts away), the depth from dynamic_header(); of those that reach the depth,
# the one with the smallest Lmax.  89 has no such assignment below Lmax 12; 90 has one at 11.  b_conditions() has the oracle
# confirm each: its header, re-encoded by the statement, bit for bit.
B_DEPTH = {
    "depth-7": ({10: 34, 5: 21, 8: 13, 7: 8, 9: 5, 4: 3}, 10, 7, 0),
    "depth-8": ({8: 55, 9: 34, 7: 21, 6: 13, 10: 8, 5: 5, 4: 3}, 10, 8, 1),
    "depth-9": ({9: 90, 10: 55, 11: 34, 8: 21, 6: 13, 7: 8, 4: 5, 5: 3}, 11, 9, 2),
}


def b_names():
    return ["19-symbols", "18-symbols"] + list(B_DEPTH)


def b_conditions(oracle):
    assert case_block(oracle, "T", "2-inc")["bl_n"] == 2             # REPZ18 and 1: the all-match block
    b = case_block(oracle, "Z", "lead-255")
    assert (b["bl_n"], b["btype"]) == (3, 2), b                      # REPZ18, 2 and 1
    for name, n in (("19-symbols", 19), ("18-symbols", 18)):
        b = case_block(oracle, "B", name)
        assert (b["bl_n"], b["btype"], b["hclen"]) == (n, 2, 19), (name, b["bl_n"], b["btype"])
    for name, (_, _, depth, rounds) in B_DEPTH.items():
        b = case_block(oracle, "B", name)
        assert b["btype"] == 2 and b["bl_depth"] == depth and b["bl_rounds"] == rounds, (name, b["bl_depth"], b["bl_rounds"])
    for family, name in all_cases():
        for b in block_facts(oracle, family, name):
            assert b["bl_forced"] == 0 and b["hclen"] >= 18



# ------------------------------------------------------------------ L: every HLIT
def l_plane(name: str) -> np.ndarray:
    return build_plane({0: 64, 1: 63}, None if name == "none" else {257 + int(name): 1})


def l_names():
    return ["none"] + [str(k) for k in range(29)]


# The emulator's share: a case is a second there, whatever its size.  Of every family the cases on either side of each
# branch, and all of those that the hand mutations listed in test_sim_huffman_edges.py need to fail.
SIM_CASES = {
    "T": ("2-eq", "2-inc", "4-inc", "15-inc", "16-inc", "17-inc", "32-eq", "143-inc", "144-inc", "145-inc", "285-inc", "286-eq", "286-inc"),
    "Z": ("lead-138", "lead-141", "lead-149", "lead-255", "inner-a", "inner-b", "starts-63", "crosses-3"),
    "N": ("runs-0", "runs-1", "runs-2", "runs-3", "runs-4", "all-256", "ends-285"),
    "B": ("19-symbols", "18-symbols", "depth-7", "depth-8", "depth-9"),
    "L": ("none", "0", "27", "28"),
    "F": ("16-lit", "16-len", "18-lit", "18-len"),
}


def l_conditions(oracle):
    for name in l_names():
        b = case_block(oracle, "L", name)
        assert b["btype"] == 2 and b["hlit"] == (257 if name == "none" else 258 + int(name)), (name, b["btype"], b["hlit"])
        assert b["nsym"] <= 128


# ------------------------------------------------------------------ F: literal/length chains deeper than 15
F_RARE_CODES = (281, 282, 283)


def f_plane(name: str) -> np.ndarray:
    """counts c[k] = c[k-1] + c[k-2] + 1 behind END_BLOCK's 1: the tree is one chain, len(c) - 1 deep.  "lit": every symbol
    a byte; "len": the rarest are length codes with five extra bits"""
    depth, where = name.split("-")
    c = [1, 1]
    while len(c) < int(depth) + 1:
        c.append(c[-1] + c[-2] + 1)
    c = c[1:]
    if where == "lit":
        return build_plane({40 + 3 * k: f for k, f in enumerate(c)})
    nrare = len(F_RARE_CODES) if int(depth) > 16 else 1
    return build_plane({40 + 3 * k: f for k, f in enumerate(c[nrare:])}, dict(zip(F_RARE_CODES, c[:nrare])))


def f_names():
    return ["16-lit", "16-len", "18-lit", "18-len"]


def f_conditions(oracle):
    for name in f_names():
        depth, where = name.split("-")
        b = case_block(oracle, "F", name)
        assert b["btype"] == 2 and b["ll_depth"] == int(depth) and max(b["lens"]) == 15, (name, b["ll_depth"], b["btype"])
        long = [s for s in b["ll_long"] if s != 256]
        assert len(b["ll_long"]) == (2 if depth == "16" else 4), (name, b["ll_long"])
        assert all(s < 256 for s in long) if where == "lit" else all(s > 256 for s in long), (name, long)
    assert case_block(oracle, "F", "16-lit")["ll_rounds"] == 1 and case_block(oracle, "F", "18-lit")["ll_rounds"] >= 2


# ------------------------------------------------------------------ the catalogue
FAMILIES = {"T": (t_names, t_plane), "Z": (z_names, z_plane), "N": (n_names, n_plane), "B": (b_names, b_plane),
            "L": (l_names, l_plane), "F": (f_names, f_plane)}


def all_cases():
    return [(family, name) for family, (names, _) in FAMILIES.items() for name in names()]


@functools.lru_cache(maxsize=None)
def plane_of(key) -> np.ndarray:
    p = FAMILIES[key[0]][1](key[1])
    assert len(p) <= 72000, (key, len(p))
    p.setflags(write=False)
    return p


def case_words(family: str, name: str) -> np.ndarray:
    return words_of(plane_of((family, name)))


def conditions(oracle, family: str):
    {"T": t_conditions, "Z": z_conditions, "N": n_conditions, "B": b_conditions, "L": l_conditions, "F": f_conditions}[family](oracle)


# ------------------------------------------------------------------ the classes the catalogue has to reach
ZERO_RESTS = ("0", "1", "2", "3..10", "11..137")
REQUIRED = (
    {("tree-size", n) for n in T_N}
    | {("zero-run", 1, rest) for rest in ZERO_RESTS}              # 138 | 139 | 140 | 141, 148 | 149, 255, 256
    | {("zero-run", 0, rest) for rest in ZERO_RESTS[1:]}          # 1 | 2 | 3, 10 | 11, 137
    | {("zero-run-length", R) for R in Z_LEAD + (255, 256) + Z_INNER_A + (138,)}
    | {("run",) + ref.run_class(R, 8)[1:] + (behind,) for R in range(1, 31) for behind in ("zero", "nonzero")}
    | {("run-length", R) for R in N_RUNS + (256,)}
    | {("zero-run-group", "starts-63"), ("zero-run-group", "crosses->=3"), ("run-group", "crosses->=3"), ("run-ends", 285)}
    | {("group", g) for g in ("starts-63", "starts-0", "crosses-1", "crosses-2", "crosses->=3")}
    | {("bl-size", n) for n in (2, 3, 18, 19)}
    | {("bl-depth", 7, 0), ("bl-depth", 8, 1), ("bl-depth", 9, 2)}      # (depth, passes of the repair loop: 2 = two or more)
    | {("hlit", h) for h in range(257, 287)}
    | {("ll-repair", "one-level", "lit"), ("ll-repair", "one-level", "len"), ("ll-repair", ">=3-levels", "lit"),
       ("ll-repair", ">=3-levels", "len")}
)


def reached(oracle):
    """the classes the oracle's streams of the whole catalogue show: run classes and header facts from dynamic blocks alone"""
    got = set()
    for family, name in all_cases():
        for b in block_facts(oracle, family, name):
            got.add(("tree-size", b["n"]))
            if b["btype"] != 2:
                continue
            got.add(("hlit", b["hlit"]))
            got.add(("bl-size", b["bl_n"]))
            got.add(("bl-depth", min(b["bl_depth"], 9), min(b["bl_rounds"], 2)))
            got |= {("group", g) for g in b["groups"]}
            for c, behind, a, R in b["runs"]:
                facts = ref.group_facts(a, R)
                if c[0] == "z":
                    got.add(("zero-run",) + c[1:])
                    got.add(("zero-run-length", R))
                    got |= {("zero-run-group", g) for g in facts}
                else:
                    got.add(("run",) + c[1:] + (behind,))
                    got.add(("run-length", R))
                    got |= {("run-group", g) for g in facts}
                    if a + R == 286:
                        got.add(("run-ends", 285))
            if b["ll_depth"] > 15:
                long = [s for s in b["ll_long"] if s != 256]
                got.add(("ll-repair", "one-level" if b["ll_depth"] == 16 else ">=3-levels" if b["ll_depth"] >= 18 else "two-levels",
                         "lit" if all(s < 256 for s in long) else "len" if all(s > 256 for s in long) else "both"))
    return got


# ------------------------------------------------------------------ the check of one case, and what to say when bytes differ
class _Recording(edges.Backend):
    """passes every call on and keeps the container the codec wrote"""

    def __init__(self, be):
        self.be, self.container = be, None

    def compress_prefilled(self, words):
        got, olen, sums = self.be.compress_prefilled(words)
        self.container = bytes(got[:olen])
        return got, olen, sums

    def blocks(self, stream):
        return self.be.blocks(stream)

    def probe(self, words):
        return self.be.probe(words)

    def decode(self, records, nwords):
        return self.be.decode(records, nwords)


def header_fields(z: bytes, pos: int):
    """the fields of the dynamic header whose block starts at bit pos: name -> value, in the order they are sent"""
    v = int.from_bytes(z, "little") >> (pos + 3)
    out, at = {}, 0

    def bits(n):
        nonlocal at
        x = (v >> at) & ((1 << n) - 1)
        at += n
        return x

    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    out.update(HLIT=hlit, HDIST=hdist, HCLEN=hclen)
    cl = [0] * 19
    for i in range(hclen):
        cl[ref.BL_ORDER[i]] = bits(3)
        out["length of bit-length symbol %d" % ref.BL_ORDER[i]] = cl[ref.BL_ORDER[i]]
    tab, maxlen = mixed._table(cl)
    have, i = 0, 0
    while have < hlit + hdist and i < 400:
        s, l = tab[(v >> at) & ((1 << maxlen) - 1)] or (None, 1)
        at += l
        x = bits(ref.EXTRA_BLBITS[s]) if s is not None else 0
        out["bit-length symbol #%d" % i] = (s, x)
        if s is None:
            break
        have += 1 if s < 16 else 3 + x if s < 18 else 11 + x
        i += 1
    return out


def explain(oracle, family: str, name: str, container: bytes):
    """the first block of the case's plane in which the codec's stream differs from the oracle's, and the first field of it
    that does; None if the streams agree (or the codec wrote none)"""
    plane = plane_of((family, name))
    want = oracle.deflate(plane)
    try:
        have = mixed.plane_stream(b"\0" * 17 + container, LANE)
    except AssertionError:
        return None if len(want) + 4 >= len(plane) else "the codec stored the plane RAW"
    if have == want:
        return None
    blocks = edges.stream_info(oracle, plane)[3]
    bit = 0
    for k, b in enumerate(blocks):
        if _bits_at(have, bit, b["bits"]) != _bits_at(want, bit, b["bits"]):
            break
        bit += b["bits"]
    where = "block %d (type %d, symbols of bytes %d ... %d)" % (k, b["btype"], b["start"], b["end"])
    t = _bits_at(have, bit, 3) >> 1
    if t != b["btype"]:
        return "%s: block type %d" % (where, t)
    if t != 2:
        return "%s: the bits of a block without a header differ" % where
    hf, wf = header_fields(have, bit), header_fields(want, bit)
    for field in wf:
        if hf.get(field) != wf[field]:
            return "%s: %s is %r, the oracle's %r" % (where, field, hf.get(field), wf[field])
    try:
        hl, wl = mixed.walk_blocks(have)[k][2], mixed.walk_blocks(want)[k][2]
    except Exception as e:                                                  # noqa: BLE001 (whatever a broken stream raises)
        return "%s: the header agrees, the codec's stream does not parse behind it (%s)" % (where, type(e).__name__)
    for s in range(ref.L_CODES):
        if hl[s] != wl[s]:
            return "%s: code length of symbol %d is %d, the oracle's %d" % (where, s, hl[s], wl[s])
    return "%s: header and code lengths agree, the symbols' bits differ" % where


def check(be, oracle, family: str, name: str, max_batch_chunks: int = 2):
    """decision_edge_cases.check_case for one case: the container in a pre-filled buffer, the block table of every stream,
    the probe's sizes and the decode of the oracle's container.  Where the container differs in the plane under test, the
    failure names the block and the field, not bytes."""
    rec = _Recording(be)
    try:
        return edges.check_case(rec, oracle, case_words(family, name), "%s-%s" % (family, name), max_batch_chunks)
    except AssertionError as e:
        why = rec.container is not None and explain(oracle, family, name, rec.container)
        if why:
            raise AssertionError("%s-%s: %s" % (family, name, why)) from e
        raise
