"""Inputs shared by test_sim_erroranalysis.py, the erroranalysis CLI tests on the emulator and test_gpu_erroranalysis.py: the
selection of the worst points (k_err_hist, k_err_collect in csrc/mrcz_tools.hip; host/erroranalysis.c).

Every case is a triple (a, b, K): the words of the original file, the words of the decoded file, and -k.  What comes out is stated
by tests/erroranalysis_ref.py.  A case that goes through ref.lines keeps K x n small (the statement scans the whole array K
times in Python)."""
import functools

import numpy as np

import util

F = lambda *x: np.array(x, np.float32).view(np.uint32)
INF, FLT_MAX, FLT_MIN = 0x7F800000, 0x7F7FFFFF, 0x00800000
NEG = 0x80000000


def _masked(n: int, seed: int, bits: int = 14):
    """Gaussian words and their masked copy, no header: natural errors below 2^(bits - 20)"""
    a = util.gauss_words(n, seed=seed, header=False)
    return a, a & np.uint32((0xFFFFFFFF << bits) & 0xFFFFFFFF)


# ------------------------------------------------------------------ base: the data of test_host_sim.py's reference test
def base(k: int, nanat):
    w = util.gauss_words(50000, seed=k)
    dec = util.erase_expected(w, 14)
    f = dec.view(np.float32)
    f[1234] += 3.5
    f[40000] -= 3.5
    if nanat is not None:
        f[nanat] = np.float32(np.nan)
        f[nanat + 5000] = np.float32(np.nan)
    return w, dec[:49000].copy(), k


# ------------------------------------------------------------------ wide: one error per binade
WIDE_N = 5000 + 77
WIDE_EXP = np.round(np.linspace(-149, 127, 64)).astype(int)        # 64 binades from the smallest denormal to 2^127


def wide(K: int, lo: int = 0, hi: int = 64):
    """b = a but for the points lo..hi-1 of 64, whose errors lie in 64 different binades: the K-th key walks other buckets in
    every pass.  The original is 0 at every other planted point, so half of them have a relative error and half have none."""
    rng = np.random.default_rng(64)
    a = util.gauss_words(WIDE_N, seed=64, header=False)
    b = a.copy()
    pos = np.sort(rng.choice(WIDE_N, 64, replace=False))
    order = rng.permutation(64)
    for j in range(lo, hi):
        e = int(WIDE_EXP[j])
        frac = 1.0 + (0 if e == -149 else int(rng.integers(0, 1 << 20)) / float(1 << 20))
        d = np.float32(np.ldexp(frac, e))
        p = pos[order[j]]
        if j & 1:
            a[p] = 0
            b[p] = d.view(np.uint32)
        else:
            x = np.float32(1.5) if e > -20 else np.float32(np.ldexp(1.5, e + 3))
            a[p] = x.view(np.uint32)
            b[p] = np.float32(x + d).view(np.uint32)
    return a, b, K


# ------------------------------------------------------------------ pass 0 lands in bucket 0
def denormal_errors(K: int = 7):
    """20 errors with keys below 2^21 (denormals under 2^-128) over both lower radix fields, two of them equal; every other
    error is 0.  A flush-to-zero subtraction prints 20 zeros."""
    n = 1000
    a = np.zeros(n, np.uint32)
    a[::3] = 0x00000123                                           # denormal originals: the sum below is an integer sum
    b = a.copy()
    rng = np.random.default_rng(21)
    keys = [1, 2, 1023, 1024, 1025, (1 << 21) - 1, 1 << 20, (1 << 20) | 1, 2047, 2048, 2049, 77777, 77777]
    keys += [int(x) for x in rng.integers(1, 1 << 21, 7)]
    pos = np.sort(rng.choice(n, len(keys), replace=False))
    for p, k in zip(pos, keys):
        b[p] = a[p] + np.uint32(k)
    assert len(keys) == 20 and K < n
    return a, b, K


def zero_tail():
    """five non-zero errors and -k 8: the K-th error is exactly 0, three points of zero error come out in file order"""
    a, _ = _masked(300, 8)
    b = a.copy()
    f = b.view(np.float32)
    for p, d in ((17, 0.5), (18, 2.0), (100, 0.25), (255, 1.0), (299, 0.125)):
        f[p] += np.float32(d)
    return a, b, 8


def identical(K: int = 4):
    w = util.gauss_words(20000, seed=3)
    return w, w.copy(), K


# ------------------------------------------------------------------ keys that differ in the lowest bit of a prefix
BOUNDARY_KEYS = (0x40A00000, 0x40800000,      # bit 21: other bucket in pass 0's lowest bit
                 0x40000400, 0x40000000,      # bit 10: same pass-0 bucket, neighbours in pass 1
                 0x3F800001, 0x3F800000)      # bit 0: same buckets in passes 0 and 1, neighbours in pass 2


def key_boundaries(K: int):
    """six planted errors (the original is 0 there, so the key is the decoded word) in three pairs; -k 1 .. 6 cuts before, inside
    and after each pair.  Around them the natural errors of a masked Gaussian, all below 2^-6."""
    a, b = _masked(1000 + 3, 10)
    a, b = a.copy(), b.copy()
    for p, k in zip((900, 5, 333, 334, 1002, 0), BOUNDARY_KEYS):
        a[p] = 0
        b[p] = k
    return a, b, K


# ------------------------------------------------------------------ special values
def _special_pairs(x=0x41200000):
    return [(0x00000000, NEG),                           # +0 against -0: error 0
            (FLT_MIN, FLT_MIN + 1),                      # one ulp at FLT_MIN: a denormal error
            (F(1.0)[0], INF),                            # an infinite error
            (INF, INF),                                  # Inf - Inf: a NaN difference of two numbers
            (INF, INF | NEG),                            # infinite error, relative error Inf / Inf
            (FLT_MAX, FLT_MAX | NEG),                    # overflow to an infinite error
            (x, 0x7FC00000),                             # a NaN in the decoded file
            (0xFFC12345, x),                             # a negative NaN with a payload in the original: printf says -nan
            (F(16777216.0)[0], F(0.5)[0])]               # 16777215.5: inexact in float32


def specials(where: str, K: int):
    pairs = np.array(_special_pairs(), np.uint32)
    if where == "only":
        return pairs[:, 0].copy(), pairs[:, 1].copy(), K
    a, b = _masked(600 + 7, 12)
    a, b = a.copy(), b.copy()
    if where == "head":                                  # indices 0 .. 8: three short segments between the walls, then the rest
        idx = np.arange(9)
    elif where == "tail":                                # indices n-9 .. n-1
        idx = np.arange(len(a) - 9, len(a))
    else:                                                # "ends": the Inf / -Inf pair first, the negative NaN last, the rest adjacent
        idx = np.array([300, 301, 302, 303, 0, 304, 305, len(a) - 1, 306])
    a[idx], b[idx] = pairs[:, 0], pairs[:, 1]
    return a, b, K


# ------------------------------------------------------------------ ties
def equal_errors(K: int = 12):
    """300 points with an error of exactly 0.25 and 300 different relative errors; everything else is equal"""
    n = 1000
    rng = np.random.default_rng(300)
    a = np.full(n, F(3.0)[0], np.uint32)
    b = a.copy()
    pos = np.sort(rng.choice(n, 300, replace=False))
    v = (4.0 + 0.25 * rng.permutation(300)).astype(np.float32)   # multiples of 0.25 below 128: v + 0.25 is exact
    a[pos] = v.view(np.uint32)
    b[pos] = (v + np.float32(0.25)).view(np.uint32)
    return a, b, K


NEAR_U = 2.0 ** -33        # one ulp of a float32 in [2^-10, 2^-9): every number below is a multiple of it


def near_ties(K: int, swap: bool):
    """Errors near 0.0008, where a float32 ulp is 2^-34 and 1e-7f lies between 858 and 859 units of 2^-33.  Two pairs 858 units
    apart (the reference calls them equal and lets the larger relative error win) and two pairs 859 apart (it does not), the
    smaller error always with the smaller original, that is, the larger relative error; each in both file orders."""
    a, b = _masked(2000 + 1, 33, bits=4)                 # natural errors below 2^-16
    a, b = a.copy(), b.copy()
    A, E = 9448928, 6871947                              # 0.0011 and 0.0008 in units of 2^-33
    plant = [(A, E), (A - 1000, E - 858),                # a tie within 1e-7f
             (A, E - 20000), (A - 1000, E - 20000 - 859),            # no tie
             (A - 1000, E - 40000 - 858), (A, E - 40000),            # a tie, the smaller error first in the file
             (A - 1000, E - 60000 - 859), (A, E - 60000)]            # no tie, the smaller error first
    pos = [100, 1500, 200, 1600, 300, 1700, 400, 1800]
    if swap:
        pos = pos[::-1]
    for p, (am, em) in zip(pos, plant):
        x, y = np.float32(am * NEAR_U), np.float32((am + em) * NEAR_U)
        assert float(x) == am * NEAR_U and float(y) == (am + em) * NEAR_U and float(np.float32(y - x)) == em * NEAR_U
        a[p], b[p] = x.view(np.uint32), y.view(np.uint32)
    return a, b, K


def tie_chain(levels, ranks, K: int):
    """Errors 800 units of 2^-33 (0.93e-7) apart, level by level below the largest, so that every level is "equal" to the next
    one and to no other, with the relative errors ranked by `ranks` (the original shrinks by 1 % per rank).  A point several
    levels under the K-th error decides which of the top points comes out: found by random search against a selection that
    only keeps what lies within 4e-7 of the K-th error.  Behind the chain 100 equal errors 5e-6 lower: with a candidate buffer
    of 64 records the first, wide hand-back does not fit."""
    a, b = _masked(2000 + 1, 34, bits=4)                 # natural errors below 2^-16
    a, b = a.copy(), b.copy()
    A, E = 12000000, 4000000                             # 0.0014 and 0.00047 in units of 2^-33
    plant = [(50 + 100 * i, A - 120000 * int(r), E - 800 * l) for i, (l, r) in enumerate(zip(levels, ranks))]
    plant += [(1500 + j, A, E - 43000) for j in range(100)]
    for p, am, em in plant:
        x, y = np.float32(am * NEAR_U), np.float32((am + em) * NEAR_U)
        assert float(x) == am * NEAR_U > 10E-4 and float(y) == (am + em) * NEAR_U and float(np.float32(y - x)) == em * NEAR_U
        a[p], b[p] = x.view(np.uint32), y.view(np.uint32)
    return a, b, K


# ------------------------------------------------------------------ -k against the number of points, lengths
def k_relation(n: int, K: int, na: int = 0, nb: int = 0):
    """n points in common, the original na words longer, the decoded file nb words longer"""
    a, b = _masked(n + max(na, nb), n + K)
    return a[: n + na].copy(), b[: n + nb].copy(), K


# ------------------------------------------------------------------ NaN walls
def walls(at, K: int, n: int = 2000 + 5):
    a, b = _masked(n, 97, bits=12)
    b = b.copy()
    b[np.asarray(at)] = 0x7FC00000
    return a, b, K


def walls202():
    """the data of test_host_sim.py's candidate-buffer test: 202 walls, the first at 500"""
    w = util.gauss_words(20000, seed=3)
    d = util.erase_expected(w, 12)
    d.view(np.float32)[500:20000:97] = np.float32(np.nan)
    return w, d, 6


def walls202_early():
    """202 walls from index 3 on: -k 12 runs through four segments and three walls"""
    a, b = _masked(202 * 3 + 50, 202, bits=12)
    b = b.copy()
    b[3:202 * 3 + 3:3] = 0x7FC00000
    return a, b, 12


CASES = {
    "base_k2_nan777": lambda: base(2, 777),
    "base_k5_nan2": lambda: base(5, 2),
    "base_k6": lambda: base(6, None),
    "base_k3_nan0": lambda: base(3, 0),
    "wide_k1": lambda: wide(1),
    "wide_k12": lambda: wide(12),
    "wide_low_k12": lambda: wide(12, 0, 14),             # only the 14 smallest: the K-th error is a denormal
    "wide_mid_k9": lambda: wide(9, 0, 40),
    "denormal_errors_k7": lambda: denormal_errors(7),
    "denormal_errors_k12": lambda: denormal_errors(12),
    "zero_tail": zero_tail,
    "identical": identical,
    **{f"key_boundaries_k{k}": (lambda k=k: key_boundaries(k)) for k in range(1, 7)},
    "specials_only_k9": lambda: specials("only", 9),
    "specials_only_k12": lambda: specials("only", 12),
    "specials_head_k12": lambda: specials("head", 12),
    "specials_tail_k12": lambda: specials("tail", 12),
    "specials_ends_k5": lambda: specials("ends", 5),
    "equal_errors_k12": equal_errors,
    **{f"near_ties_k{k}{'_swapped' if s else ''}": (lambda k=k, s=s: near_ties(k, s)) for k in (1, 3, 5, 8) for s in (False, True)},
    "tie_chain_k1": lambda: tie_chain([5, 4, 1, 6, 3, 2, 2, 6, 3, 4, 5, 6, 6, 6], [5, 4, 3, 2, 12, 7, 1, 0, 9, 10, 11, 8, 13, 6], 1),
    "tie_chain_k3": lambda: tie_chain([3, 0, 5, 1, 3, 1, 4, 6, 5, 2, 4, 6], [8, 11, 9, 6, 3, 0, 4, 5, 7, 1, 2, 10], 3),
    "k_equals_n": lambda: k_relation(12, 12),
    "k_equals_n_257": lambda: k_relation(257, 257),
    "k_above_n": lambda: k_relation(5, 9),
    "k_zero": lambda: k_relation(100, 0),
    "one_point": lambda: k_relation(1, 1),
    "one_point_k3": lambda: k_relation(1, 3),
    "original_longer": lambda: k_relation(1000, 4, na=300),
    "decoded_longer": lambda: k_relation(1000, 4, nb=300),
    "n_256": lambda: k_relation(256, 5),
    "n_258": lambda: k_relation(258, 5),
    "wall_at_0": lambda: walls([0], 4),
    "wall_at_3_k8": lambda: walls([3], 8),
    "adjacent_walls": lambda: walls([2, 3], 6),
    "adjacent_walls_at_0": lambda: walls([0, 1, 5], 7),
    "wall_at_the_end": lambda: walls([2004], 3),
    "walls202": walls202,
    "walls202_early": walls202_early,
}
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name: str):
    a, b, K = CASES[name]()
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, K


@functools.lru_cache(maxsize=None)
def expected_lines(name: str) -> str:
    """ref.lines of a case, computed once and shared by every test that needs it"""
    import erroranalysis_ref as ref
    return ref.lines(*case(name))


def points(name: str):
    """the points both files have: what the kernels see"""
    a, b, K = case(name)
    n = min(len(a), len(b))
    return a[:n], b[:n], K


def segments(a, b):
    """the NaN-free ranges [lo, hi) the walls cut the array into"""
    import erroranalysis_ref as ref
    w = np.flatnonzero(ref.err_key(a, b) == ref.NAN_KEY)
    edges = np.concatenate(([-1], w, [len(a)]))
    return [(int(lo) + 1, int(hi)) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo + 1]


# ------------------------------------------------------------------ GPU only
GRID_POINTS = 3 * 2048 * 256 + 77      # k_err_hist / k_err_collect run 2048 blocks of 256: three whole grid-stride steps and 77 points


def grid_stride():
    """every thread takes more than one step and the last step is ragged; the errors of `wide` repeated through the array, and
    natural errors between them"""
    a, b = _masked(GRID_POINTS, 2048, bits=10)
    a, b = a.copy(), b.copy()
    wa, wb, _ = wide(1)
    for off in (0, 2048 * 256 - 3000, 2 * 2048 * 256 + 11, GRID_POINTS - WIDE_N):
        a[off: off + WIDE_N], b[off: off + WIDE_N] = wa, wb
    return a, b, 100


BATCH = 64 << 20                       # floats per device batch of the tool (host/erroranalysis.c)
BIG_N = BATCH + 70001


def two_batches():
    """The shipped batch size: 64 Mi + 70 001 points, so the second batch is short.  a = Gaussian words, b = a masked by 8 bits
    (errors below 2^-11), a NaN wall at 3, three planted errors before it, eight more (1.0, 1.25, .. 2.75) on both sides of the
    batch boundary, at the ends and inside.  The expectation is known by construction: returns (a, b, {k: [(n1, n2) words of
    the lines, in order]})."""
    rng = np.random.default_rng(26)
    a = np.empty(BIG_N, np.uint32)
    step = 1 << 22
    for o in range(0, BIG_N, step):
        m = min(step, BIG_N - o)
        a[o: o + m] = rng.normal(10.0, 3.0, m).astype(np.float32).view(np.uint32)
    b = a & np.uint32(0xFFFFFF00)
    f1, f2 = a.view(np.float32), b.view(np.float32)

    def plant(p, d):                    # original 8.0, so that 8 + d and the difference are exact
        f1[p] = np.float32(8.0)
        f2[p] = np.float32(8.0 + d)

    plant(0, 0.5)
    plant(1, 0.75)
    plant(2, 0.625)
    b[3] = 0x7FC00000
    tail = [4, BATCH - 1, BATCH, BATCH + 1, (1 << 26) + 4096, BIG_N - 1, 12345678, BATCH + 33333]
    errs = [1.0 + 0.25 * j for j in (3, 0, 7, 4, 1, 6, 2, 5)]
    for p, d in zip(tail, errs):
        plant(p, d)
    pair = lambda p: (int(a[p]), int(b[p]))
    head = [pair(1), pair(2), pair(0)]
    by_err = [pair(p) for _, p in sorted(zip(errs, tail), reverse=True)]
    return a, b, {3: head, 9: head + [pair(3)] + by_err[:5]}


# ------------------------------------------------------------------ the two calls of the C ABI, on the emulator or on the device
import ctypes

EINVAL = -1
RECORD = np.dtype([("index", "<u8"), ("n1", "<u4"), ("n2", "<u4")])      # ErrPoint (csrc/mrcz_tools.hip)
GUARD, FILL = 64, 0xA5
FILLED = np.frombuffer(bytes([FILL]) * 16, RECORD)[0]


class Abi:
    """mrcz_err_hist / mrcz_err_collect of `lib` (libmrcz_sim.so or libmrcz_hip.so) on a context of its own, with device buffers
    from mrcz_dev_malloc"""

    def __init__(self, lib):
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        self.lib = lib
        for f, args in (("mrcz_create", [ctypes.POINTER(vp), i32, u32]), ("mrcz_dev_malloc", [vp, ctypes.POINTER(vp), u64]),
                        ("mrcz_dev_free", [vp, vp]), ("mrcz_copy_h2d", [vp, vp, vp, u64]), ("mrcz_copy_d2h", [vp, vp, vp, u64]),
                        ("mrcz_err_hist", [vp, vp, vp, u64, i32, u32, i32, vp]),
                        ("mrcz_err_collect", [vp, vp, vp, u64, u64, u32, vp, u64, u64, ctypes.POINTER(u64)])):
            getattr(lib, f).restype = i32
            getattr(lib, f).argtypes = args
        lib.mrcz_destroy.restype = None
        lib.mrcz_destroy.argtypes = [vp]
        self.ctx = vp()
        assert lib.mrcz_create(ctypes.byref(self.ctx), 0, 1) == 0

    def close(self):
        self.lib.mrcz_destroy(self.ctx)

    def malloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        assert self.lib.mrcz_dev_malloc(self.ctx, ctypes.byref(p), max(nbytes, 16)) == 0
        return p.value

    def free(self, *ptrs):
        for p in ptrs:
            assert self.lib.mrcz_dev_free(self.ctx, p) == 0

    def upload(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        if arr.nbytes:
            assert self.lib.mrcz_copy_h2d(self.ctx, p, arr.ctypes.data, arr.nbytes) == 0
        return p

    def download(self, p: int, count: int, dtype) -> np.ndarray:
        out = np.empty(count, dtype)
        if count:
            assert self.lib.mrcz_copy_d2h(self.ctx, out.ctypes.data, p, out.nbytes) == 0
        return out

    def hist(self, d1, d2, lo, hi, pass_, prefix, reset, want=True):
        """one call over the points [lo, hi); returns (status, the 2048 counters or None)"""
        h = np.full(2048, 0x5A5A5A5A5A5A5A5A, np.uint64)
        rc = self.lib.mrcz_err_hist(self.ctx, d1 + 4 * lo, d2 + 4 * lo, hi - lo, pass_, prefix, reset, h.ctypes.data if want else None)
        return rc, (h if want else None)

    def collect(self, d1, d2, lo, hi, base_index, thr, dp, cap, count_in):
        out = ctypes.c_uint64(0xDEAD)
        rc = self.lib.mrcz_err_collect(self.ctx, d1 + 4 * lo, d2 + 4 * lo, hi - lo, base_index, thr, dp, cap, count_in, ctypes.byref(out))
        return rc, out.value


def first_kth_key(a, b, K: int) -> int:
    """the statement's K-th key of the first range without a NaN difference (what the tool's first radix select looks for)"""
    import erroranalysis_ref as ref
    segs = segments(a, b)
    if not segs:
        return 0
    lo, hi = segs[0]
    return ref.kth_key(a[lo:hi], b[lo:hi], max(1, min(K, hi - lo)))


def prefixes(kth: int):
    return 0, kth >> 21, kth >> 10


def check_hist(abi: Abi, a, b, K: int, split_passes=()):
    """every pass against ref.hist with the prefix of the statement's K-th key; for the passes in `split_passes` also the protocol: three unequal
    calls (reset on the first, the counters asked for on the last), an empty call that reads them again, a reset"""
    import erroranalysis_ref as ref
    n = len(a)
    d1, d2 = abi.upload(a), abi.upload(b)
    kth = first_kth_key(a, b, K)
    try:
        for p in range(3):
            want = ref.hist(a, b, p, prefixes(kth)[p])
            rc, got = abi.hist(d1, d2, 0, n, p, prefixes(kth)[p], 1)
            assert rc == 0 and np.array_equal(got, want), (p, hex(kth), np.flatnonzero(got != want)[:8])
            assert int(want.sum()) == (n if p == 0 else int(np.count_nonzero(ref.err_key(a, b) >> np.uint32(ref.PASSES[p][2]) == prefixes(kth)[p])))
            if p not in split_passes:
                continue
            c1 = n // 7
            c2 = c1 + (n - c1) * 2 // 3
            assert abi.hist(d1, d2, 0, c1, p, prefixes(kth)[p], 1, want=False) == (0, None)
            assert abi.hist(d1, d2, c1, c2, p, prefixes(kth)[p], 0, want=False) == (0, None)
            rc, got = abi.hist(d1, d2, c2, n, p, prefixes(kth)[p], 0)
            assert rc == 0 and np.array_equal(got, want), (p, c1, c2)
            rc, got = abi.hist(d1, d2, 0, 0, p, prefixes(kth)[p], 0)              # n = 0: what was accumulated so far
            assert rc == 0 and np.array_equal(got, want)
            rc, got = abi.hist(d1, d2, 0, n, p, prefixes(kth)[p], 0)              # no reset: it adds up
            assert rc == 0 and np.array_equal(got, 2 * want)
            rc, got = abi.hist(d1, d2, 0, 0, p, prefixes(kth)[p], 1)              # reset = 1 clears
            assert rc == 0 and not got.any()
            assert abi.hist(d1, d2, 0, n, 3, 0, 1)[0] == EINVAL
            assert abi.hist(d1, d2, 0, n, -1, 0, 1)[0] == EINVAL
    finally:
        abi.free(d1, d2)


def check_collect(abi: Abi, a, b, thr: int, base_index: int = 0, count_in: int = 0, cap=None, pieces: int = 1):
    """the records of mrcz_err_collect against ref.collect: the count is exact whatever the capacity, the slots [count_in, cap)
    hold distinct true matches (all of them when they fit), and no byte outside those slots changes.  pieces = 2: two calls,
    the second continuing the first's count with base_index moved on, as the tool's batches do."""
    import erroranalysis_ref as ref
    n = len(a)
    want = ref.collect(a, b, thr, base_index)
    if cap is None:
        cap = count_in + len(want) + 3
    d1, d2 = abi.upload(a), abi.upload(b)
    dp = abi.upload(np.full(cap + GUARD, FILLED, RECORD))
    try:
        cut = n // 3 if pieces == 2 else n
        rc, cnt = abi.collect(d1, d2, 0, cut, base_index, thr, dp, cap, count_in)
        assert rc == 0
        if pieces == 2:
            assert cnt == count_in + len(ref.collect(a[:cut], b[:cut], thr))
            rc, cnt = abi.collect(d1, d2, cut, n, base_index + cut, thr, dp, cap, cnt)
            assert rc == 0
        assert cnt == count_in + len(want), (cnt, count_in, len(want))
        rec = abi.download(dp, cap + GUARD, RECORD)
        end = max(count_in, min(cap, cnt))
        got = [(int(r["index"]), int(r["n1"]), int(r["n2"])) for r in rec[count_in:end]]
        assert len(set(got)) == len(got), "a record was stored twice"
        assert set(got) <= want, sorted(set(got) - want)[:4]
        if cnt <= cap:
            assert set(got) == want
        assert (rec[:count_in] == FILLED).all(), "records below count_in were written"
        assert (rec[end:] == FILLED).all(), "records past the count, or past the capacity, were written"
    finally:
        abi.free(d1, d2, dp)
    return len(want)
