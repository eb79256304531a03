"""The statement of erroranalysis in numpy and plain Python: what mrcz_err_hist / mrcz_err_collect count and hand back, and what
the tool prints.  It reads nothing from the code under test; tests/test_sim_erroranalysis.py, the CLI tests on the emulator and
tests/test_gpu_erroranalysis.py take every expectation from here, and one CPU test holds it against the reference's own binary.

A point is a pair of float32 words (n1 from the original file, n2 from the decoded one):

    err     = fabsf(n2 - n1)                       one float32 subtraction, denormals kept
    relErr  = |n1| > 10E-4 ? err / |n1| : 0        float32 division; the test against 10E-4 is made in double
    key     = the bit pattern of err, 0xffffffff where err is NaN

The tool prints the first K points after K bubble passes from the end of the array; a pass swaps two neighbours when the later
one has the larger err, or when the errs are within 1e-7f and the later one has the larger relErr.  No comparison with a NaN is
true, so a point with a NaN err stays where it is and nothing passes it."""
import numpy as np

NAN_KEY = 0xFFFFFFFF
# (shift, bits, prefix shift) of the three radix passes (include/mrcz_hip.h, mrcz_err_hist); pass 0 has no prefix
PASSES = ((21, 11, None), (10, 11, 21), (0, 10, 10))
ZERO = np.float32(1e-7)


def _f32(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def err_f32(a, b) -> np.ndarray:
    """fabsf(n2 - n1) as float32"""
    with np.errstate(all="ignore"):
        return np.abs(_f32(b) - _f32(a))


def err_key(a, b) -> np.ndarray:
    e = err_f32(a, b)
    k = e.view(np.uint32).copy()
    k[np.isnan(e)] = NAN_KEY
    return k


def hist(a, b, pass_: int, prefix: int) -> np.ndarray:
    shift, bits, pshift = PASSES[pass_]
    k = err_key(a, b)
    if pshift is not None:
        k = k[(k >> np.uint32(pshift)) == np.uint32(prefix)]
    return np.bincount((k >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=2048).astype(np.uint64)


def collect(a, b, thr: int, base_index: int = 0) -> set:
    k = err_key(a, b)
    return {(base_index + int(i), int(a[i]), int(b[i])) for i in np.flatnonzero(k >= np.uint32(thr))}


def kth_key(a, b, K: int) -> int:
    """the K-th largest key (K = 1: the largest) of a range without NaN differences"""
    k = np.sort(err_key(a, b))
    assert 1 <= K <= len(k) and k[-1] != NAN_KEY
    return int(k[len(k) - K])


def _spell(x: np.float32, upper: bool) -> str:
    """glibc's %f / %E of a float (promoted to double: the sign of a NaN survives)"""
    if np.isnan(x):
        s = "-nan" if int(np.float32(x).view(np.uint32)) >> 31 else "nan"
        return s.upper() if upper else s
    return ("%E" if upper else "%f") % float(x)


def rel_f32(a, b) -> np.ndarray:
    e32, n1 = err_f32(a, b), np.abs(_f32(a))
    with np.errstate(all="ignore"):
        return np.where(n1.astype(np.float64) > 10E-4, e32 / n1, np.float32(0)).astype(np.float32)


def print_points(a, b) -> str:
    """one line "%f %f %f %E %f %E" of n1, n2, err, err, relErr, relErr for every point, in the order given"""
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    cols = (_f32(a), _f32(b), err_f32(a, b), err_f32(a, b), rel_f32(a, b), rel_f32(a, b))
    return "".join(" ".join(_spell(c[p], u) for c, u in zip(cols, (False, False, False, True, False, True))) + "\n" for p in range(len(a)))


def lines(a, b, K: int) -> str:
    """stdout of `erroranalysis -a A -b B -k K`: the literal K passes over the whole array"""
    n = min(len(a), len(b))
    a, b = np.ascontiguousarray(a[:n], dtype=np.uint32), np.ascontiguousarray(b[:n], dtype=np.uint32)
    K = max(0, min(int(K), n))
    e32, r32 = err_f32(a, b), rel_f32(a, b)
    err32 = [np.float32(x) for x in e32]        # float32 scalars: err32[i] - err32[j] below is a float32 subtraction
    err, rel = e32.tolist(), r32.tolist()       # the same values as Python floats: comparisons only
    order = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(K):
            for i in range(n - 1, k, -1):
                x, y = order[i], order[i - 1]
                if err[x] > err[y]:
                    order[i], order[i - 1] = y, x
                elif abs(err32[x] - err32[y]) <= ZERO:
                    if rel[x] > rel[y]:
                        order[i], order[i - 1] = y, x
    return print_points(a[order[:K]], b[order[:K]])
