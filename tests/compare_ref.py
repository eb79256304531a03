"""numpy statement of compare decode (include/mrcz_hip.h, mrcz_uncompress_compare / mrcz_compare_finish): the summary of decoded
words against original words.  Every compare test takes its expectations from here, never from the code under test.

Per point every value is one correctly rounded IEEE double operation, so counts, maxima, minima and indices are compared exactly.
The sums are compared against math.fsum of the numpy terms with the tolerance that follows from the definition and nothing else:
any order of adding n doubles is within (n + 2) * 2^-53 * fsum(|terms|) of the exact sum; the + 2 covers the rounding of d * d,
which the device may contract into an fma with the running sum."""
import ctypes
import math

import numpy as np

NONE = 0xFFFFFFFFFFFFFFFF
COUNTS = ("n", "n_header_diff", "n_diff", "n_finite", "n_special_diff", "n_over_abs", "n_over_rel", "first_over", "max_err_index",
          "max_rel_index")
EXACT = ("max_err", "max_rel", "orig_min", "orig_max")
SUMS = ("sum_err", "sum_abs_err", "sum_err2", "orig_sum", "orig_sum2")
FIELDS = COUNTS + ("max_err", "max_rel", "sum_err", "sum_abs_err", "sum_err2", "orig_min", "orig_max", "orig_sum", "orig_sum2")


class Compare(ctypes.Structure):
    """mrcz_compare_t"""
    _fields_ = [(k, ctypes.c_uint64) for k in COUNTS] + [(k, ctypes.c_double) for k in FIELDS[len(COUNTS):]]


def as_dict(rec) -> dict:
    return {k: getattr(rec, k) for k in FIELDS}


def _on(eps):
    return eps is not None and eps >= 0        # negative, NaN or None: the check is off


def fold(orig: np.ndarray, dec: np.ndarray, first_word: int = 0, eps_abs=None, eps_rel=None, exact_sums=True) -> dict:
    """summary of file words [first_word, first_word + len(orig)).  Returns the fields of mrcz_compare_t, and under "abs" the sum
    of the absolute values of every sum's terms (the tolerance's scale).  exact_sums: math.fsum; otherwise extended precision."""
    orig = np.ascontiguousarray(orig, np.uint32)
    dec = np.ascontiguousarray(dec, np.uint32)
    assert orig.shape == dec.shape
    idx = first_word + np.arange(len(orig), dtype=np.uint64)
    hdr = idx < 256
    with np.errstate(invalid="ignore"):
        a = orig.view(np.float32).astype(np.float64)
        b = dec.view(np.float32).astype(np.float64)
    diff = orig != dec
    fin = np.isfinite(a) & np.isfinite(b) & ~hdr
    spec = ~hdr & ~fin & diff
    af, bf, ix = a[fin], b[fin], idx[fin]
    d = bf - af
    err = np.abs(d)
    mag = np.abs(af)
    rel = np.zeros_like(err)
    big = mag > 1e-3
    rel[big] = err[big] / mag[big]
    oa = err > eps_abs if _on(eps_abs) else np.zeros(len(err), bool)
    orl = rel > eps_rel if _on(eps_rel) else np.zeros(len(err), bool)
    over = np.concatenate([ix[oa | orl], idx[spec]])
    r = {"n": int((~hdr).sum()), "n_header_diff": int((hdr & diff).sum()), "n_diff": int((~hdr & diff).sum()), "n_finite": int(fin.sum()),
         "n_special_diff": int(spec.sum()), "n_over_abs": int(oa.sum()), "n_over_rel": int(orl.sum()),
         "first_over": int(over.min()) if len(over) else NONE}
    if len(err):
        r["max_err"], r["max_err_index"] = float(err.max()), int(ix[np.argmax(err)])     # argmax: the first (lowest) index
        r["max_rel"], r["max_rel_index"] = float(rel.max()), int(ix[np.argmax(rel)])
        r["orig_min"], r["orig_max"] = float(af.min()), float(af.max())
    else:
        r.update(max_err=0.0, max_rel=0.0, max_err_index=NONE, max_rel_index=NONE, orig_min=math.inf, orig_max=-math.inf)
    terms = {"sum_err": d, "sum_abs_err": err, "sum_err2": d * d, "orig_sum": af, "orig_sum2": af * af}
    r["abs"] = {}
    for k, t in terms.items():
        if exact_sums:
            r[k], r["abs"][k] = math.fsum(t), math.fsum(np.abs(t))
        else:
            r[k], r["abs"][k] = float(np.sum(t, dtype=np.longdouble)), float(np.sum(np.abs(t), dtype=np.longdouble))
    return r


def total(chunks: list) -> dict:
    """mrcz_compare_finish over per-chunk folds (in chunk order); the sums exactly (fsum of the chunks' exact sums)"""
    t = {k: sum(c[k] for c in chunks) for k in COUNTS[:7]}
    t["first_over"] = min(c["first_over"] for c in chunks)
    have = [c for c in chunks if c["n_finite"]]
    for m, i in (("max_err", "max_err_index"), ("max_rel", "max_rel_index")):
        best = max((c[m] for c in have), default=0.0)
        t[m] = best
        t[i] = min((c[i] for c in have if c[m] == best), default=NONE)
    t["orig_min"] = min((c["orig_min"] for c in chunks), default=math.inf)
    t["orig_max"] = max((c["orig_max"] for c in chunks), default=-math.inf)
    t["abs"] = {}
    for k in SUMS:
        t[k] = math.fsum(c[k] for c in chunks)
        t["abs"][k] = math.fsum(c["abs"][k] for c in chunks)
    return t


def assert_matches(got: dict, want: dict, what="", slack=2):
    """counts, extremes and indices exactly; sums within (n_finite + slack) * 2^-53 * sum|terms| (module docstring)"""
    for k in COUNTS + EXACT:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in SUMS:
        tol = (want["n_finite"] + slack) * 2.0 ** -53 * want["abs"][k]
        assert abs(got[k] - want[k]) <= tol, (what, k, got[k], want[k], tol)


def fold_chunks(orig, dec, chk, eps_abs=None, eps_rel=None, exact_sums=True) -> list:
    return [fold(orig[a: a + chk], dec[a: a + chk], a, eps_abs, eps_rel, exact_sums) for a in range(0, len(orig), chk)]


def derived(t: dict) -> dict:
    """mean_err, rmse, psnr_db as mrc_verify and MrcZipCodec.verify derive them"""
    n = t["n_finite"]
    mean = t["sum_err"] / n if n else 0.0
    rmse = math.sqrt(t["sum_err2"] / n) if n else 0.0
    psnr = math.inf if rmse == 0 else 20.0 * math.log10((t["orig_max"] - t["orig_min"]) / rmse) if n else math.inf
    return {"mean_err": mean, "rmse": rmse, "psnr_db": psnr}
