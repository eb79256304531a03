"""numpy statement of the absolute-error mode (include/mrcz_hip.h, mrcz_compress_chunks_abs): the words a container written
with bound eps decodes to.  Every abs-error test compares against this function."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def f32_toward_zero(eps: float) -> np.float32:
    """a double bound as the float32 the codec uses: rounded toward zero, so that the bound holds for the value given"""
    eps = float(eps)
    if np.isfinite(eps) and abs(eps) > FLT_MAX:
        return np.float32(np.copysign(FLT_MAX, eps))
    with np.errstate(over="ignore"):
        f = np.float32(eps)
    if np.isfinite(f) and abs(float(f)) > abs(eps):
        f = np.nextafter(f, np.float32(0))
    return f


def abs_params(eps):
    """(q, E): q = floor(log2(eps)), E = bits(eps) of a float32 eps that is finite and > 0"""
    e32 = np.float32(eps)
    assert np.isfinite(e32) and e32 > 0, eps
    E = int(np.array([e32], np.float32).view(np.uint32)[0])
    exp = E >> 23
    q = exp - 127 if exp else -150 + E.bit_length()
    return q, E


def abs_round(words: np.ndarray, eps, first_word_index: int = 0) -> np.ndarray:
    """words of a file from file word `first_word_index` on; words at file index < 256 (the MRC header) are kept as -b keeps
    them.  eps is taken as a float32 (pass f32_toward_zero(x) for a double x)."""
    q, E = abs_params(eps)
    w = np.ascontiguousarray(words, dtype=np.uint32).astype(np.int64)
    e = (w >> 23) & 0xFF
    mag = w & 0x7FFFFFFF
    u = np.maximum(e, 1) - 150
    b = np.clip(q - u + 1, 0, 23)
    half = (np.int64(1) << b) >> 1
    r = (mag + half) & ~((np.int64(1) << b) - 1)
    r = np.where(r >= 0x7F800000, mag & ~(half - 1), r)
    out = np.where(mag <= E, 0, (w & 0x80000000) | r)
    out = np.where(e == 0xFF, w, out)
    keep = max(0, min(len(w), 256 - first_word_index))
    out[:keep] = w[:keep]
    return out.astype(np.uint32)


def max_abs_error(a: np.ndarray, b: np.ndarray) -> float:
    """max |a - b| in float64 over the words where both are finite"""
    with np.errstate(invalid="ignore"):  # signalling NaNs
        x = np.asarray(a, np.uint32).view(np.float32).astype(np.float64)
        y = np.asarray(b, np.uint32).view(np.float32).astype(np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    return float(np.max(np.abs(x[ok] - y[ok]), initial=0.0))


def edge_words() -> np.ndarray:
    """NaNs, infinities, zeros, denormals, FLT_MAX and words on either side of the binade edges, both signs"""
    pos = [0x00000000, 0x00000001, 0x00000002, 0x00000003, 0x007FFFFF, 0x00400000, 0x00800000, 0x00800001, 0x00FFFFFF,
           0x3F800000, 0x3F7FFFFF, 0x3FFFFFFF, 0x3F800001, 0x3C23D70A, 0x358637BD, 0x7149F2CA, 0x7E967699,
           0x7F7FFFFF, 0x7F7FFFFE, 0x7F7F0000, 0x7F000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]
    pos = np.array(pos, np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)])
