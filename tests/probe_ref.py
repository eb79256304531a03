"""What the probe tests expect, from the CPU oracle and numpy alone (never from the code under test): the container a setting gives
(oracle), what it decodes to (tests/util.erase_expected, abs_error_ref.abs_round, the oracle's int-mode decode) and the numpy fold of
tests/compare_ref.py over original and decode.  A setting is ("bits", b), ("abs", eps) with eps a float32, or ("int",)."""
import ctypes

import numpy as np

import compare_ref as ref
import util
from abs_error_ref import abs_round

CHK = util.CHUNK
N_SMALL = 300001          # one short chunk, no multiple of four: the last group of the fold takes 4-byte loads
MASK, ABS, INT8 = 0, 1, 2  # MRCZ_PROBE_*
EINVAL = -1


def small_volume() -> np.ndarray:
    """300 001 words: arbitrary header bits, noise, a constant run, +-0, denormals, +-Inf, and NaNs whose only mantissa bits lie in the
    low byte planes (a mask turns them into Inf: a special that differs), the last words of the ragged tail among the specials"""
    w = util.gauss_words(N_SMALL, seed=77, header=False)
    w[:256] = util.kat_words(256)
    w[40000:90000] = 0x41200000                                     # a constant run of 10.0f
    special = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000003, 0x00012345, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                        0x7F800001, 0xFF8000FF, 0x7F800100, 0xFF80FF00, 0x7FFFFFFF, 0x3C23D70A, 0xBC23D70B, 0x42FE0001, 0xC3000001], np.uint32)
    for a in (256, 1000, 150001, N_SMALL - len(special)):
        w[a: a + len(special)] = special
    return w


def bind(lib):
    vp, u64, i32, f32, f64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_float, ctypes.c_double
    lib.mrcz_probe_chunks.argtypes = [vp, vp, u64, u64, i32, i32, f32, f64, f64, vp, ctypes.POINTER(u64), vp]
    lib.mrcz_compare_finish.argtypes = [vp, vp, u64, u64, vp]


def abi_args(setting):
    """(xform, bits, eps) of mrcz_probe_chunks"""
    if setting[0] == "bits":
        return MASK, int(setting[1]), 0.0
    if setting[0] == "abs":
        return ABS, 0, float(setting[1])
    return INT8, 0, 0.0


def container(oracle, w: np.ndarray, setting) -> bytes:
    if setting[0] == "bits":
        return oracle.compress(w.tobytes(), int(setting[1]))
    if setting[0] == "abs":
        return oracle.compress(abs_round(w, np.float32(setting[1])).tobytes(), 0)
    return oracle.compress_int(w.tobytes())


def decoded(oracle, w: np.ndarray, setting, z: bytes = None) -> np.ndarray:
    if setting[0] == "bits":
        return util.erase_expected(w, int(setting[1]))
    if setting[0] == "abs":
        return abs_round(w, np.float32(setting[1]))
    return np.frombuffer(oracle.uncompress(z if z is not None else container(oracle, w, setting), int_mode=True), np.uint32)


def record_offsets(z: bytes, nfl: int) -> list:
    """offsets in the container of every chunk record and of the end of the last"""
    offs, off = [], 17
    for _ in range((nfl + CHK - 1) // CHK):
        offs.append(off)
        off += 16 + int(sum(int(x) & 0x7fffffff for x in np.frombuffer(z[off: off + 16], "<u4")))
    assert off == len(z)
    return offs + [off]


def plane_sums(z: bytes, nfl: int, first_chunk: int = 0) -> list:
    """per plane the sum over the chunks' headers of (payload length + 4): mzip_t.zfsz"""
    s = [0, 0, 0, 0]
    for off in record_offsets(z, nfl)[first_chunk:-1]:
        for j, x in enumerate(np.frombuffer(z[off: off + 16], "<u4")):
            s[j] += (int(x) & 0x7fffffff) + 4
    return s


def expectation(oracle, w: np.ndarray, setting, eps_abs=None, eps_rel=None) -> dict:
    """everything a probe of the whole file `w` must return"""
    z = container(oracle, w, setting)
    dec = decoded(oracle, w, setting, z)
    chunks = ref.fold_chunks(w, dec, CHK, eps_abs, eps_rel)
    return {"container_bytes": len(z), "record_bytes": len(z) - 17, "plane_bytes": plane_sums(z, len(w)), "chunks": chunks,
            "total": ref.total(chunks), "offsets": record_offsets(z, len(w)), "z": z}


def records(raw: bytes, nchunks: int) -> list:
    sz = ctypes.sizeof(ref.Compare)
    return [ref.as_dict(ref.Compare.from_buffer_copy(raw[c * sz: (c + 1) * sz])) for c in range(nchunks)]


def assert_probe(size, planes, recs, want, what=""):
    assert size == want["record_bytes"], (what, size, want["record_bytes"])
    assert list(planes) == want["plane_bytes"], (what, list(planes), want["plane_bytes"])
    assert len(recs) == len(want["chunks"])
    for c, (g, x) in enumerate(zip(recs, want["chunks"])):
        ref.assert_matches(g, x, (what, "chunk", c))
