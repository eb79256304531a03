"""CPU-only: the absolute-error mode of the compressor (k_tile_summary<Xform::AbsErr>, k_erase_abs) run by the SIMT emulator,
pinned bit for bit: the records equal the oracle's -b 0 records of the words abs_error_ref.abs_round gives, and they decode
to those words."""
import ctypes

import numpy as np
import pytest

import util
from abs_error_ref import abs_round, edge_words, f32_toward_zero, max_abs_error

EPS = [2.0 ** -149, 1e-6, 0.01, 1.0, 1e30]
EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    s.lib.mrcz_compress_chunks_abs.argtypes = [vp, vp, u64, u64, ctypes.c_float, vp, u64, ctypes.POINTER(u64), vp]
    s.lib.mrcz_compress_chunks_abs_async.argtypes = [vp, vp, u64, u64, ctypes.c_float, vp, u64, vp]
    s.lib.mrcz_erase_abs.argtypes = [vp, vp, u64, u64, ctypes.c_float]
    return s


def _compress_abs(sim, words, eps, first_chunk=0):
    n = len(words)
    din = util.aligned_empty(4 * n).view(np.uint32)
    din[:] = words
    cap = int(sim.lib.mrcz_records_bound(n))
    dout = util.aligned_empty(cap + 8)
    olen = ctypes.c_uint64()
    rc = sim.lib.mrcz_compress_chunks_abs(sim.ctx, din.ctypes.data, n, first_chunk, eps, dout.ctypes.data, cap, ctypes.byref(olen), None)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    assert np.array_equal(din, words)  # the input is read, not rounded in place
    return dout[:olen.value].tobytes()


def _erase_abs(sim, words, eps, first_word_index=0):
    d = util.aligned_empty(4 * len(words)).view(np.uint32)
    d[:] = words
    assert sim.lib.mrcz_erase_abs(sim.ctx, d.ctypes.data, len(words), first_word_index, eps) == 0
    return d.copy()


def _check(sim, oracle, words, eps, first_chunk=0):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    eps = f32_toward_zero(eps)
    want = abs_round(words, eps, first_word_index=first_chunk * util.CHUNK)
    got = _compress_abs(sim, words, eps, first_chunk)
    assert got == oracle.compress(want.tobytes(), 0)[17:], (len(words), float(eps), first_chunk)
    assert np.array_equal(sim.uncompress_records(got, len(words)), want)
    assert np.array_equal(_erase_abs(sim, words, eps, first_chunk * util.CHUNK), want)
    assert max_abs_error(words, want) <= float(eps)
    return want


def _random_bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("eps", EPS)
def test_gauss_poisson_and_random_bits(sim, oracle, eps):
    for w in (util.gauss_words(30000, seed=5), util.poisson_words(20000, seed=6), _random_bits(9000, seed=7)):
        _check(sim, oracle, w, eps)


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_ragged_sizes_around_the_header_and_the_tile(sim, oracle, n):
    w = util.gauss_words(n, seed=n)
    w[: min(n, 256)] = _random_bits(min(n, 256), seed=n)  # header words that the rounding would change: kept as they are
    for eps in (1e-6, 0.01, 1.0):
        _check(sim, oracle, w, eps)


@pytest.mark.parametrize("eps", EPS)
def test_a_chunk_past_the_first_rounds_its_first_256_words_too(sim, oracle, eps):
    w = util.gauss_words(5000, seed=9)
    want = _check(sim, oracle, w, eps, first_chunk=1)
    assert not np.array_equal(want[:256], w[:256]) or float(f32_toward_zero(eps)) < 1e-30


@pytest.mark.parametrize("eps", EPS + [3.4e38])
def test_nan_inf_zeros_denormals_and_flt_max(sim, oracle, eps):
    e = edge_words()
    w = np.concatenate([np.zeros(256, np.uint32), np.tile(e, 40), util.gauss_words(3000, seed=3, header=False)])
    want = _check(sim, oracle, w, eps)
    f, g = w.view(np.float32), want.view(np.float32)
    assert np.array_equal(np.isnan(f), np.isnan(g)) and np.array_equal(w[np.isinf(f)], want[np.isinf(f)])
    assert np.all(np.isfinite(g[np.isfinite(f)]))  # the rounding never carries into Inf


def test_values_within_eps_become_zero_and_the_rest_keep_their_sign(sim, oracle):
    w = np.concatenate([np.zeros(256, np.uint32), util.gauss_words(20000, seed=12, header=False)])
    w[256:] = (w[256:].view(np.float32) - np.float32(10.0)).view(np.uint32)  # centred: many values within eps of 0
    want = _check(sim, oracle, w, 0.5)
    f, g = w[256:].view(np.float32), want[256:].view(np.float32)
    small = np.abs(f) <= np.float32(0.5)
    assert small.any() and np.all(want[256:][small] == 0)
    assert np.all(np.signbit(f[~small]) == np.signbit(g[~small]))


def test_larger_bounds_zero_more_low_bits(sim):
    w = util.gauss_words(50000, seed=13)
    zero_low = [np.mean(abs_round(w, f32_toward_zero(e))[256:] & 0xFFFF == 0) for e in (1e-4, 1e-3, 1e-2, 1e-1)]
    assert zero_low == sorted(zero_low) and zero_low[-1] > 0.9


@pytest.mark.parametrize("eps", [0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_bad_bounds_are_refused(sim, eps):
    n = 1000
    din = util.aligned_empty(4 * n).view(np.uint32)
    din[:] = util.gauss_words(n)
    cap = int(sim.lib.mrcz_records_bound(n))
    dout = util.aligned_empty(cap + 8)
    olen = ctypes.c_uint64(123)
    assert sim.lib.mrcz_compress_chunks_abs(sim.ctx, din.ctypes.data, n, 0, eps, dout.ctypes.data, cap, ctypes.byref(olen), None) == EINVAL
    assert olen.value == 0
    res = np.zeros(5, np.uint64)
    assert sim.lib.mrcz_compress_chunks_abs_async(sim.ctx, din.ctypes.data, n, 0, eps, dout.ctypes.data, cap, res.ctypes.data) == EINVAL
    assert sim.lib.mrcz_erase_abs(sim.ctx, din.ctypes.data, n, 0, eps) == EINVAL
    assert np.array_equal(din, util.gauss_words(n))
