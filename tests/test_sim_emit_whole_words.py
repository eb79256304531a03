"""CPU-only twin of test_gpu_emit_whole_words.py: the product's HIP sources on the SIMT emulator, compressing into a buffer
pre-filled with 0xA5 (emit_whole_words_cases.py says why), record bytes against the oracle, pattern intact behind them.

Not here: the two-lane batch (eight chunks, minutes on the emulator; the emulator runs a lane's kernels in submission
order anyway, so it could not show a race between lanes).  The GPU file has it."""
import ctypes

import numpy as np
import pytest

import emit_whole_words_cases as cases
import util


def _compress_prefilled(sim, words, bits):
    n = len(words)
    din = util.aligned_empty(4 * n).view(np.uint32)
    din[:] = words
    cap = int(sim.lib.mrcz_records_bound(n)) + cases.SLACK
    dout = util.aligned_empty(cap)
    dout[:] = cases.PATTERN
    olen = ctypes.c_uint64()
    rc = sim.lib.mrcz_compress_chunks(sim.ctx, din.ctypes.data, n, 0, bits, dout.ctypes.data, cap, ctypes.byref(olen), None)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    return dout, int(olen.value)


def _splits(sim):
    sim.lib.mrcz_debug_emit_splits.restype = ctypes.c_int64
    sim.lib.mrcz_debug_emit_splits.argtypes = [ctypes.c_void_p]
    return int(sim.lib.mrcz_debug_emit_splits(sim.ctx))


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_prefilled_output_equals_the_oracle(simlib, oracle, name):
    words, bits = cases.SMALL[name]()
    got, olen = _compress_prefilled(simlib, words, bits)
    cases.check(got, olen, oracle.compress(words, bits)[17:], name)
    if name == "long_codes_b0":
        assert _splits(simlib) > 0      # the halving path was taken, with a carried word across the cut
    if name.startswith("gauss300k"):
        assert _splits(simlib) == 0     # (and the counter is not stuck)


def test_chunk_boundary_shares_dwords(simlib, oracle):
    words, bits = cases.CHUNK_PLUS()
    got, olen = _compress_prefilled(simlib, words, bits)
    cases.check(got, olen, oracle.compress(words, bits)[17:], "chunk_plus_1000_b8")
