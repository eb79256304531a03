"""CPU-only twin of test_gpu_emit_mixed.py: the product's HIP sources on the SIMT emulator over planes of mixed runs and
literals (emit_mixed_cases.py says which part of k_emit each input is for), compressed into a buffer pre-filled with 0xA5:
record bytes against the oracle, pattern intact behind them.

Not here: the two-lane batch (eight chunks: minutes on the emulator, which runs a lane's kernels in submission order
anyway).  The GPU file has it."""
import ctypes

import numpy as np
import pytest

import emit_mixed_cases as mixed
import emit_whole_words_cases as cases
import util


def _compress_prefilled(sim, words, bits=0):
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


def _check(sim, oracle, plane, name):
    words = mixed.words_of(plane)
    ref = oracle.compress(words, 0)
    got, olen = _compress_prefilled(sim, words)
    cases.check(got, olen, ref[17:], name)
    return ref


@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
def test_run_lengths(simlib, oracle, shuffled):
    _check(simlib, oracle, mixed.run_set(shuffled), f"runs shuffled={shuffled}")


@pytest.mark.parametrize("shift", mixed.SHIFTS)
def test_alignment(simlib, oracle, shift):
    _check(simlib, oracle, mixed.run_set(True, shift), f"runs shifted by {shift}")


def test_pairing(simlib, oracle):
    plane = mixed.pairing_plane()
    mixed.check_pairing_plane(plane)
    _check(simlib, oracle, plane, "pairing")


@pytest.mark.parametrize("second", sorted(mixed.BOUNDARY_TYPES))
def test_block_boundary(simlib, oracle, second):
    plane = mixed.boundary_plane(second)
    ref = _check(simlib, oracle, plane, f"boundary, second block {second}")
    mixed.check_boundary(plane, mixed.plane_stream(ref), second)


def test_long_codes(simlib, oracle):
    plane = mixed.long_code_plane()
    ref = _check(simlib, oracle, plane, "long codes")
    mixed.check_long_codes(plane, mixed.plane_stream(ref))
