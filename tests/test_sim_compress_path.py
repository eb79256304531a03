"""CPU-only twin of test_gpu_compress_path.py: the product's HIP sources on the SIMT emulator (compress_path_cases.py says
which kernel each input is for).  Every case is compressed into a buffer pre-filled with 0xA5 and compared with the CPU
oracle byte for byte; the probe, which runs the same sizing passes, must return the sizes the compressor returns.

Not here: the whole constant chunk and the two-lane batch (minutes on the emulator); the GPU file has them.

Mutations tried by hand on this file, each of which makes the named case fail:
  k_block_reduce leaves out wave 1's partial row            -> constant-294912 (nine segments) and every longer block
  k_stream_layout takes .x (dynamic bits) for a static block -> static_block_cut_by_a_segment_boundary
(the third, an off-by-one in k_huffman's per-workgroup block prefix, needs two streams with blocks: it fails every case
here, and the two-lane case of the GPU file)"""
import ctypes

import numpy as np
import pytest

import compress_path_cases as cases
import emit_mixed_cases as mixed
import emit_whole_words_cases as whole
import probe_ref as pr
import util


@pytest.fixture(scope="module")
def sim(simlib):
    pr.bind(simlib.lib)
    return simlib


def _compress_prefilled(sim, words, bits):
    n = len(words)
    din = util.aligned_empty(4 * n).view(np.uint32)
    din[:] = words
    cap = int(sim.lib.mrcz_records_bound(n)) + whole.SLACK
    dout = util.aligned_empty(cap)
    dout[:] = whole.PATTERN
    olen = ctypes.c_uint64()
    planes = (ctypes.c_uint64 * 4)()
    rc = sim.lib.mrcz_compress_chunks(sim.ctx, din.ctypes.data, n, 0, bits, dout.ctypes.data, cap, ctypes.byref(olen), planes)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    return dout, int(olen.value), list(planes)


def _probe_sizes(sim, words, bits):
    din = util.aligned_empty(4 * len(words)).view(np.uint32)
    din[:] = words
    olen = ctypes.c_uint64(12345)
    planes = (ctypes.c_uint64 * 4)()
    rc = sim.lib.mrcz_probe_chunks(sim.ctx, din.ctypes.data, len(words), 0, pr.MASK, bits, 0.0, -1.0, -1.0, None, ctypes.byref(olen), planes)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    return int(olen.value), list(planes)


def _check(sim, oracle, words, bits, name, probe=True):
    z = oracle.compress(words, bits)
    got, olen, planes = _compress_prefilled(sim, words, bits)
    whole.check(got, olen, z[17:], name)
    assert planes == pr.plane_sums(z, len(words)), name
    if probe:
        assert _probe_sizes(sim, words, bits) == (olen, planes), name
    return z


@pytest.mark.parametrize("n", sorted(cases.CONSTANT_N))
def test_constant_planes_over_many_pairs(sim, oracle, n):
    z = _check(sim, oracle, cases.constant_words(n), 0, f"constant-{n}")
    cases.check_constant(n, z)


def test_sparse_plane_with_many_match_lengths(sim, oracle):
    z = _check(sim, oracle, mixed.words_of(cases.sparse_plane()), 0, "sparse")
    cases.check_sparse(z)


def test_static_block_cut_by_a_segment_boundary(sim, oracle):
    plane, cut = cases.static_cut_plane()
    z = _check(sim, oracle, mixed.words_of(plane), 0, "static cut")
    cases.check_static_cut(plane, cut, z)


@pytest.mark.parametrize("name", cases.KEPT)
def test_kept_inputs(sim, oracle, name):
    words, bits = cases.kept(name)
    _check(sim, oracle, words, bits, name, probe=False)
