"""CPU-only twin of test_gpu_cleared_planes.py: the product's HIP sources on the SIMT emulator (cleared_planes_cases.py says what
each input is for).  Every case is compressed into a buffer pre-filled with 0xA5 and compared with the CPU oracle byte for byte,
the per-plane sums included; the probe, which runs the same sizing passes, must return the sizes the compressor returns.

The "-s int" case of a chunk that does not start a file is here too: the oracle codes it as the second chunk of a file whose
first chunk is all zeros, as it does for the mask.

Not here: the two-chunk call with a file-start and a later chunk in one grid (a whole chunk on the emulator); the GPU file has it.

Mutations tried by hand on this file, each of which makes the named cases fail:
  tile_cleared ignores unmasked_below (tile 0 of a file's first chunk taken as zeros)
        -> every test_file_start_chunk case, test_run_from_the_header_into_cleared_tiles, test_int_mode_file_start, and
           test_stale_workspace at every size
  k_emit's RAW tail still reads pl[] for a cleared tile
        -> test_stale_workspace[13] alone: only a workspace that an earlier call filled shows it
  k_histogram still loads a cleared tile (the histograms count what an earlier call left)
        -> test_stale_workspace[4097], and test_other_mask_levels[12, 16, 24, 32] and test_int_mode_chunk_behind_the_first
           behind the cases that ran before them on the same context (at 14 words the block is static with any histogram)
  k_emit's STORED copy still reads the plane for a cleared tile
        -> nothing: no input was found that puts a stored block into a cleared tile (a run of zeros always codes shorter);
           the branch is there for the rule "no read of a byte this call did not store", not for a known case"""
import ctypes

import numpy as np
import pytest

import cleared_planes_cases as cases
import emit_whole_words_cases as whole
import probe_ref as pr
import util


@pytest.fixture(scope="module")
def sim(simlib):
    pr.bind(simlib.lib)
    return simlib


def _compress_prefilled(sim, words, setting, first_chunk):
    n = len(words)
    din = util.aligned_empty(4 * n).view(np.uint32)
    din[:] = words
    cap = int(sim.lib.mrcz_records_bound(n)) + whole.SLACK
    dout = util.aligned_empty(cap)
    dout[:] = whole.PATTERN
    olen = ctypes.c_uint64()
    planes = (ctypes.c_uint64 * 4)()
    if setting == "int":
        rc = sim.lib.mrcz_compress_chunks_int8(sim.ctx, din.ctypes.data, n, first_chunk, dout.ctypes.data, cap, ctypes.byref(olen), planes)
    else:
        rc = sim.lib.mrcz_compress_chunks(sim.ctx, din.ctypes.data, n, first_chunk, setting, dout.ctypes.data, cap, ctypes.byref(olen), planes)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    return dout, int(olen.value), list(planes)


def _probe_sizes(sim, words, setting, first_chunk):
    din = util.aligned_empty(4 * len(words)).view(np.uint32)
    din[:] = words
    olen = ctypes.c_uint64(12345)
    planes = (ctypes.c_uint64 * 4)()
    xform, bits = (pr.INT8, 0) if setting == "int" else (pr.MASK, setting)
    rc = sim.lib.mrcz_probe_chunks(sim.ctx, din.ctypes.data, len(words), first_chunk, xform, bits, 0.0, -1.0, -1.0, None, ctypes.byref(olen), planes)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    return int(olen.value), list(planes)


def _check(sim, oracle, case, probe=True):
    name, words, setting, first_chunk = case
    record, sums = cases.expected(oracle, case)
    got, olen, planes = _compress_prefilled(sim, words, setting, first_chunk)
    whole.check(got, olen, record, name)
    assert planes == sums, name
    if probe:
        assert _probe_sizes(sim, words, setting, first_chunk) == (olen, planes), name
    return record


@pytest.mark.parametrize("n", cases.NONFIRST_N)
def test_chunk_behind_the_first(sim, oracle, n):
    record = _check(sim, oracle, cases.nonfirst(n))
    cases.check_raw_edge(n, record)


@pytest.mark.parametrize("n", cases.FILESTART_N)
def test_file_start_chunk(sim, oracle, n):
    _check(sim, oracle, cases.filestart(n))


def test_run_from_the_header_into_cleared_tiles(sim, oracle):
    case = cases.filestart_run()
    cases.check_run_from_header(case[1])
    _check(sim, oracle, case)


@pytest.mark.parametrize("bits", cases.LEVELS)
def test_other_mask_levels(sim, oracle, bits):
    _check(sim, oracle, cases.level(bits))


@pytest.mark.parametrize("n", cases.INT_FILESTART_N)
def test_int_mode_file_start(sim, oracle, n):
    _check(sim, oracle, cases.int_filestart(n))


def test_int_mode_chunk_behind_the_first(sim, oracle):
    _check(sim, oracle, cases.int_nonfirst())


@pytest.mark.parametrize("n", cases.STALE_N)
def test_stale_workspace(sim, oracle, n):
    """every plane row of the workspace holds 0xA5 before each case: a read of a byte this call did not store changes the records"""
    for case in cases.stale_cases(n):
        sim.compress_records(cases.stale_words(n), 0)
        _check(sim, oracle, case, probe=False)
