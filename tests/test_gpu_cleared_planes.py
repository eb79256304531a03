"""GPU: byte planes that the mask or the "-s int" quantiser clears are neither stored by k_tile_summary nor loaded by k_histogram
and k_emit (cleared_planes_cases.py says what each input is for).  Every case is compressed into a buffer pre-filled with 0xA5
and compared with the CPU oracle byte for byte, the per-plane sums included; the probe, which runs the same sizing passes, must
return the sizes the compressor returns."""
import numpy as np
import pytest

import cleared_planes_cases as cases
import emit_whole_words_cases as whole
import probe_ref as pr
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from datacompressionfloat_amd import MrcZipCodec
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield c
    c.close()


def _device(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def _compress_prefilled(codec, dev, setting, first_chunk):
    import torch
    out = torch.full((codec.records_bound(dev.numel()) + whole.SLACK,), whole.PATTERN, dtype=torch.uint8, device="cuda")
    rec, planes = codec.compress_device(dev, 0 if setting == "int" else setting, first_chunk, out=out, int_mode=setting == "int")
    return out.cpu().numpy(), rec.numel(), [int(p) for p in planes]


def _check(codec, oracle, case, probe=True):
    name, words, setting, first_chunk = case
    record, sums = cases.expected(oracle, case)
    dev = _device(words)
    got, olen, planes = _compress_prefilled(codec, dev, setting, first_chunk)
    whole.check(got, olen, record, name)
    assert planes == sums, name
    if probe:
        size, pplanes, _ = codec.probe_device(dev, 0 if setting == "int" else setting, first_chunk, int_mode=setting == "int")
        assert (size, pplanes) == (olen, planes), name
    return record


@pytest.mark.parametrize("n", cases.NONFIRST_N)
def test_chunk_behind_the_first(codec, oracle, n):
    record = _check(codec, oracle, cases.nonfirst(n))
    cases.check_raw_edge(n, record)


@pytest.mark.parametrize("n", cases.FILESTART_N)
def test_file_start_chunk(codec, oracle, n):
    _check(codec, oracle, cases.filestart(n))


def test_run_from_the_header_into_cleared_tiles(codec, oracle):
    case = cases.filestart_run()
    cases.check_run_from_header(case[1])
    _check(codec, oracle, case)


@pytest.mark.parametrize("bits", cases.LEVELS)
def test_other_mask_levels(codec, oracle, bits):
    _check(codec, oracle, cases.level(bits))


@pytest.mark.parametrize("n", cases.INT_FILESTART_N)
def test_int_mode_file_start(codec, oracle, n):
    _check(codec, oracle, cases.int_filestart(n))


def test_int_mode_chunk_behind_the_first(codec, oracle):
    _check(codec, oracle, cases.int_nonfirst())


@pytest.mark.parametrize("n", cases.STALE_N)
def test_stale_workspace(codec, oracle, n):
    """every plane row of the workspace holds 0xA5 before each case: a read of a byte this call did not store changes the records"""
    stale = _device(cases.stale_words(n))
    for case in cases.stale_cases(n):
        codec.compress_device(stale, 0)
        _check(codec, oracle, case, probe=False)


def test_file_start_and_later_chunk_in_one_grid(codec, oracle):
    """One call of two chunks at b = 8: chunk 0 starts the file (its tile 0 of plane 0 is loaded), chunk 1 does not (every tile
    of its plane 0 is cleared).  Twice into the same pre-filled buffer."""
    import torch
    words, bits = cases.two_chunk_words()
    ref = oracle.compress(words, bits, threads=16)
    dev = _device(words)
    out = torch.full((codec.records_bound(len(words)) + whole.SLACK,), whole.PATTERN, dtype=torch.uint8, device="cuda")
    for turn in range(2):
        rec, planes = codec.compress_device(dev, bits, 0, out=out)
        whole.check(out.cpu().numpy(), rec.numel(), ref[17:], f"two chunks turn {turn}")
        assert [int(p) for p in planes] == pr.plane_sums(ref, len(words))
    size, pplanes, _ = codec.probe_device(dev, bits)
    assert (size, pplanes) == (rec.numel(), [int(p) for p in planes])
