"""GPU: k_emit on planes of mixed runs and literals -- a match's bits come from the block's length table and two symbols are
appended at a time.  emit_mixed_cases.py says which part of the kernel each input is for.  Every case compresses into a
buffer pre-filled with 0xA5: the record bytes equal the CPU oracle's byte for byte, and the bytes behind the returned length
still hold the pattern."""
import numpy as np
import pytest

import emit_mixed_cases as mixed
import emit_whole_words_cases as cases
import util

pytestmark = pytest.mark.gpu

LANE_SPLIT_CHUNKS = 8     # mrcz_api.hip: a batch of nb >= 8 chunks runs as two lanes on two streams


@pytest.fixture(scope="module")
def codec():
    from datacompressionfloat_amd import MrcZipCodec
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield c
    c.close()


def _compress_prefilled(codec, words, bits=0):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
    out = torch.full((codec.records_bound(len(words)) + cases.SLACK,), cases.PATTERN, dtype=torch.uint8, device="cuda")
    rec, planes = codec.compress_device(dev, bits, 0, out=out)
    assert sum(planes) == rec.numel()
    return out.cpu().numpy(), rec.numel()


def _check(codec, oracle, plane, name, threads=0):
    words = mixed.words_of(plane)
    ref = oracle.compress(words, 0, threads=threads)
    got, olen = _compress_prefilled(codec, words)
    cases.check(got, olen, ref[17:], name)
    return ref


@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
def test_run_lengths(codec, oracle, shuffled):
    _check(codec, oracle, mixed.run_set(shuffled), f"runs shuffled={shuffled}")


@pytest.mark.parametrize("shift", mixed.SHIFTS)
def test_alignment(codec, oracle, shift):
    _check(codec, oracle, mixed.run_set(True, shift), f"runs shifted by {shift}")


def test_pairing(codec, oracle):
    plane = mixed.pairing_plane()
    mixed.check_pairing_plane(plane)
    _check(codec, oracle, plane, "pairing")


@pytest.mark.parametrize("second", sorted(mixed.BOUNDARY_TYPES))
def test_block_boundary(codec, oracle, second):
    plane = mixed.boundary_plane(second)
    ref = _check(codec, oracle, plane, f"boundary, second block {second}")
    mixed.check_boundary(plane, mixed.plane_stream(ref), second)


def test_long_codes(codec, oracle):
    plane = mixed.long_code_plane()
    ref = _check(codec, oracle, plane, "long codes")
    mixed.check_long_codes(plane, mixed.plane_stream(ref))


def test_two_lanes(oracle):
    """The shifted run set repeated over the smallest batch mrcz_api.hip cuts into two lanes (eight chunks): every chunk
    meets the runs at another offset, and both lanes' emits run the table and pair code on two streams."""
    from datacompressionfloat_amd import MrcZipCodec
    n = (LANE_SPLIT_CHUNKS - 1) * util.CHUNK + 1000
    unit = mixed.run_set(True, 17)
    plane = np.tile(unit, n // len(unit) + 1)[:n]
    big = MrcZipCodec(0, max_batch_chunks=LANE_SPLIT_CHUNKS)
    try:
        _check(big, oracle, plane, "two lanes", threads=16)
    finally:
        big.close()
