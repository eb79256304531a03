"""GPU: the compressor writes whole output words and clears only the boundary words, so it must not depend on what the
output buffer held before.  Every case compresses into a buffer pre-filled with 0xA5 (emit_whole_words_cases.py says why
and which boundary each input is for): the record bytes equal the CPU oracle's byte for byte, and the bytes behind the
returned length still hold the pattern.

The staging buffer's halving path (`cap` in k_emit): the "long_codes_b0" input reaches it -- the emulator twin and this
file both read the library's count of parts cut in two (mrcz_debug_emit_splits) after that case."""
import numpy as np
import pytest

import emit_whole_words_cases as cases
import util

pytestmark = pytest.mark.gpu

LANE_SPLIT_CHUNKS = 8     # mrcz_api.hip: a batch of nb >= 8 chunks runs as two lanes on two streams (contexts of >= 8 chunks)


@pytest.fixture(scope="module")
def codec():
    from datacompressionfloat_amd import MrcZipCodec
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield c
    c.close()


def _compress_prefilled(codec, words, bits):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
    out = torch.full((codec.records_bound(len(words)) + cases.SLACK,), cases.PATTERN, dtype=torch.uint8, device="cuda")
    rec, planes = codec.compress_device(dev, bits, 0, out=out)
    assert sum(planes) == rec.numel()
    return out.cpu().numpy(), rec.numel()


@pytest.mark.parametrize("name", sorted(cases.SMALL))
def test_prefilled_output_equals_the_oracle(codec, oracle, name):
    from datacompressionfloat_amd import codec as codec_module
    words, bits = cases.SMALL[name]()
    got, olen = _compress_prefilled(codec, words, bits)
    cases.check(got, olen, oracle.compress(words, bits)[17:], name)
    if name == "long_codes_b0":
        assert int(codec_module._LIB.mrcz_debug_emit_splits(codec._ctx)) > 0      # the halving path was taken


def test_chunk_boundary_shares_dwords(codec, oracle):
    words, bits = cases.CHUNK_PLUS()
    got, olen = _compress_prefilled(codec, words, bits)
    cases.check(got, olen, oracle.compress(words, bits)[17:], "chunk_plus_1000_b8")


def test_two_lanes_meet_in_one_dword(oracle):
    """The smallest batch mrcz_api.hip cuts into two lanes: the second lane's records start where the first lane's end (not
    on a dword boundary), and the first lane is emitted on one stream while the second is laid out on another.  Twice into
    the same pre-filled buffer: the second call meets the first call's records, not the pattern."""
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    n = (LANE_SPLIT_CHUNKS - 1) * util.CHUNK + 1000
    words = util.gauss_words(n, seed=1234)
    ref = oracle.compress(words, 8, threads=16)[17:]
    big = MrcZipCodec(0, max_batch_chunks=LANE_SPLIT_CHUNKS)
    try:
        dev = torch.from_numpy(words.view(np.int32)).cuda()
        out = torch.full((big.records_bound(n) + cases.SLACK,), cases.PATTERN, dtype=torch.uint8, device="cuda")
        for turn in range(2):
            rec, planes = big.compress_device(dev, 8, 0, out=out)
            assert sum(planes) == rec.numel()
            cases.check(out.cpu().numpy(), rec.numel(), ref, f"two_lanes turn {turn}")
    finally:
        big.close()
