"""GPU: the small kernels between the histograms and the emit pass of the compressor (compress_path_cases.py says which
kernel each input is for).  Every case is compressed into a buffer pre-filled with 0xA5 and compared with the CPU oracle
byte for byte; the probe, which runs the same sizing passes, must return the sizes the compressor returns."""
import numpy as np
import pytest

import compress_path_cases as cases
import emit_mixed_cases as mixed
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


def _compress_prefilled(codec, dev, nwords, bits):
    import torch
    out = torch.full((codec.records_bound(nwords) + whole.SLACK,), whole.PATTERN, dtype=torch.uint8, device="cuda")
    rec, planes = codec.compress_device(dev, bits, 0, out=out)
    return out.cpu().numpy(), rec.numel(), [int(p) for p in planes]


def _check(codec, oracle, words, bits, name, probe=True, threads=0):
    import torch
    z = oracle.compress(words, bits, threads=threads)
    dev = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
    got, olen, planes = _compress_prefilled(codec, dev, len(words), bits)
    whole.check(got, olen, z[17:], name)
    assert planes == pr.plane_sums(z, len(words)), name
    if probe:
        size, pplanes, _ = codec.probe_device(dev, bits)
        assert (size, pplanes) == (olen, planes), name
    return z


@pytest.mark.parametrize("n", sorted(cases.CONSTANT_N))
def test_constant_planes_over_many_pairs(codec, oracle, n):
    z = _check(codec, oracle, cases.constant_words(n), 0, f"constant-{n}")
    cases.check_constant(n, z)


def test_sparse_plane_with_many_match_lengths(codec, oracle):
    z = _check(codec, oracle, mixed.words_of(cases.sparse_plane()), 0, "sparse")
    cases.check_sparse(z)


def test_static_block_cut_by_a_segment_boundary(codec, oracle):
    plane, cut = cases.static_cut_plane()
    z = _check(codec, oracle, mixed.words_of(plane), 0, "static cut")
    cases.check_static_cut(plane, cut, z)


@pytest.mark.parametrize("name", cases.KEPT)
def test_kept_inputs(codec, oracle, name):
    words, bits = cases.kept(name)
    _check(codec, oracle, words, bits, name, probe=False)


def test_one_block_over_all_segments_of_a_chunk(codec, oracle):
    words, bits = cases.constant_chunk_plus()
    z = _check(codec, oracle, words, bits, "constant chunk + 1000", probe=False)
    for plane in range(4):
        blocks = cases.coded_blocks(mixed.plane_stream(z, plane, chunk=0))
        assert len(blocks) == 1 and blocks[0][0] == 2          # one block over the chunk's 192 segments
        assert len(cases.coded_blocks(mixed.plane_stream(z, plane, chunk=1))) == 1


def test_two_lanes_number_their_own_blocks(oracle):
    """The smallest batch that runs as two lanes, twice into the same pre-filled buffer.  Each lane's k_huffman derives the
    (stream, block) of its trees from its own streams' block counts."""
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    words, bits = cases.two_lane_words()
    ref = oracle.compress(words, bits, threads=16)
    for chunk in (1, 3, 5):     # plane 0, masked to zero, is one dynamic block over the chunk's 192 segments
        blocks = cases.coded_blocks(mixed.plane_stream(ref, 0, chunk=chunk))
        assert len(blocks) == 1 and blocks[0][0] == 2, (chunk, [b[:2] for b in blocks])
    big = MrcZipCodec(0, max_batch_chunks=cases.TWO_LANE_CHUNKS)
    try:
        dev = torch.from_numpy(words.view(np.int32)).cuda()
        out = torch.full((big.records_bound(len(words)) + whole.SLACK,), whole.PATTERN, dtype=torch.uint8, device="cuda")
        for turn in range(2):
            rec, planes = big.compress_device(dev, bits, 0, out=out)
            whole.check(out.cpu().numpy(), rec.numel(), ref[17:], f"two lanes turn {turn}")
            assert [int(p) for p in planes] == pr.plane_sums(ref, len(words))
    finally:
        big.close()
