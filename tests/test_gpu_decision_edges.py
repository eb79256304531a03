"""GPU: inputs that sit exactly on the comparisons of k_stream_layout (decision_edge_cases.py says which, and asserts from the
oracle that each input sits there).  Every case: the container, byte for byte, in a buffer pre-filled with 0xA5; the block table
of every stream (mrcz_debug_blocks) against the oracle's; the probe's sizes; and the decode of the oracle's container.

Beyond the emulator twin: every length of family A, A0 once more as the ragged last chunk behind a full one, a full-size chunk
at the RAW threshold (D) and the shape of SURVEY App. C-1 (E).

A value that a kernel fails to write reads here as whatever the workspace held; only the emulator twin, whose fresh device
memory is zero, turns such a read into a failure on every run."""
import numpy as np
import pytest

import decision_edge_cases as cases
import emit_whole_words_cases as whole
import util

pytestmark = pytest.mark.gpu

MAX_BATCH = 4          # every input here is one batch: mrcz_debug_blocks shows the last batch of a call only


class GpuBackend(cases.Backend):
    def __init__(self, codec, lib):
        self.codec, self.lib, self.dev = codec, lib, None

    def _upload(self, words):
        import torch
        self.dev = torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32)).cuda()      # a copy: some inputs are read-only
        return self.dev

    def compress_prefilled(self, words):
        import torch
        dev = self._upload(words)
        out = torch.full((self.codec.records_bound(len(words)) + whole.SLACK,), whole.PATTERN, dtype=torch.uint8, device="cuda")
        rec, planes = self.codec.compress_device(dev, 0, 0, out=out)
        return out.cpu().numpy(), rec.numel(), [int(p) for p in planes]

    def blocks(self, stream):
        return cases.debug_blocks(self.lib, self.codec._ctx, stream)

    def probe(self, words):
        size, planes, _ = self.codec.probe_device(self.dev, 0)        # the words compress_prefilled uploaded
        return size, planes

    def decode(self, records, nwords):
        import torch
        rec = torch.zeros(len(records) + 8, dtype=torch.uint8, device="cuda")
        rec[:len(records)] = torch.from_numpy(np.frombuffer(records, np.uint8).copy()).cuda()
        out, consumed = self.codec.uncompress_device(rec[:len(records)], nwords)
        assert consumed == len(records)
        return out.cpu().numpy().view(np.uint32), self.codec.last_fallbacks()


@pytest.fixture(scope="module")
def be():
    from datacompressionfloat_amd import MrcZipCodec
    from datacompressionfloat_amd.codec import _LIB
    c = MrcZipCodec(0, max_batch_chunks=MAX_BATCH)
    yield GpuBackend(c, _LIB)
    c.close()


def _check(be, oracle, words, name):
    return cases.check_case(be, oracle, words, name, max_batch_chunks=MAX_BATCH)


@pytest.mark.parametrize("n", range(1, 81))
def test_raw_threshold_small_planes(be, oracle, n):
    z = _check(be, oracle, cases.a_case(oracle, n), f"A-{n}")
    cases.check_a_headers(oracle, n, z)


@pytest.mark.parametrize("n", cases.A0_N)
def test_raw_threshold_in_the_ragged_last_chunk(be, oracle, n):
    z = _check(be, oracle, cases.a_case(oracle, n, behind_full_chunk=True), f"A0-behind-a-chunk-{n}")
    cases.check_a_headers(oracle, n, z, chunk=1)


@pytest.mark.parametrize("k", sorted(cases.B_CASES))
def test_stored_tie(be, oracle, k):
    _check(be, oracle, cases.b_case(oracle, k), f"B-{k}")


@pytest.mark.parametrize("name", list(cases.C_CASES))
def test_static_dynamic_byte_tie(be, oracle, name):
    _check(be, oracle, cases.c_case(oracle, name), f"C-{name}")


@pytest.mark.parametrize("name", cases.g_names())
def test_window_slides(be, oracle, name):
    _check(be, oracle, cases.g_case(oracle, name), f"G-{name}")


@pytest.mark.parametrize("name", cases.f_names())
def test_block_boundary_by_symbols(be, oracle, name):
    _check(be, oracle, cases.f_case(oracle, name), f"F-{name}")


@pytest.mark.parametrize("m", list(cases.D_M))
def test_full_size_chunk_at_the_raw_threshold(be, oracle, m):
    cases.d_conditions()
    z = _check(be, oracle, cases.d_case(oracle, m), f"D-{m}")
    cases.d_check_header(oracle, m, z)


def test_incompressible_chunk_then_compressible_chunk(be, oracle):
    """The shape of SURVEY App. C-1: a full-size incompressible chunk, then a compressible one, in one file.  The reference
    binary itself diverges on this input (its encoder state carries over from the chunk that hit the output cap) and must not
    be consulted; this codec and the oracle code every chunk with fresh state, and the oracle is the expectation."""
    z = _check(be, oracle, cases.e_words(), "E")
    cases.e_check_headers(oracle, z)
