"""GPU: blocks that sit on the edges of the Huffman builder, k_huffman and k_huffman_hdr (huffman_edge_cases.py says which and
asserts, from the oracle and huffman_ref.py alone, that each input sits there; the emulator twin test_sim_huffman_edges.py
runs those assertions).  Every case of every family: the container, byte for byte, in a buffer pre-filled with 0xA5; the block
table of every stream (mrcz_debug_blocks) against the oracle's, which is what checks k_huffman's opt_len and static_len on the
blocks that are not emitted dynamic; the probe's sizes; and the decode of the oracle's container with no fall-back
(k_validate_wave parses the same headers).

A case is a compress call of its own: a call holds whole chunks, and a second case in it would have to stand behind a
full-size one."""
import pytest

import huffman_edge_cases as cases
from test_gpu_decision_edges import GpuBackend

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from datacompressionfloat_amd import MrcZipCodec
    from datacompressionfloat_amd.codec import _LIB
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield GpuBackend(c, _LIB)
    c.close()


@pytest.mark.parametrize("family,name", cases.all_cases(), ids=lambda v: str(v))
def test_case(be, oracle, family, name):
    cases.check(be, oracle, family, name)
