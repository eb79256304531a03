"""CPU-only twin of test_gpu_huffman_edges.py: the product's HIP sources on the SIMT emulator, at blocks that sit on the edges
of the Huffman builder (huffman_edge_cases.py says which and asserts, from the oracle and huffman_ref.py alone, that each
input sits there).  Also here, because they need no codec: the statement of trees.c pinned against every header the oracle
writes for the catalogue, and the list of classes the catalogue has to reach.

Every family runs here, 41 of the 85 cases (SIM_CASES: N, B and F in full, of T, Z and L the cases next to a branch): a case
is about a second on the emulator whatever its size, half of it the decode, and the module 40 s (the GPU twin runs all 85
cases in under 3 s).

Mutations of mrcz_huffman.hip tried by hand on this file with all 85 cases (none committed), and the families that fail:
  run_codes, zero branch:  r < 3u -> r < 4u                    T Z N B L      (a rest of three zeros)
  run_codes, other branch: r < 3u -> r < 4u                    T Z N B L F
  R / 138u, R % 138u -> 137u                                   T Z N B L F
  h < 4u -> h < 5u                                             T Z N B L F
  rest / 6u -> rest / 7u                                       T Z N B F
  M[(k + k2) % 5] -> M[min(k + k2, 4)]                         none: the same function, `k + k2 < 5` stands in the same
                                                               condition (the % only keeps the unrolled index in range)
  bl_tree_build's repair: bits = 6 -> bits = 5                 B: depth-8, depth-9
  no recomputation of opt_len `if (repaired)`                  F: all four (18-len by not coming back from compress)
  heap_len >= 16 -> heap_len > 16                              every family
  KEY_INF fill loop one slot short (k < last)                  T: 2-eq, 2-inc, 15 / 16 / 17-inc, 143 / 144 / 145-inc (what the
                                                               slot holds instead is not fixed; one run ended in a crash)
  has_g = true                                                 T: 285-inc, 286-inc"""
import pytest

import huffman_edge_cases as cases
import probe_ref as pr
from test_sim_decision_edges import SimBackend


@pytest.fixture(scope="module")
def be(simlib):
    pr.bind(simlib.lib)
    return SimBackend(simlib)


def test_statement_reproduces_every_header_of_the_catalogue(oracle):
    """block_facts() re-encodes each dynamic header of the oracle's streams through huffman_ref.py and compares the bits, the
    code lengths and every block's opt_len / static_len: a wrong statement cannot pass"""
    dynamic = 0
    for family, name in cases.all_cases():
        dynamic += sum(b["btype"] == 2 for b in cases.block_facts(oracle, family, name))
    # every block but T's static ones (every "eq" and T_STATIC); the all-match plane has a dynamic block in front of its own
    assert dynamic == len(cases.all_cases()) - len(cases.T_N) - len(cases.T_STATIC) + 1


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_family_sits_on_its_edge(oracle, family):
    cases.conditions(oracle, family)


def test_catalogue_reaches_every_class(oracle):
    missing = cases.REQUIRED - cases.reached(oracle)
    assert not missing, sorted(missing, key=str)


@pytest.mark.parametrize("family,name", [c for c in cases.all_cases() if c[1] in cases.SIM_CASES[c[0]]], ids=lambda v: str(v))
def test_case(be, oracle, family, name):
    cases.check(be, oracle, family, name)
