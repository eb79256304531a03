"""CPU-only twin of test_gpu_decision_edges.py: the product's HIP sources on the SIMT emulator, at inputs that sit exactly on
the comparisons of k_stream_layout (decision_edge_cases.py says which, and asserts from the oracle that each input sits there).
Every case: the container, byte for byte, in a buffer pre-filled with 0xA5; the block table of every stream (mrcz_debug_blocks)
against the oracle's; the probe's sizes; and the decode of the oracle's container.

Not here: the families D (a full-size chunk at the RAW threshold) and E and A0 behind a full chunk, which are
minutes on the emulator, and most of A's 80 lengths; the GPU file has them.

Every case runs in a fresh context of an emulator build whose fresh device memory is zero (see zeroed_lib).  That is what
made the one disagreement these inputs found fail on every run, not with the order of the tests: a stream of 65274 + 32768 j
bytes makes its last window slide at position n itself, k_histogram has no tile for that position and wrote no slide
position, and k_stream_layout's search over the slide positions read whatever the workspace held there for the stream's full
blocks (G-65274, G-98042 in the block table; F-65534-stored-full in the container).  k_stream_layout now takes n for it.

Mutations of k_stream_layout tried by hand on this file (one token each, none committed), and the cases that fail:
  n > len + 4u                        ->  >=                              A: 13, 49, 51, 52
  stored_len + 4u <= opt_lenb         ->  <                               B: all three
  static_lenb == opt_lenb             ->  m.static_len <= m.opt_len       C: all eight
  start >= 32768u * (k - 1u)          ->  >                               B: all three, G: all (a stream's first block starts
                                                                          at 0 and is then never stored)
  the same, only where k > 1                                              G: start-on-slide
  s_q[mid] < end                      ->  <=                              F: 65534-stored-full
  full = ... || nsym == nblk * 32767  ->  full = (b + 1 < si.nblk)        F: 65534-stored-full"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import decision_edge_cases as cases
import emit_whole_words_cases as whole
import probe_ref as pr
import util


class SimBackend(cases.Backend):
    def __init__(self, sim):
        self.sim = sim

    def compress_prefilled(self, words):
        sim, n = self.sim, len(words)
        din = util.aligned_empty(4 * n).view(np.uint32)
        din[:] = words
        cap = int(sim.lib.mrcz_records_bound(n)) + whole.SLACK
        dout = util.aligned_empty(cap)
        dout[:] = whole.PATTERN
        olen = ctypes.c_uint64()
        planes = (ctypes.c_uint64 * 4)()
        rc = sim.lib.mrcz_compress_chunks(sim.ctx, din.ctypes.data, n, 0, 0, dout.ctypes.data, cap, ctypes.byref(olen), planes)
        assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
        return dout, int(olen.value), list(planes)

    def blocks(self, stream):
        return cases.debug_blocks(self.sim.lib, self.sim.ctx, stream)

    def probe(self, words):
        sim = self.sim
        din = util.aligned_empty(4 * len(words)).view(np.uint32)
        din[:] = words
        olen = ctypes.c_uint64(12345)
        planes = (ctypes.c_uint64 * 4)()
        rc = sim.lib.mrcz_probe_chunks(sim.ctx, din.ctypes.data, len(words), 0, pr.MASK, 0, 0.0, -1.0, -1.0, None, ctypes.byref(olen), planes)
        assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
        return int(olen.value), list(planes)

    def decode(self, records, nwords):
        out = self.sim.uncompress_records(records, nwords)
        return out, self.sim.fallbacks


@pytest.fixture(scope="module")
def zeroed_lib(tmp_path_factory):
    """The emulator build with -DSIM_POISON_DEVICE=0: fresh device memory is zero, not whatever malloc returns.  A slide
    position that no kernel wrote then reads as 0, in front of every block's end, on every run (with stale or arbitrary
    values the same read is right by luck most of the time, and the test passes or fails with the order of the tests)."""
    so = tmp_path_factory.mktemp("sim_zeroed") / "libmrcz_sim_zeroed.so"
    csrc = os.path.join(util.ROOT, "datacompressionfloat_amd", "csrc")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fPIC", "-I" + util.SIM_DIR, "-I" + csrc, "-Wno-attributes",
                           "-Wno-unknown-pragmas", "-DSIM_POISON_DEVICE=0", "-shared", "-o", str(so),
                           os.path.join(csrc, "mrcz_api.hip"), os.path.join(util.SIM_DIR, "sim_runtime.cpp")])
    lib = ctypes.CDLL(str(so))
    pr.bind(lib)
    return lib


@pytest.fixture
def be(zeroed_lib):
    """a fresh context for every case: nothing an earlier case left in the workspace can stand in for a value this one
    fails to write"""
    sim = util.SimCodec(zeroed_lib)
    yield SimBackend(sim)
    zeroed_lib.mrcz_destroy(sim.ctx)


@pytest.mark.parametrize("family", ["a", "b", "c", "g", "f"])
def test_family_sits_on_its_edge(oracle, family):
    getattr(cases, family + "_conditions")(oracle)


@pytest.mark.parametrize("n", cases.A_SIM)
def test_raw_threshold_small_planes(be, oracle, n):
    z = cases.check_case(be, oracle, cases.a_case(oracle, n), f"A-{n}")
    cases.check_a_headers(oracle, n, z)


@pytest.mark.parametrize("k", sorted(cases.B_CASES))
def test_stored_tie(be, oracle, k):
    cases.check_case(be, oracle, cases.b_case(oracle, k), f"B-{k}")


@pytest.mark.parametrize("name", list(cases.C_CASES))
def test_static_dynamic_byte_tie(be, oracle, name):
    cases.check_case(be, oracle, cases.c_case(oracle, name), f"C-{name}")


@pytest.mark.parametrize("name", cases.g_names())
def test_window_slides(be, oracle, name):
    cases.check_case(be, oracle, cases.g_case(oracle, name), f"G-{name}")


@pytest.mark.parametrize("name", cases.f_names())
def test_block_boundary_by_symbols(be, oracle, name):
    cases.check_case(be, oracle, cases.f_case(oracle, name), f"F-{name}")
