"""CPU-only: the probe (mrcz_probe_chunks, k_probe_fold, k_probe_sizes) on the SIMT emulator build of the product sources.  The size
it returns must be the length of the CPU oracle's container of the same setting minus the 17-byte file header, the plane sums those
of the oracle container's chunk headers, and every chunk record the numpy fold of tests/compare_ref.py over the original and what
the container decodes to (tests/probe_ref.py): counts, extremes and indices exactly, the sums within compare_ref.assert_matches'
bound.  No point and no chunk is left out of any comparison."""
import ctypes

import numpy as np
import pytest

import compare_ref as ref
import probe_ref as pr
import util
from abs_error_ref import f32_toward_zero
from test_sim_binned import N, _volume

CHK = util.CHUNK
EINVAL = -1
EPS = f32_toward_zero(0.01)
GARBAGE = 0xA5
RSZ = ctypes.sizeof(ref.Compare)


@pytest.fixture(scope="module")
def sim():
    s = util.load_sim()
    pr.bind(s.lib)
    return s


@pytest.fixture(scope="module")
def small():
    return pr.small_volume()


@pytest.fixture(scope="module")
def three(oracle):
    w = _volume()
    return w, pr.expectation(oracle, w, ("bits", 8), 1e-4, 2.0 ** -17)


def new_acc(nchunks):
    a = util.aligned_empty(RSZ * max(nchunks, 1))
    a[:] = GARBAGE                                  # d_acc needs no zeroing
    return a


def device(words):
    d = util.aligned_empty(4 * max(len(words), 4)).view(np.uint32)
    d[: len(words)] = words
    return d


def probe(lib, ctx, words, setting, first_chunk=0, acc=None, eps_abs=-1.0, eps_rel=-1.0, want_planes=True):
    """one mrcz_probe_chunks over `words` = the file's words from chunk first_chunk on: (rc, record bytes, plane_bytes)"""
    d = device(words)
    x, bits, eps = pr.abi_args(setting)
    olen = ctypes.c_uint64(12345)
    planes = (ctypes.c_uint64 * 4)()
    rc = lib.mrcz_probe_chunks(ctx, d.ctypes.data, len(words), first_chunk, x, bits, eps, eps_abs, eps_rel,
                               None if acc is None else acc.ctypes.data, ctypes.byref(olen), planes if want_planes else None)
    return rc, olen.value, list(planes)


@pytest.mark.parametrize("setting", [("bits", 0), ("bits", 8), ("bits", 12), ("bits", 23), ("bits", 32), ("abs", EPS), ("int",)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_short_chunk_size_planes_and_record(sim, oracle, small, setting):
    want = pr.expectation(oracle, small, setting, 1e-3, 2.0 ** -10)
    acc = new_acc(1)
    rc, size, planes = probe(sim.lib, sim.ctx, small, setting, acc=acc, eps_abs=1e-3, eps_rel=2.0 ** -10)
    assert rc == 0, sim.lib.mrcz_last_error(sim.ctx)
    pr.assert_probe(size, planes, pr.records(acc.tobytes(), 1), want, setting)
    t = ref.Compare()
    assert sim.lib.mrcz_compare_finish(sim.ctx, acc.ctypes.data, 0, 1, ctypes.byref(t)) == 0
    ref.assert_matches(ref.as_dict(t), want["total"], (setting, "total"))
    tot = want["total"]
    assert tot["n"] == pr.N_SMALL - 256 and tot["n_header_diff"] == 0
    if setting in (("bits", 8), ("bits", 12), ("bits", 23), ("bits", 32)):
        assert tot["n_special_diff"] > 0 and tot["first_over"] != ref.NONE   # NaNs that the mask turns into Inf
    if setting in (("bits", 23), ("bits", 32), ("int",)):
        assert tot["n_over_rel"] > 0 and tot["n_over_abs"] > 0              # both checks are on
    if setting == ("bits", 0):
        assert tot["n_diff"] == 0 and tot["max_err"] == 0


def test_cuts_and_batches_do_not_change_bits_or_sizes(sim, three):
    w, want = three
    kw = dict(eps_abs=1e-4, eps_rel=2.0 ** -17)
    acc = new_acc(3)
    rc, size, planes = probe(sim.lib, sim.ctx, w, ("bits", 8), acc=acc, **kw)        # the module's context: batches of two chunks
    assert rc == 0
    pr.assert_probe(size, planes, pr.records(acc.tobytes(), 3), want, "batches of 2")
    base = acc.tobytes()
    for mb in (1, 3):
        c = util.SimCodec(sim.lib, max_batch_chunks=mb)
        a = new_acc(3)
        a[:] = 0x3C
        assert probe(sim.lib, c.ctx, w, ("bits", 8), acc=a, **kw) == (0, size, planes), mb
        assert a.tobytes() == base, mb
        sim.lib.mrcz_destroy(c.ctx)
    # one call per chunk with its own first_chunk, in reverse order
    a = new_acc(3)
    sizes, psum = [], [0, 0, 0, 0]
    for c in (2, 1, 0):
        rc, s, p = probe(sim.lib, sim.ctx, w[c * CHK: (c + 1) * CHK], ("bits", 8), first_chunk=c, acc=a, **kw)
        assert rc == 0
        sizes.append(s)
        psum = [x + y for x, y in zip(psum, p)]
    offs = want["offsets"]
    assert sizes == [offs[c + 1] - offs[c] for c in (2, 1, 0)] and psum == planes
    assert a.tobytes() == base
    # the words from chunk 1 on: the oracle container's records from chunk 1 on (the header words are masked there)
    a = new_acc(3)
    rc, s, p = probe(sim.lib, sim.ctx, w[CHK:], ("bits", 8), first_chunk=1, acc=a, **kw)
    assert rc == 0 and s == offs[3] - offs[1] and p == pr.plane_sums(want["z"], N, first_chunk=1)
    assert a.tobytes()[:RSZ] == bytes([GARBAGE]) * RSZ and a.tobytes()[RSZ:] == base[RSZ:]      # chunk 0's record is untouched


def test_rejected_arguments_nothing_to_do_and_sizes_only(sim, oracle, small):
    lib, ctx = sim.lib, sim.ctx
    d = device(small)
    acc = new_acc(1)
    clean = acc.tobytes()
    olen = ctypes.c_uint64(7)
    call = lambda ctx_=ctx, din=d.ctypes.data, n=pr.N_SMALL, x=pr.MASK, bits=8, eps=0.0, a=acc.ctypes.data, ol=ctypes.byref(olen): \
        lib.mrcz_probe_chunks(ctx_, din, n, 0, x, bits, eps, -1.0, -1.0, a, ol, None)
    assert call(x=3) == EINVAL and call(x=-1) == EINVAL                       # unknown transform
    assert call(bits=33) == EINVAL and call(bits=-1) == EINVAL
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert call(x=pr.ABS, bits=0, eps=eps) == EINVAL, eps
    assert call(din=None) == EINVAL
    assert call(din=d.ctypes.data + 4, n=1000) == EINVAL                      # misaligned
    assert call(ol=None) == EINVAL
    assert call(ctx_=None) == EINVAL
    assert acc.tobytes() == clean
    olen.value = 7
    assert call(n=0) == 0 and olen.value == 0                                 # nothing to do ...
    assert call(n=0, din=None) == 0 and olen.value == 0
    assert acc.tobytes() == clean                                             # ... and nothing touched
    # d_acc = NULL: sizes only
    want = pr.expectation(oracle, small, ("bits", 8))
    rc, size, planes = probe(lib, ctx, small, ("bits", 8))
    assert (rc, size, planes) == (0, want["record_bytes"], want["plane_bytes"])
    rc, size, _ = probe(lib, ctx, small, ("bits", 8), want_planes=False)
    assert (rc, size) == (0, want["record_bytes"])


def test_compress_after_a_probe_on_the_same_context(sim, oracle, small):
    # the probe leaves the workspace usable: a compress call straight after still writes the oracle's container
    for probed, bits in ((("bits", 12), 8), (("int",), 0), (("abs", EPS), 8)):
        assert probe(sim.lib, sim.ctx, small, probed, acc=new_acc(1))[0] == 0
        assert sim.compress_records(small, bits) == oracle.compress(small.tobytes(), bits)[17:], (probed, bits)
