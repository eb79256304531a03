"""GPU: top-planes decode on the MI355X.  The three-chunk volume of tests/test_sim_top.py in its three containers (written by the
CPU oracle) through MrcZipCodec.uncompress_top_device, ordinary and thinned records, every cut; every comparison is bit equality
with oracle.uncompress(container) & mask(keep).  bench.py's 1 GiB volume at -b 8 and -b 0 against uncompress_device & mask on the
device; mrc_extract -P 2 -H on a file in /dev/shm; unzip_top and read_mrc_top from a path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import top_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero
from top_ref import COMBOS

pytestmark = pytest.mark.gpu

CHK = util.CHUNK
EPS = f32_toward_zero(0.01)
BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lib():
    from datacompressionfloat_amd.codec import _LIB
    return _LIB


@pytest.fixture(scope="module")
def small(oracle):
    from test_sim_binned import _volume
    w = _volume()
    out = {"n": len(w)}
    for tag, z in (("b8", oracle.compress(w.tobytes(), 8)), ("b0", oracle.compress(w.tobytes(), 0)), ("eps", oracle.compress(abs_round(w, EPS).tobytes(), 0))):
        out[tag] = (z, np.frombuffer(oracle.uncompress(z), np.uint32))
    return out


def _dev(torch, codec, b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(codec.device)


def _bits(torch, t):
    """the elements of a float32 / bfloat16 cuda tensor as numpy uint32 / uint16"""
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint16)


def _top(torch, lib, codec, rec, nfl, keep, u16, thinned, first_chunk=0, nchunks=None, out=None):
    src = ref.thin(lib, rec, nfl, keep, first_chunk=first_chunk) if thinned else rec
    return codec.uncompress_top_device(_dev(torch, codec, src), nfl, keep, torch.bfloat16 if u16 else torch.float32, first_chunk=first_chunk,
                                       nchunks=nchunks, thinned=thinned, out=out)


def test_small_volume_every_combination_and_cut(torch, lib, small):
    from datacompressionfloat_amd import MrcZipCodec
    n = small["n"]
    codecs = {m: MrcZipCodec(0, max_batch_chunks=m) for m in (1, 2, 64)}
    for tag in ("b8", "b0", "eps"):
        z, full = small[tag]
        rec = z[17:]
        for keep, u16 in COMBOS:
            for thinned in (False, True):
                got = _top(torch, lib, codecs[2], rec, n, keep, u16, thinned)
                assert np.array_equal(_bits(torch, got), ref.expected(full, keep, u16)), (tag, keep, u16, thinned)
                assert codecs[2].last_fallbacks() == 0 and codecs[2].last_chain_fallbacks() == 0
    z, full = small["b8"]
    rec = z[17:]
    offs = ref.offsets(rec, n)
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            for m in (1, 64):
                assert np.array_equal(_bits(torch, _top(torch, lib, codecs[m], rec, n, keep, u16, thinned)), ref.expected(full, keep, u16))
            out = torch.empty(n, dtype=torch.bfloat16 if u16 else torch.float32, device=codecs[1].device)
            for c in (2, 1, 0):                                               # one call per chunk, in reverse order
                _top(torch, lib, codecs[1], rec[offs[c]: offs[c + 1]], n, keep, u16, thinned, first_chunk=c, nchunks=1, out=out[c * CHK:])
            assert np.array_equal(_bits(torch, out), ref.expected(full, keep, u16)), (keep, u16, thinned)
    # torch.bfloat16 is the upper half of the full decode's words
    fd, _ = codecs[2].uncompress_device(_dev(torch, codecs[2], rec), n)
    bf = _top(torch, lib, codecs[2], rec, n, 2, True, False)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf.view(torch.int16), (fd.view(torch.int32) >> 16).to(torch.int16))
    assert torch.equal(bf.float().view(torch.int32), fd.view(torch.int32) & -65536)
    for c in codecs.values():
        c.close()


@pytest.mark.parametrize("n", [1, 3, 5, 7, 9, 257, 4099, 16386, CHK + 1, CHK + 3, CHK + 5])
def test_ragged_last_chunks(torch, lib, oracle, n):
    from datacompressionfloat_amd import MrcZipCodec
    codec = MrcZipCodec(0, max_batch_chunks=2)
    w = util.gauss_words(n, seed=n, header=False)
    z = oracle.compress(w.tobytes(), 10)
    full = np.frombuffer(oracle.uncompress(z), np.uint32)
    for keep, u16 in COMBOS:
        for thinned in (False, True):
            got = _top(torch, lib, codec, z[17:], n, keep, u16, thinned)
            assert np.array_equal(_bits(torch, got), ref.expected(full, keep, u16)), (keep, u16, thinned)
    codec.close()


def test_dropped_planes_are_never_read_and_refusals(torch, lib, small):
    from datacompressionfloat_amd import MrcZipCodec, MrczError
    codec = MrcZipCodec(0, max_batch_chunks=2)
    n = small["n"]
    for tag, keep, u16 in (("b0", 2, True), ("b8", 2, False), ("b8", 3, False)):
        z, full = small[tag]
        bad = ref.poison(z[17:], n, keep)
        assert bad != z[17:]
        got = _top(torch, lib, codec, bad, n, keep, u16, False)
        assert np.array_equal(_bits(torch, got), ref.expected(full, keep, u16)), (tag, keep)
        assert codec.last_fallbacks() == 0 and codec.last_chain_fallbacks() == 0
    z, full = small["b8"]
    rec = z[17:]
    with pytest.raises(MrczError):
        _top(torch, lib, codec, rec[: len(rec) - 7], n, 2, True, False)       # the records end early: an error status
    with pytest.raises(MrczError):
        codec.uncompress_top_device(_dev(torch, codec, rec), n, 3, torch.bfloat16)
    with pytest.raises(MrczError):
        codec.uncompress_top_device(_dev(torch, codec, rec), n, 4, torch.float32)
    with pytest.raises(MrczError):
        codec.uncompress_top_device(_dev(torch, codec, rec), n, 2, torch.float32, first_chunk=1, nchunks=3)
    got = _top(torch, lib, codec, rec, n, 2, True, True)                      # the context still works
    assert np.array_equal(_bits(torch, got), ref.expected(full, 2, True))
    codec.close()


def test_unzip_top_and_read_mrc_top_from_a_path(torch, small, tmp_path):
    from datacompressionfloat_amd import MrcZipCodec
    from test_sim_binned import D0, NX, NY, NZ
    codec = MrcZipCodec(0, max_batch_chunks=2)
    z, full = small["b8"]
    p = tmp_path / "vol.mrc.zip"
    p.write_bytes(z)
    for keep, dtype in ((2, torch.bfloat16), (2, torch.float32), (3, torch.float32)):
        u16 = dtype == torch.bfloat16
        flat = codec.unzip_top(str(p), keep, dtype)
        assert flat.dtype == dtype and np.array_equal(_bits(torch, flat), ref.expected(full, keep, u16))
        assert np.array_equal(_bits(torch, codec.unzip_top(z, keep, dtype)), ref.expected(full, keep, u16))
        vol = codec.read_mrc_top(str(p), keep, dtype)
        assert tuple(vol.shape) == (NZ, NY, NX) and vol.dtype == dtype
        assert np.array_equal(_bits(torch, vol.contiguous()).reshape(NZ, NY, NX), ref.expected(full[D0: D0 + NX * NY * NZ], keep, u16).reshape(NZ, NY, NX))
    # the dropped payloads replaced by 0xFF on disk: nothing of them is read
    p.write_bytes(z[:17] + ref.poison(z[17:], small["n"], 2))
    assert np.array_equal(_bits(torch, codec.unzip_top(str(p))), ref.expected(full, 2, True))
    codec.close()


def test_one_gib_volume_against_the_full_decode_on_the_device(torch):
    sys.path.insert(0, util.ROOT)
    import bench
    from datacompressionfloat_amd import MrcZipCodec
    nfl = (1 << 30) // 4
    w = bench.make_volume(nfl, 1234, True)
    c64, c8 = MrcZipCodec(0, max_batch_chunks=64), MrcZipCodec(0, max_batch_chunks=8)
    dw = torch.from_numpy(w.view(np.int32)).to(c64.device)
    for bits in (8, 0):
        rec, _ = c64.compress_device(dw, bits)
        full, _ = c64.uncompress_device(rec, nfl)
        full = full.view(torch.int32)
        bf = c64.uncompress_top_device(rec, nfl, 2, torch.bfloat16)
        assert torch.equal(bf.view(torch.int16), (full >> 16).to(torch.int16)), bits
        assert c64.last_fallbacks() == 0
        del bf
        k3 = c8.uncompress_top_device(rec, nfl, 3, torch.float32)              # batches of 8 against one of 64
        assert torch.equal(k3.view(torch.int32), full & -256), bits
        del k3, full, rec
    c64.close()
    c8.close()


def test_mrc_extract_P2_H_on_a_file_in_shm(oracle):
    d = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    import tempfile
    with tempfile.TemporaryDirectory(dir=d) as t:
        n = 2 * CHK + 70001
        w = util.gauss_words(n, seed=91)
        z = oracle.compress(w.tobytes(), 8)
        full = np.frombuffer(oracle.uncompress(z), np.uint32)
        zp, op = os.path.join(t, "a.zip"), os.path.join(t, "a.raw")
        run = lambda args: subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        open(zp, "wb").write(z)
        r = run([os.path.join(BIN, "mrc_extract"), "-i", zp, "-o", op, "-P", "2", "-H"])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(op, np.uint16), ref.expected(full, 2, True))
        r = run([os.path.join(BIN, "mrc_extract"), "-i", zp, "-o", op, "-P", "3"])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(op, np.uint32), ref.expected(full, 3))
        open(zp, "wb").write(z[:17] + ref.poison(z[17:], n, 2))             # dropped payloads 0xFF on disk
        r = run([os.path.join(BIN, "mrc_extract"), "-i", zp, "-o", op, "-P", "2", "-H"])
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(op, np.uint16), ref.expected(full, 2, True))
        r = run([os.path.join(BIN, "mrc_extract"), "-i", zp, "-o", op, "-P", "3", "-H"])
        assert r.returncode == 255, (r.returncode, r.stderr)
