"""GPU: range decode on the MI355X -- windows of the 1 GiB App. D volume equal the same words of the whole-file decode, the
reference-written fixtures (deflate, LZ4, "-s int") decode in ranges, read_mrc_slab equals numpy slicing of the full decode,
and `mrc_extract -z` equals the slice of `mrc_tar -t unzip`."""
import os
import subprocess

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")
CHK = util.CHUNK


@pytest.fixture(scope="module")
def codec():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    assert torch.cuda.is_available()
    c = MrcZipCodec(0, max_batch_chunks=8)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [8, 12])
def test_windows_of_the_one_gib_volume(bits):
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    n = 268435456
    big = MrcZipCodec(0, max_batch_chunks=43)
    small = MrcZipCodec(0, max_batch_chunks=4)     # ranges of more than four chunks go through several batches
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    rec, _ = big.compress_device(words, bits, 0)
    del words
    full, consumed = big.uncompress_device(rec, n)
    assert consumed == rec.numel()
    windows = [(0, 256), (3, 300), (255, 4099), (1, 2), (CHK - 5, CHK + 7), (17 * CHK + 1, 17 * CHK + 1 + 2 * CHK + 3),
               (20 * CHK + 4096 * 7 + 2, 20 * CHK + 4096 * 9 + 1), (5 * CHK, 15 * CHK + 3), (n - 1, n), (n - 12345, n),
               (41 * CHK - 1, n), (0, n)]
    for w0, w1 in windows:
        for c in (big, small):
            got, _ = c.uncompress_range_device(rec, n, w0, w1)
            assert torch.equal(got, full[w0:w1]), (bits, w0, w1, c is small)
    # records that start at the window's chunk
    offs, off = [], 0
    hdr = rec[:0]
    for _ in range(22):
        offs.append(off)
        hdr = rec[off: off + 16].cpu().numpy().view(np.uint32)
        off += 16 + int(sum(int(x) & 0x7fffffff for x in hdr))
    got, cons = small.uncompress_range_device(rec[offs[21]:], n, 21 * CHK + 9, 21 * CHK + 70001, first_chunk=21)
    assert torch.equal(got, full[21 * CHK + 9: 21 * CHK + 70001]) and cons == off - offs[21]
    big.close()
    small.close()


def test_reference_fixtures_decode_in_ranges(codec):
    from golden.make_golden import int_cases, lz4_cases, small_cases
    cases = [(name, "float") for name in small_cases()] + [(name, "int") for name in int_cases()] + [(name, "float") for name in lz4_cases()]
    for name, mode in cases:
        z = open(os.path.join(util.GOLDEN, name + ".zip"), "rb").read()
        full = codec.unzip_bytes(z, mode=mode)
        n = len(full) // 4
        for w0, w1 in {(0, n), (1, min(n, 300)), (n - 3, n), (min(255, n - 1), min(257, n)), (n // 3, n // 2 + 1)}:
            if w0 >= w1:
                continue
            assert codec.unzip_range(z, w0, w1, mode=mode) == full[4 * w0: 4 * w1], (name, w0, w1)
    # the context decodes deflate containers again after LZ4 ones
    z = open(os.path.join(util.GOLDEN, "gauss20000_b12.zip"), "rb").read()
    assert codec.unzip_range(z, 10, 20) == codec.unzip_bytes(z)[40:80]


NX, NY, NZ, NSYMBT = 1000, 700, 30, 96


def _mrc_volume():
    rng = np.random.default_rng(5)
    w = np.zeros(256 + NSYMBT // 4 + NX * NY * NZ, np.uint32)
    w[:256] = util.kat_words(256)
    w[0:4] = [NX, NY, NZ, 2]
    w[23] = NSYMBT
    w[256 + NSYMBT // 4:] = rng.normal(100.0, 20.0, NX * NY * NZ).astype(np.float32).view(np.uint32)
    return w


def test_read_mrc_slab_equals_numpy_slicing(codec, tmp_path):
    import torch
    w = _mrc_volume()
    z = codec.zip_bytes(w.tobytes(), 10)
    p = tmp_path / "vol.mrc.zip"
    p.write_bytes(z)
    full = np.frombuffer(codec.unzip_bytes(z), np.uint32)
    vol = full[256 + NSYMBT // 4:].view(np.float32).reshape(NZ, NY, NX)
    for z0, z1 in ((0, 1), (8, 10), (12, 21), (29, 30), (0, NZ)):
        slab = codec.read_mrc_slab(p, z0, z1)
        assert slab.is_cuda and slab.dtype == torch.float32 and tuple(slab.shape) == (z1 - z0, NY, NX)
        assert np.array_equal(slab.cpu().numpy().view(np.uint32), vol[z0:z1].view(np.uint32)), (z0, z1)
    # only the covering records are read: a file cut after chunk 0 still gives the sections inside chunk 0
    offs_end = 17 + 16 + sum(int(x) & 0x7fffffff for x in np.frombuffer(z[17:33], "<u4"))
    cut = tmp_path / "cut.mrc.zip"
    cut.write_bytes(z[:offs_end])
    assert np.array_equal(codec.read_mrc_slab(cut, 2, 5).cpu().numpy().view(np.uint32), vol[2:5].view(np.uint32))
    from datacompressionfloat_amd import MrczError
    with pytest.raises(MrczError):
        codec.read_mrc_slab(cut, 20, 21)
    with pytest.raises(MrczError):
        codec.read_mrc_slab(p, 5, NZ + 1)


def test_mrc_extract_sections_equal_the_mrc_tar_slice(codec, tmp_path):
    w = _mrc_volume()
    src, z, back = tmp_path / "vol.mrc", tmp_path / "vol.mrc.zip", tmp_path / "back.mrc"
    src.write_bytes(w.tobytes())
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(z), "-o", str(back), "-t", "unzip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    full = np.fromfile(back, np.uint32)
    d0, sec = 256 + NSYMBT // 4, NX * NY
    for z0, z1 in ((0, 1), (8, 10), (29, 30)):
        out = tmp_path / f"s{z0}.raw"
        r = subprocess.run([os.path.join(BIN, "mrc_extract"), "-i", str(z), "-o", str(out), "-z", f"{z0}:{z1}"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(out, np.uint32), full[d0 + z0 * sec: d0 + z1 * sec]), (z0, z1)
    out = tmp_path / "w.raw"
    r = subprocess.run([os.path.join(BIN, "mrc_extract"), "-i", str(z), "-o", str(out), "-w", f"{CHK - 3}:9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(np.fromfile(out, np.uint32), full[CHK - 3: CHK + 6])
