"""GPU: binned decode on the MI355X -- read_mrc_binned and `mrc_extract -N` equal a numpy fold of the full decode bit for bit; a
13-chunk volume binned through batches of four chunks equals one call per chunk and one batch; a device-generated,
device-compressed ~4 GiB volume at factor 4 equals the same fold done in float64 torch on the GPU over uncompress_device's output;
and the result agrees with avg_pool3d within float32 rounding (the meaning of the mean)."""
import os
import subprocess

import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")
CHK = util.CHUNK


def bin_expected(vol_u32, fx, fy, fz):           # vol (nz, ny, nx) of decoded words
    nz, ny, nx = vol_u32.shape; mz, my, mx = nz // fz, ny // fy, nx // fx
    v = vol_u32[:mz*fz, :my*fy, :mx*fx].view(np.float32).astype(np.float64)
    v = v.reshape(mz, fz, my, fy, mx, fx).transpose(0, 2, 4, 1, 3, 5).reshape(mz, my, mx, -1)
    s = v[..., 0].copy()
    for t in range(1, v.shape[-1]):
        s += v[..., t]
    return (s / v.shape[-1]).astype(np.float32)  # compare bits; NaN vs NaN by position only


def torch_fold(words, d0, nx, ny, nz, fx, fy, fz):
    """bin_expected in float64 torch on the GPU, over decoded words (int32 cuda tensor): the same order of additions"""
    import torch
    mz, my, mx = nz // fz, ny // fy, nx // fx
    vol = words[d0: d0 + nx * ny * nz].view(torch.float32).reshape(nz, ny, nx)[: mz * fz, : my * fy, : mx * fx]
    v = vol.reshape(mz, fz, my, fy, mx, fx)
    s = None
    for k in range(fz):
        for j in range(fy):
            for l in range(fx):
                t = v[:, k, :, j, :, l].to(torch.float64)
                s = t.clone() if s is None else s.add_(t)
    return (s / float(fx * fy * fz)).to(torch.float32)


def _same_bits(got, exp):
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    gn, en = np.isnan(got), np.isnan(exp)
    return got.shape == exp.shape and np.array_equal(gn, en) and np.array_equal(got.view(np.uint32)[~en], exp.view(np.uint32)[~en])


def _geom(d0, nx, ny, nz, fx, fy, fz):
    from datacompressionfloat_amd._lib import MrczBinGeom
    return MrczBinGeom(d0, nx, ny, nz, fx, fy, fz)


@pytest.fixture(scope="module")
def codec():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    assert torch.cuda.is_available()
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield c
    c.close()


NX, NY, NZ, NSYMBT = 1000, 700, 30, 96
D0 = 256 + NSYMBT // 4                   # 21000280 words: four chunks, boundaries inside sections 8, 17 and 26


def _mrc_volume():
    rng = np.random.default_rng(6)
    w = np.zeros(D0 + NX * NY * NZ, np.uint32)
    w[:256] = util.kat_words(256)
    w[0:4] = [NX, NY, NZ, 2]
    w[23] = NSYMBT
    w[D0:] = rng.normal(100.0, 20.0, NX * NY * NZ).astype(np.float32).view(np.uint32)
    special = np.array([0x80000000, 0x00000000, 0x00012300, 0x80045600, 0x7F800000, 0xFF800000, 0x7FC00000, 0x80000000], np.uint32)
    for z, y in ((0, 0), (8, 699), (17, 350), (29, 699)):
        a = D0 + (z * NY + y) * NX
        w[a: a + NX] = np.resize(special, NX)
    a = D0 + 12 * NX * NY
    w[a: a + 4 * NX] = 0x80000000                       # -0.0 rows: their bins stay -0.0
    return w


def test_read_mrc_binned_and_mrc_extract_equal_the_numpy_fold(codec, tmp_path):
    import torch
    w = _mrc_volume()
    z = codec.zip_bytes(w.tobytes(), 10)
    p = tmp_path / "vol.mrc.zip"
    p.write_bytes(z)
    vol = np.frombuffer(codec.unzip_bytes(z), np.uint32)[D0:].reshape(NZ, NY, NX)
    for factor in (1, 2, (3, 5, 7), (1, 1, NZ), (NX, NY, 1), np.int64(4)):
        f3 = (int(factor),) * 3 if np.ndim(factor) == 0 else factor
        got = codec.read_mrc_binned(p, factor)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (NZ // f3[2], NY // f3[1], NX // f3[0])
        assert _same_bits(got.cpu().numpy(), bin_expected(vol, *f3)), factor
    got = codec.read_mrc_binned(z, (2, 2, 1)).cpu().numpy()          # a container in memory
    assert _same_bits(got, bin_expected(vol, 2, 2, 1))
    assert (got[12, :2].view(np.uint32) == 0x80000000).all()
    from datacompressionfloat_amd import MrczError
    for bad in (0, (NX + 1, 1, 1), (1, 1, NZ + 1), (2, 2)):
        with pytest.raises(MrczError):
            codec.read_mrc_binned(p, bad)
    # the command line, on a container written by mrc_tar
    src, zc, back = tmp_path / "vol.mrc", tmp_path / "vol_cli.mrc.zip", tmp_path / "back.mrc"
    src.write_bytes(w.tobytes())
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(src), "-o", str(zc), "-b", "8", "-t", "zip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(zc), "-o", str(back), "-t", "unzip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    vol8 = np.fromfile(back, np.uint32)[D0:].reshape(NZ, NY, NX)
    for spec, f3 in (("4", (4, 4, 4)), ("3,5,7", (3, 5, 7))):
        out = tmp_path / f"bin{spec}.raw"
        r = subprocess.run([os.path.join(BIN, "mrc_extract"), "-i", str(zc), "-o", str(out), "-N", spec], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        exp = bin_expected(vol8, *f3)
        assert _same_bits(np.fromfile(out, np.float32).reshape(exp.shape), exp), spec


def _bin_chunks(g, nfl):
    import ctypes
    from datacompressionfloat_amd import codec as codec_mod
    c0, c1 = ctypes.c_uint64(), ctypes.c_uint64()
    assert codec_mod._LIB.mrcz_bin_chunks(ctypes.byref(g), nfl, CHK, ctypes.byref(c0), ctypes.byref(c1)) == 0
    return c0.value, c1.value


def _record_offsets(rec, nchunks):
    offs, off = [], 0
    for _ in range(nchunks):
        offs.append(off)
        off += 16 + int(sum(int(v) & 0x7fffffff for v in rec[off: off + 16].cpu().numpy().view("<u4")))
    return offs + [off]


def test_batches_of_four_equal_one_call_per_chunk():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    nx, ny, nz, d0 = 1024, 1024, 72, 256            # 13 chunks, the last one holding the volume's last 256 words
    n = d0 + nx * ny * nz
    big = MrcZipCodec(0, max_batch_chunks=13)
    small = MrcZipCodec(0, max_batch_chunks=4)
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    rec, _ = big.compress_device(words, 8, 0)
    rec = rec.clone()
    del words
    full, _ = big.uncompress_device(rec, n)
    offs = _record_offsets(rec, 13)
    for f in ((3, 5, 7), (4, 4, 4), (1, 1, 72)):
        g = _geom(d0, nx, ny, nz, *f)
        shape = (nz // f[2], ny // f[1], nx // f[0])
        c0, c1 = _bin_chunks(g, n)
        assert c0 == 0 and c1 == (13 if f[2] != 7 else 12)    # fz = 7: sections 70 and 71 are a remainder, chunk 12 unused
        acc = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
        assert small.uncompress_binned_device(rec, n, g, acc) == c1
        four = small.binned_finish_device(g, acc)
        acc = torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
        for c in range(13):
            piece = rec[offs[c]: offs[c + 1]].clone()
            assert small.uncompress_binned_device(piece, n, g, acc, first_chunk=c, nchunks=1) == (1 if c < c1 else 0)
        per_chunk = small.binned_finish_device(g, acc)
        acc.fill_(3.0)
        assert big.uncompress_binned_device(rec, n, g, acc) == c1
        one = big.binned_finish_device(g, acc)
        assert torch.equal(four.view(torch.int32), per_chunk.view(torch.int32)), f
        assert torch.equal(four.view(torch.int32), one.view(torch.int32)), f
        assert torch.equal(four.view(torch.int32), torch_fold(full, d0, nx, ny, nz, *f).view(torch.int32)), f
    big.close()
    small.close()


def test_a_4gib_volume_at_factor_4_equals_the_torch_fold_and_avg_pool3d():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    nx, ny, nz, d0 = 2048, 2048, 256, 256           # 4 GiB of voxels, 171 chunks
    n = d0 + nx * ny * nz
    c = MrcZipCodec(0, max_batch_chunks=16)
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    c.generate_kat_device(words, 0)
    rec, _ = c.compress_device(words, 8, 0)
    rec = rec.clone()
    del words
    torch.cuda.empty_cache()
    g = _geom(d0, nx, ny, nz, 4, 4, 4)
    acc = torch.empty((nz // 4, ny // 4, nx // 4), dtype=torch.float64, device="cuda")
    assert _bin_chunks(g, n) == (0, (n + CHK - 1) // CHK)
    assert c.uncompress_binned_device(rec, n, g, acc) == (n + CHK - 1) // CHK
    got = c.binned_finish_device(g, acc)
    full, _ = c.uncompress_device(rec, n)
    del rec
    torch.cuda.empty_cache()
    exp = torch_fold(full, d0, nx, ny, nz, 4, 4, 4)
    assert torch.equal(got.view(torch.int32), exp.view(torch.int32))
    vol = full[d0:].view(torch.float32).reshape(1, 1, nz, ny, nx)
    pool = torch.nn.functional.avg_pool3d(vol, 4)[0, 0]
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, pool, rtol=1e-5, atol=1e-6)
    c.close()
