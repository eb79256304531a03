"""GPU: box decode on the MI355X -- read_mrc_boxes and `mrc_extract -B` equal numpy slicing of the full decode; 2000 random
32^3 boxes of a 13-chunk volume, decoded through batches of four chunks, equal a torch gather from uncompress_device; a box
whose rows skip a whole chunk never decodes it (its payload is garbage); the reference's LZ4 fixtures decode as flat volumes."""
import io
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


def _geom(d0, nx, ny, nz, bx, by, bz, fill_bits=0):
    from datacompressionfloat_amd._lib import MrczBoxGeom
    return MrczBoxGeom(d0, nx, ny, nz, bx, by, bz, fill_bits)


def _expect_np(vol, origins, size, fill_bits):
    """numpy: pad the (nz, ny, nx) volume with the fill word by a box on every side, then slice"""
    bx, by, bz = size
    nz, ny, nx = vol.shape
    pad = np.pad(vol, ((bz, bz), (by, by), (bx, bx)), constant_values=np.uint32(fill_bits))
    out = np.full((len(origins), bz, by, bx), np.uint32(fill_bits), np.uint32)
    for i, (x0, y0, z0) in enumerate(np.asarray(origins, np.int64)):
        if -bx <= x0 <= nx and -by <= y0 <= ny and -bz <= z0 <= nz:
            out[i] = pad[z0 + bz: z0 + 2 * bz, y0 + by: y0 + 2 * by, x0 + bx: x0 + 2 * bx]
    return out


NX, NY, NZ, NSYMBT = 1000, 700, 30, 96
D0 = 256 + NSYMBT // 4


def _mrc_volume():
    rng = np.random.default_rng(5)
    w = np.zeros(D0 + NX * NY * NZ, np.uint32)
    w[:256] = util.kat_words(256)
    w[0:4] = [NX, NY, NZ, 2]
    w[23] = NSYMBT
    w[D0:] = rng.normal(100.0, 20.0, NX * NY * NZ).astype(np.float32).view(np.uint32)
    return w


CENTRES = np.array([[500, 350, 15], [0.5, 0.5, 0.5], [999.4, 699.6, 29.5], [-40, 300, 10], [512.5, 100.49, 8.5], [10, 10, 45],
                    [300, 690, 1], [700.7, 20.2, 22.5], [1200, 350, 15], [250, 250, 12]], np.float64)


def test_read_mrc_boxes_equals_numpy_slicing(codec, tmp_path):
    import torch
    w = _mrc_volume()
    z = codec.zip_bytes(w.tobytes(), 10)
    p = tmp_path / "vol.mrc.zip"
    p.write_bytes(z)
    vol = np.frombuffer(codec.unzip_bytes(z), np.uint32)[D0:].reshape(NZ, NY, NX)
    for size, fill in ((64, 0.0), ((33, 17, 9), -2.5), ((1, 1, 1), float("nan")), (np.int64(20), 7.0)):
        s3 = (int(size),) * 3 if np.ndim(size) == 0 else size
        got = codec.read_mrc_boxes(p, CENTRES, size, fill=fill)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(CENTRES), s3[2], s3[1], s3[0])
        org = np.floor(CENTRES + 0.5).astype(np.int64) - np.array(s3) // 2
        fb = int(np.array([fill], np.float32).view(np.uint32)[0])
        assert np.array_equal(got.cpu().numpy().view(np.uint32), _expect_np(vol, org, s3, fb)), size
    # integer centres from a list, a container in memory
    got = codec.read_mrc_boxes(z, [[100, 200, 3], [101, 201, 3]], (8, 6, 4))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _expect_np(vol, [[96, 197, 1], [97, 198, 1]], (8, 6, 4), 0))
    # only the touched records are read: a file cut after chunk 0 still gives boxes inside chunk 0
    end0 = 17 + 16 + sum(int(x) & 0x7fffffff for x in np.frombuffer(z[17:33], "<u4"))
    cut = tmp_path / "cut.mrc.zip"
    cut.write_bytes(z[:end0])
    got = codec.read_mrc_boxes(cut, [[500, 350, 3], [-5, 3, 2]], 8)          # sections -1 .. 6: chunk 0 holds sections 0 .. 8
    org = np.array([[496, 346, -1], [-9, -1, -2]])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _expect_np(vol, org, (8, 8, 8), 0))
    from datacompressionfloat_amd import MrczError
    with pytest.raises(MrczError):
        codec.read_mrc_boxes(cut, [[500, 350, 25]], 16)
    assert tuple(codec.read_mrc_boxes(p, np.zeros((0, 3)), 8).shape) == (0, 8, 8, 8)


def test_mrc_extract_boxes_equal_the_mrc_tar_slice(tmp_path):
    w = _mrc_volume()
    src, z, back = tmp_path / "vol.mrc", tmp_path / "vol.mrc.zip", tmp_path / "back.mrc"
    src.write_bytes(w.tobytes())
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([os.path.join(BIN, "mrc_tar"), "-i", str(z), "-o", str(back), "-t", "unzip"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    vol = np.fromfile(back, np.uint32)[D0:].reshape(NZ, NY, NX)
    cfile = tmp_path / "centres.txt"
    cfile.write_text("# picked\n" + "\n".join(" ".join(str(v) for v in c) for c in CENTRES) + "\n\n")
    out = tmp_path / "boxes.raw"
    r = subprocess.run([os.path.join(BIN, "mrc_extract"), "-i", str(z), "-o", str(out), "-B", str(cfile), "-S", "48,32,16", "-F", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    org = np.floor(CENTRES + 0.5).astype(np.int64) - np.array([24, 16, 8])
    exp = _expect_np(vol, org, (48, 32, 16), 0x3F800000)
    assert np.array_equal(np.fromfile(out, np.uint32).reshape(exp.shape), exp)


def test_many_random_boxes_through_small_batches():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    nx, ny, nz, d0 = 1024, 1024, 72, 256            # 13 chunks
    n = d0 + nx * ny * nz
    big = MrcZipCodec(0, max_batch_chunks=13)
    small = MrcZipCodec(0, max_batch_chunks=4)      # covered runs of up to four chunks: several batches per call
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    big.generate_kat_device(words, 0)
    rec, _ = big.compress_device(words, 8, 0)
    del words
    full, _ = big.uncompress_device(rec, n)
    rng = np.random.default_rng(17)
    org = np.stack([rng.integers(-40, nx + 8, 2000), rng.integers(-40, ny + 8, 2000), rng.integers(-40, nz + 8, 2000)], 1).astype(np.int32)
    fill = 0x7FC01234
    g = _geom(d0, nx, ny, nz, 32, 32, 32, fill)
    import ctypes
    from datacompressionfloat_amd import codec as codec_mod
    covered = np.zeros(13, np.uint8)
    assert codec_mod._LIB.mrcz_boxes_chunks(ctypes.byref(g), org.ctypes.data, len(org), n, CHK, covered.ctypes.data) == 0
    assert covered.sum() >= 12
    out, decoded = small.uncompress_boxes_device(rec, n, g, org)
    assert decoded == covered.sum()
    o = torch.from_numpy(org.astype(np.int64)).cuda()
    r = torch.arange(32, device="cuda")
    x = o[:, 0, None, None, None] + r[None, None, None, :]
    y = o[:, 1, None, None, None] + r[None, None, :, None]
    zz = o[:, 2, None, None, None] + r[None, :, None, None]
    inside = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (zz >= 0) & (zz < nz)
    idx = torch.where(inside, d0 + (zz * ny + y) * nx + x, torch.zeros_like(x))
    exp = torch.where(inside, full[idx], torch.full_like(idx, fill, dtype=torch.int32).to(torch.int32))
    assert torch.equal(out, exp.to(torch.int32))
    # the same boxes from the whole-volume context: one batch
    out2, decoded2 = big.uncompress_boxes_device(rec, n, g, org)
    assert decoded2 == decoded and torch.equal(out2, out)
    big.close()
    small.close()


def test_a_skipped_middle_chunk_is_never_decoded(codec):
    import torch
    nx, ny, nz, d0 = 13000000, 2, 1, 256
    n = d0 + nx * ny * nz                            # five chunks; row 1 starts in chunk 2
    rng = np.random.default_rng(23)
    w = rng.normal(0.0, 1.0, n).astype(np.float32).view(np.uint32)
    rec, _ = codec.compress_device(torch.from_numpy(w.view(np.int32)).cuda(), 8, 0)
    rec = rec.clone()
    full = util.erase_expected(w, 8)
    offs, off = [], 0
    h = rec.cpu().numpy()
    for _ in range(5):
        offs.append(off)
        off += 16 + int(sum(int(v) & 0x7fffffff for v in h[off: off + 16].view("<u4")))
    rec[offs[1] + 16: offs[2]] = torch.from_numpy(rng.integers(0, 256, offs[2] - offs[1] - 16, dtype=np.uint8)).cuda()
    # box 0: row 0 in chunk 0, row 1 in chunk 2; box 1: the end of row 1 (chunk 4) and a row past the volume
    org = np.array([[0, 0, 0], [12999990, 1, 0]], np.int32)
    g = _geom(d0, nx, ny, nz, 64, 2, 1, 0xFFFFFFFF)
    out, decoded = codec.uncompress_boxes_device(rec, n, g, org)
    assert decoded == 3                               # chunks 0, 2 and 4; chunk 1 (garbage) and chunk 3 only walked
    vol = full[d0:].reshape(1, ny, nx)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _expect_np(vol, org, (64, 2, 1), 0xFFFFFFFF))


def test_lz4_fixtures_as_flat_volumes(codec):
    import torch
    from golden.make_golden import lz4_cases
    for name in lz4_cases():
        z = open(os.path.join(util.GOLDEN, name + ".zip"), "rb").read()
        full = np.frombuffer(codec.unzip_bytes(z), np.uint32)
        nfl, chk = codec._container_header(io.BytesIO(z))    # sets the context's compressor types (LZ4 planes)
        nx = nfl - 256
        g = _geom(256, nx, 1, 1, 100, 3, 1, 0x12345678)
        org = np.array([[0, 0, 0], [-50, -1, 0], [nx - 60, 0, 0], [nx // 2, -2, 0], [nx + 5, 0, 0], [17, 0, -1]], np.int32)
        rec = torch.frombuffer(bytearray(z[17:]), dtype=torch.uint8).cuda()
        out, decoded = codec.uncompress_boxes_device(rec, nfl, g, org, chk=chk)
        assert decoded == 1
        exp = _expect_np(full[256:].reshape(1, 1, nx), org, (100, 3, 1), 0x12345678)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), exp), name
