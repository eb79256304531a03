"""GPU: the absolute-error mode on the MI355X.  compress_device(abs_err=eps) writes the oracle's -b 0 container of the words
abs_error_ref.abs_round gives; every reader (whole, range, boxes, binned, the reference's own mrc_tar) decodes it to those
words with no option; `mrc_tar -e` / `erasebytes -e` / `erroranalysis` agree; the bound holds."""
import os
import subprocess

import numpy as np
import pytest

import util
from abs_error_ref import abs_round, f32_toward_zero, max_abs_error

pytestmark = pytest.mark.gpu

BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")
EPS = [2.0 ** -10, 0.01, 0.5]

NX, NY, NZ, NSYMBT = 1024, 1024, 16, 0
D0 = 256 + NSYMBT // 4  # 16 Mi voxels after the header: 64 MiB, two full chunks and a ragged third


def _run(args, **kw):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, **kw)


def _mrc_volume():
    """a cryo-EM-like map: mostly near-zero solvent, a denser blob of larger values"""
    rng = np.random.default_rng(17)
    w = np.zeros(D0 + NX * NY * NZ, np.uint32)
    w[:256] = util.kat_words(256)
    w[0:4] = [NX, NY, NZ, 2]
    w[23] = NSYMBT
    v = rng.normal(0.0, 0.05, (NZ, NY, NX)).astype(np.float32)
    v[4:12, 300:700, 300:700] += rng.normal(3.0, 1.0, (8, 400, 400)).astype(np.float32)
    w[D0:] = v.reshape(-1).view(np.uint32)
    return w


@pytest.fixture(scope="module")
def codec():
    import torch
    from datacompressionfloat_amd import MrcZipCodec
    assert torch.cuda.is_available()
    c = MrcZipCodec(0, max_batch_chunks=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def volume():
    return _mrc_volume()


@pytest.mark.parametrize("eps", EPS)
def test_compress_device_equals_the_oracle_container_of_the_rounded_words(codec, oracle, volume, eps):
    import torch
    e32 = f32_toward_zero(eps)
    for w in (volume, util.poisson_words(2 * util.CHUNK + 4321, seed=8)):
        want = abs_round(w, e32)
        dev = torch.from_numpy(w.view(np.int32).copy()).cuda()
        rec, planes = codec.compress_device(dev, 0, abs_err=eps)
        ref = oracle.compress(want.tobytes(), 0, threads=8)
        assert rec.cpu().numpy().tobytes() == ref[17:], (len(w), eps)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), w)  # the input is not rounded in place
        back, _ = codec.uncompress_device(rec, len(w))
        assert np.array_equal(back.cpu().numpy().view(np.uint32), want)
        assert max_abs_error(w, want) <= float(e32)
        assert np.array_equal(codec.erase_abs_device(dev, eps).cpu().numpy().view(np.uint32), want)


def test_range_box_and_binned_reads_of_the_container(codec, oracle, volume, tmp_path):
    from test_gpu_binned import bin_expected, _same_bits
    from test_gpu_boxes import _expect_np
    eps = 0.01
    want = abs_round(volume, f32_toward_zero(eps))
    z = codec.zip_bytes(volume.tobytes(), 0, abs_err=eps)
    assert z == oracle.compress(want.tobytes(), 0, threads=8)
    p = tmp_path / "vol.mrc.zip"
    p.write_bytes(z)
    assert codec.unzip_bytes(z) == want.tobytes()
    for w0, w1 in ((0, 300), (util.CHUNK - 5, util.CHUNK + 7), (len(volume) - 1000, len(volume)), (123456, 2 * util.CHUNK + 99)):
        assert codec.unzip_range(p, w0, w1) == want[w0:w1].tobytes(), (w0, w1)
    vol = want[D0:].reshape(NZ, NY, NX)
    centres = np.array([[500, 500, 8], [10, 10, 1], [1020, 900, 15], [512.5, 300.4, 3.5]], np.float64)
    got = codec.read_mrc_boxes(p, centres, 32)
    org = np.floor(centres + 0.5).astype(np.int64) - 16
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _expect_np(vol, org, (32, 32, 32), 0))
    for f in (2, (4, 4, 2)):
        f3 = (f,) * 3 if np.ndim(f) == 0 else f
        assert _same_bits(codec.read_mrc_binned(p, f).cpu().numpy(), bin_expected(vol, *f3)), f


def test_bad_bounds_and_excluded_combinations(codec):
    import torch
    from datacompressionfloat_amd import MrczError
    w = util.gauss_words(5000)
    dev = torch.from_numpy(w.view(np.int32).copy()).cuda()
    for eps in (0.0, -1.0, float("nan"), float("inf"), 1e-50):
        with pytest.raises(MrczError):
            codec.compress_device(dev, 0, abs_err=eps)
        with pytest.raises(MrczError):
            codec.erase_abs_device(dev, eps)
    with pytest.raises(MrczError):
        codec.zip_bytes(w.tobytes(), 8, abs_err=0.01)
    with pytest.raises(MrczError):
        codec.zip_bytes(w.tobytes(), 0, mode="int", abs_err=0.01)
    assert codec.zip_bytes(w.tobytes(), 8) == codec.zip_bytes(w.tobytes(), 8, abs_err=None)  # existing calls unchanged


def test_mrc_tar_e_erasebytes_e_and_erroranalysis(oracle, volume, tmp_path):
    tar, era, ea = (os.path.join(BIN, n) for n in ("mrc_tar", "erasebytes", "erroranalysis"))
    a, z, b, e = tmp_path / "a.mrc", tmp_path / "a.zip", tmp_path / "b.mrc", tmp_path / "e.mrc"
    a.write_bytes(volume.tobytes() + b"xy")
    for eps in (2.0 ** -10, 0.25):
        want = abs_round(volume, f32_toward_zero(eps))
        r = _run([tar, "-i", str(a), "-o", str(z), "-e", repr(eps), "-t", "zip"], env=dict(os.environ, MRCZ_BATCH_CHUNKS="1"))
        assert r.returncode == 0, r.stderr
        assert z.read_bytes() == oracle.compress(want.tobytes() + b"xy", 0, threads=8)
        assert _run([tar, "-i", str(z), "-o", str(b), "-t", "unzip"]).returncode == 0
        assert b.read_bytes() == want.tobytes()
        assert _run([era, "-i", str(a), "-o", str(e), "-e", repr(eps)]).returncode == 0
        assert e.read_bytes() == want.tobytes()
        r = _run([ea, "-a", str(a), "-b", str(b), "-k", "3"])
        assert r.returncode == 0, r.stderr
        worst = [float(line.split()[3]) for line in r.stdout.splitlines()]
        assert len(worst) == 3 and 0 < max(worst) <= eps  # powers of two: %E prints them exactly
    for bad in (["-e", "0.01", "-b", "4"], ["-e", "0.01", "-s", "int"], ["-e", "-3"]):
        assert _run([tar, "-i", str(a), "-o", str(z), "-t", "zip"] + bad).returncode != 0, bad


@pytest.mark.skipif(util.ref_binary("mrc_tar_c") is None, reason="oracle/_ref not present on this box")
def test_the_reference_binary_reads_and_writes_the_same_container(tmp_path):
    """compressible planes (no full-size chunk whose plane overflows the reference's 6 MiB buffer)"""
    tar, ref = os.path.join(BIN, "mrc_tar"), util.ref_binary("mrc_tar_c")
    w = util.gauss_words(util.CHUNK + 12345, seed=23)
    eps = 0.01
    want = abs_round(w, f32_toward_zero(eps))
    src, rnd, z1, z2, back = (tmp_path / n for n in ("in.mrc", "rounded.mrc", "gpu.zip", "ref.zip", "back.mrc"))
    src.write_bytes(w.tobytes())
    rnd.write_bytes(want.tobytes())
    assert _run([tar, "-i", str(src), "-o", str(z1), "-e", str(eps), "-t", "zip"]).returncode == 0
    assert _run([ref, "-i", str(z1), "-o", str(back), "-t", "unzip"]).returncode == 0
    assert back.read_bytes() == want.tobytes()
    assert _run([ref, "-i", str(rnd), "-o", str(z2), "-b", "0", "-t", "zip"]).returncode == 0
    assert z2.read_bytes() == z1.read_bytes()
