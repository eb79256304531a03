"""GPU: digest decode on the MI355X.  The three-chunk volume of tests/test_sim_digest.py in its four containers (written by the CPU
oracle) through the C ABI (device buffers) and through MrcZipCodec; the yardstick is Python's zlib.crc32 over the CPU oracle's
decode, every comparison equality of 32-bit values.  bench.py's 1 GiB volume at -b 8 and at an absolute bound of 1e-3: the file
digest equals zlib.crc32 of the host copy of uncompress_device's output and digest_words_device of the original."""
import ctypes
import sys
import zlib

import numpy as np
import pytest

import crc_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero

pytestmark = pytest.mark.gpu

CHK = util.CHUNK
EPS_SMALL = f32_toward_zero(0.01)
EPS_BIG = f32_toward_zero(1e-3)
MODES = {"b8": ("mask", 8, None, False), "b0": ("mask", 0, None, False), "eps": ("abs", 0, float(EPS_SMALL), False), "int": ("int", 0, None, True)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def small(oracle):
    from test_sim_binned import _volume
    w = _volume()
    out = {"w": w}
    for tag, z, im in (("b8", oracle.compress(w.tobytes(), 8), False), ("b0", oracle.compress(w.tobytes(), 0), False),
                       ("eps", oracle.compress(abs_round(w, EPS_SMALL).tobytes(), 0), False), ("int", oracle.compress_int(w.tobytes()), True)):
        out[tag] = (z, np.frombuffer(oracle.uncompress(z, int_mode=im), np.uint32))
    return out


def _offsets(rec, nfl):
    offs, off = [], 0
    for c in range((nfl + CHK - 1) // CHK):
        offs.append(off)
        off += 16 + int(sum(int(x) & 0x7fffffff for x in np.frombuffer(rec[off: off + 16], "<u4")))
    offs.append(off)
    return offs


def _abi(torch, codec, z, nfl, pieces=None, garbage=0xA5, int_mode=False):
    """chunk crc32s, (file crc32, bytes) and the raw records through uncompress_digest_device / digest_finish_device"""
    from datacompressionfloat_amd._lib import MrczDigest
    assert ctypes.sizeof(MrczDigest) == ctypes.sizeof(ref.Digest) == 16
    nch = (nfl + CHK - 1) // CHK
    rec = z[17:]
    offs = _offsets(rec, nfl)
    acc = torch.full((nch * 16,), garbage, dtype=torch.uint8, device=codec.device)
    for k, n in pieces or [(0, nch)]:
        r = torch.frombuffer(bytearray(rec[offs[k]: offs[k + n]]), dtype=torch.uint8).to(codec.device)
        codec.uncompress_digest_device(r, nfl, acc, first_chunk=k, nchunks=n, int_mode=int_mode)
    crc, nbytes, chunks = codec.digest_finish_device(acc, 0, nch, per_chunk=True)
    return chunks, (crc, nbytes), acc.cpu().numpy().tobytes()


def test_small_volume_through_the_abi_and_the_codec(torch, small):
    from datacompressionfloat_amd import MrcZipCodec
    codec = MrcZipCodec(0, max_batch_chunks=2)
    w = small["w"]
    n = len(w)
    dw = torch.from_numpy(w.view(np.int32).copy()).to(codec.device)
    for tag, (xform, bits, eps, im) in MODES.items():
        z, dec = small[tag]
        want = [c for c, _ in ref.chunk_crcs(dec)]
        chunks, tot, raw = _abi(torch, codec, z, n, int_mode=im)
        assert chunks == want, tag
        assert tot == (zlib.crc32(dec.tobytes()), 4 * n), tag
        assert ref.records(np.frombuffer(raw, np.uint8), 3) == ref.chunk_crcs(dec)
        assert codec.digest(z, mode="int" if im else "float", per_chunk=True) == (tot[0], want)
        # the two sides agree: the expected decode of the original, without compressing or decoding anything
        acc = codec.digest_words_device(dw, xform, bits, eps)
        assert codec.digest_finish_device(acc, 0, 3, per_chunk=True) == (tot[0], 4 * n, want), tag
        assert acc.cpu().numpy().tobytes() == raw, tag
    acc = codec.digest_words_device(dw)
    assert codec.digest_finish_device(acc, 0, 3) == (zlib.crc32(w.tobytes()), 4 * n)
    # cut invariance on the device: batches of 1, 3 and 64, one call per chunk, reverse order
    z, dec = small["b8"]
    base = _abi(torch, codec, z, n)[2]
    others = {m: MrcZipCodec(0, max_batch_chunks=m) for m in (1, 3, 64)}
    for c, pieces in ((others[1], None), (others[3], None), (others[64], None), (codec, [(0, 1), (1, 1), (2, 1)]), (others[3], [(2, 1), (1, 1), (0, 1)])):
        assert _abi(torch, c, z, n, pieces=pieces, garbage=0x3C)[2] == base, pieces
    for c in list(others.values()) + [codec]:
        c.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 4098, 4099, CHK + 1, CHK + 2, CHK + 3])
def test_small_files_and_short_last_chunks(torch, oracle, n):
    from datacompressionfloat_amd import MrcZipCodec
    codec = MrcZipCodec(0, max_batch_chunks=2)
    w = util.gauss_words(n, seed=n, header=False)
    z = oracle.compress(w.tobytes(), 10)
    dec = np.frombuffer(oracle.uncompress(z), np.uint32)
    assert codec.digest(z, per_chunk=True) == (zlib.crc32(dec.tobytes()), [c for c, _ in ref.chunk_crcs(dec)])
    dw = torch.from_numpy(w.view(np.int32).copy()).to(codec.device)
    nch = (n + CHK - 1) // CHK
    assert codec.digest_finish_device(codec.digest_words_device(dw, "mask", 10), 0, nch) == (zlib.crc32(dec.tobytes()), 4 * n)
    assert codec.digest_finish_device(codec.digest_words_device(dw), 0, nch) == (zlib.crc32(w.tobytes()), 4 * n)
    codec.close()


def test_one_flipped_bit_in_a_raw_plane_is_caught_by_the_sidecar(torch, oracle, tmp_path):
    from datacompressionfloat_amd import MrcZipCodec, MrczError, parse_sidecar
    codec = MrcZipCodec(0, max_batch_chunks=2)
    n = 2 * CHK + 70001
    w = util.gauss_words(n, seed=77)
    z = oracle.compress(w.tobytes(), 8)
    dec = np.frombuffer(oracle.uncompress(z), np.uint32)
    side = tmp_path / "vol.zip.crc"
    text = codec.write_sidecar(z, str(side))
    sc = parse_sidecar(side.read_bytes())
    assert sc["file"] == zlib.crc32(dec.tobytes()) and sc["crcs"] == [c for c, _ in ref.chunk_crcs(dec)] and (sc["words"], sc["chunk"], sc["mode"]) == (n, CHK, "float")
    good = codec.check_sidecar(z, str(side))
    assert good["ok"] and good["differing"] == [] and good["file_got"] == sc["file"]
    rec = bytearray(z[17:])
    span = ref.raw_payload_span(bytes(rec), _offsets(bytes(rec), n), 1, CHK)
    assert span is not None, "a -b 8 container of Gaussian words has a RAW plane"
    rec[span[1] + 12345] ^= 0x10
    bad = z[:17] + bytes(rec)
    back = codec.unzip_bytes(bad)                                             # the premise: it decodes, and nobody is told
    dec_bad = np.frombuffer(oracle.uncompress(bad), np.uint32)
    assert back == dec_bad.tobytes() and int(np.count_nonzero(dec_bad != dec)) == 1
    res = codec.check_sidecar(bad, text)
    want_bad = ref.chunk_crcs(dec_bad)
    assert not res["ok"] and res["differing"] == [(1, sc["crcs"][1], want_bad[1][0])] and res["file_got"] == zlib.crc32(dec_bad.tobytes())
    assert want_bad[0][0] == sc["crcs"][0] and want_bad[2][0] == sc["crcs"][2]
    other = oracle.compress(w[: CHK + 5].tobytes(), 8)                        # a sidecar of another file is refused
    with pytest.raises(MrczError):
        codec.check_sidecar(other, text)
    with pytest.raises(MrczError):
        codec.digest(z[: len(z) - 7])                                         # a truncated container
    codec.close()


def test_one_gib_volume(torch):
    sys.path.insert(0, util.ROOT)
    import bench
    from datacompressionfloat_amd import MrcZipCodec, pack_file_header
    nfl = (1 << 30) // 4
    nch = (nfl + CHK - 1) // CHK
    assert nch == 43
    w = bench.make_volume(nfl, 1234, True)
    c64, c8 = MrcZipCodec(0, max_batch_chunks=64), MrcZipCodec(0, max_batch_chunks=8)
    dw = torch.from_numpy(w.view(np.int32)).to(c64.device)
    eps = float(EPS_BIG)
    for tag in ("b8", "eps"):
        if tag == "b8":
            rec, _ = c64.compress_device(dw, 8)
            acc_w = c64.digest_words_device(dw, "mask", 8)
        else:
            rec, _ = c64.compress_device(dw, 0, abs_err=eps)
            acc_w = c64.digest_words_device(dw, "abs", abs_err=eps)
        out, _ = c64.uncompress_device(rec, nfl)
        host = out.cpu().numpy().tobytes()
        want = zlib.crc32(host)
        want_chunks = [zlib.crc32(host[4 * c * CHK: 4 * (c + 1) * CHK]) for c in range(nch)]
        del out, host
        z = pack_file_header(4 * nfl) + rec.cpu().numpy().tobytes()
        assert c64.digest(z, per_chunk=True) == (want, want_chunks), tag
        assert c8.digest(z, per_chunk=True) == (want, want_chunks), tag     # batches of 8 against one of 64
        assert c64.digest_finish_device(acc_w, 0, nch, per_chunk=True) == (want, 4 * nfl, want_chunks), tag
        del z, rec
    assert c64.digest_finish_device(c64.digest_words_device(dw), 0, nch)[0] == zlib.crc32(w.tobytes())
    c64.close()
    c8.close()


def test_mrc_tar_k_then_mrc_verify_K(tmp_path, oracle):
    """the archive's life from the command line: the sidecar written with the container checks it after the original is gone"""
    import os
    import subprocess
    BIN = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin")
    w = util.gauss_words(2 * CHK + 12345, seed=91)
    a, z, back = tmp_path / "a.mrc", tmp_path / "a.zip", tmp_path / "b.mrc"
    a.write_bytes(w.tobytes())
    run = lambda args: subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    for opts, dec in ((["-b", "8"], util.erase_expected(w, 8)), (["-e", "0.01"], abs_round(w, f32_toward_zero(0.01)))):
        r = run([os.path.join(BIN, "mrc_tar"), "-i", str(a), "-o", str(z), "-t", "zip", "-k"] + opts)
        assert r.returncode == 0, r.stderr
        from datacompressionfloat_amd import parse_sidecar
        sc = parse_sidecar(open(str(z) + ".crc", "rb").read())
        assert sc["file"] == zlib.crc32(dec.tobytes()) and sc["crcs"] == [c for c, _ in ref.chunk_crcs(dec)]
        r = run([os.path.join(BIN, "mrc_verify"), "-z", str(z), "-K", str(z) + ".crc"])
        assert r.returncode == 0, (r.stdout, r.stderr)
        r = run([os.path.join(BIN, "mrc_verify"), "-z", str(z), "-k"])
        assert r.returncode == 0 and r.stdout == open(str(z) + ".crc").read()
        r = run([os.path.join(BIN, "mrc_tar"), "-i", str(z), "-o", str(back), "-t", "unzip", "-K", str(z) + ".crc"])
        assert r.returncode == 0 and back.read_bytes() == dec.tobytes(), (r.returncode, r.stderr)
    raw = bytearray(z.read_bytes())
    span = ref.raw_payload_span(bytes(raw[17:]), _offsets(bytes(raw[17:]), len(w)), 1, CHK)
    if span is None:                                                          # the last container (-e) may hold no RAW plane in chunk 1: any payload byte
        span = (0, _offsets(bytes(raw[17:]), len(w))[1] + 16, 0)
    raw[17 + span[1] + 999] ^= 0x01
    z.write_bytes(bytes(raw))
    r = run([os.path.join(BIN, "mrc_verify"), "-z", str(z), "-K", str(z) + ".crc"])
    assert r.returncode in (1, 255), (r.returncode, r.stdout, r.stderr)       # named, or refused as a malformed stream; never 0
