"""CPU-only: digest decode from the command line (mrc_verify -k / -K, mrc_tar -k / -K) linked against the SIMT-emulator build of
the codec.  The yardstick is Python's zlib.crc32 over the CPU oracle's decode; every comparison is equality of 32-bit values.
Exit status 0 / 1 is the verdict, 255 a refusal, never a signal."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import crc_ref as ref
import util
from abs_error_ref import abs_round, f32_toward_zero
from test_host_sim import _several_batches_and_a_ragged_tail

HOST = os.path.join(util.ROOT, "datacompressionfloat_amd", "host")
CHK = util.CHUNK
N = 2 * CHK + 70001                  # three chunks, the last short
EPS = f32_toward_zero(0.01)


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500, env=e)


def _sidecar(dec, mode="float"):
    from datacompressionfloat_amd import format_sidecar
    return format_sidecar(len(dec), CHK, mode, zlib.crc32(dec.tobytes()), [c for c, _ in ref.chunk_crcs(dec)])


def _offsets(rec, nfl):
    offs, off = [], 0
    for c in range((nfl + CHK - 1) // CHK):
        offs.append(off)
        off += 16 + int(sum(int(x) & 0x7fffffff for x in np.frombuffer(rec[off: off + 16], "<u4")))
    return offs + [off]


@pytest.fixture(scope="module")
def env(tmp_path_factory, oracle):
    util.load_sim()
    d = tmp_path_factory.mktemp("digest")
    link = ["-L" + util.SIM_DIR, "-lmrcz_sim", "-lpthread", "-lm", "-lstdc++", "-Wl,-rpath," + util.SIM_DIR]
    cc = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall"]
    subprocess.check_call(cc + ["-o", str(d / "mrc_verify"), os.path.join(HOST, "mrc_verify.c")] + link)
    subprocess.check_call(cc + ["-o", str(d / "mrc_tar")] + [os.path.join(HOST, f) for f in ("mrc_tar.c", "workers_gpu.c", "common_gpu.c", "adapt_gpu.c")] + link)
    w = util.gauss_words(N, seed=77)
    (d / "vol.mrc").write_bytes(w.tobytes())
    out = {"verify": str(d / "mrc_verify"), "tar": str(d / "mrc_tar"), "dir": d, "w": w, "orig": str(d / "vol.mrc")}
    for tag, z, im in (("b8", oracle.compress(w.tobytes(), 8), False), ("int", oracle.compress_int(w.tobytes()), True)):
        (d / f"{tag}.zip").write_bytes(z)
        dec = np.frombuffer(oracle.uncompress(z, int_mode=im), np.uint32)
        (d / f"{tag}.crc").write_text(_sidecar(dec, "int" if im else "float"))
        out[tag] = (str(d / f"{tag}.zip"), dec, str(d / f"{tag}.crc"), z)
    # silent damage: one bit of one byte of a RAW payload of chunk 1 (the plane is found by the RAW bit of the chunk header)
    z = out["b8"][3]
    rec = bytearray(z[17:])
    span = ref.raw_payload_span(bytes(rec), _offsets(bytes(rec), N), 1, CHK)
    assert span is not None, "a -b 8 container of Gaussian words has a RAW plane"
    rec[span[1] + 4321] ^= 0x04
    bad = z[:17] + bytes(rec)
    (d / "bad.zip").write_bytes(bad)
    out["bad"] = (str(d / "bad.zip"), np.frombuffer(oracle.uncompress(bad), np.uint32))
    return out


def test_mrc_verify_k_prints_the_expected_sidecar(env):
    from datacompressionfloat_amd import parse_sidecar
    for tag, extra in (("b8", []), ("int", ["-s", "int"])):
        z, dec, crc, _ = env[tag]
        r = _run([env["verify"], "-z", z, "-k"] + extra)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert r.stdout == open(crc).read()
        sc = parse_sidecar(r.stdout)
        assert sc["file"] == zlib.crc32(dec.tobytes()) and sc["crcs"] == [c for c, _ in ref.chunk_crcs(dec)]
    r = _run([env["verify"], "-a", env["orig"], "-k"])                       # a plain file: what crc32(1) prints
    assert r.returncode == 0 and r.stdout == _sidecar(env["w"])
    assert parse_sidecar(r.stdout)["file"] == zlib.crc32(open(env["orig"], "rb").read())


def test_mrc_verify_K_exit_status(env):
    d = env["dir"]
    z, dec, crc, raw = env["b8"]
    r = _run([env["verify"], "-z", z, "-K", crc])
    assert r.returncode == 0 and r.stdout == "file expected %08x got %08x\n" % ((zlib.crc32(dec.tobytes()),) * 2), (r.stdout, r.stderr)
    r = _run([env["verify"], "-z", env["int"][0], "-K", env["int"][2]])      # the mode is the sidecar's
    assert r.returncode == 0, (r.stdout, r.stderr)
    # the damaged container decodes (nobody is told), and only chunk 1 is named
    bz, bdec = env["bad"]
    want, got = ref.chunk_crcs(dec), ref.chunk_crcs(bdec)
    assert got[1] != want[1] and got[0] == want[0] and got[2] == want[2]
    r = _run([env["verify"], "-z", bz, "-K", crc])
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stdout == "chunk 1 expected %08x got %08x\nfile expected %08x got %08x\n" % (want[1][0], got[1][0], zlib.crc32(dec.tobytes()), zlib.crc32(bdec.tobytes()))
    # refusals: a sidecar of another file, a truncated container, missing files, damaged sidecars, excluded options
    other = _sidecar(dec[: CHK + 5])
    (d / "other.crc").write_text(other)
    (d / "cut.zip").write_bytes(raw[: len(raw) - 1000])
    (d / "cut_header.zip").write_bytes(raw[:10])
    text = open(crc).read()
    (d / "upper.crc").write_text(text.upper())
    (d / "short.crc").write_text(text[: text.rindex("\n2 ") + 1])
    (d / "long.crc").write_text(text + "3 00000000\n")
    (d / "empty.crc").write_text("")
    for args in (["-z", z, "-K", str(d / "other.crc")], ["-z", str(d / "cut.zip"), "-K", crc], ["-z", str(d / "cut_header.zip"), "-K", crc],
                 ["-z", str(d / "nothing.zip"), "-K", crc], ["-z", z, "-K", str(d / "nothing.crc")], ["-z", z, "-K", str(d / "upper.crc")],
                 ["-z", z, "-K", str(d / "short.crc")], ["-z", z, "-K", str(d / "long.crc")], ["-z", z, "-K", str(d / "empty.crc")],
                 ["-z", z, "-K", z], ["-z", z, "-K", crc, "-e", "0.1"], ["-z", z, "-k", "-r", "0.1"], ["-z", z, "-k", "-K", crc],
                 ["-a", env["orig"], "-z", z, "-K", crc], ["-a", env["orig"], "-z", z, "-k"], ["-k"], ["-z", str(d / "cut.zip"), "-k"],
                 ["-a", str(d / "nothing.mrc"), "-k"], ["-z", z, "-k", "-s", "double"]):
        r = _run([env["verify"]] + args)
        assert r.returncode == 255, (args, r.returncode, r.stderr)


@pytest.mark.parametrize("mode", ["b8", "eps", "int"])
def test_mrc_tar_k_writes_the_sidecar_mrc_verify_prints(env, oracle, tmp_path, mode):
    """two emulated devices, one chunk per batch, three chunks with a short last one: the writer's file order of chunk digests"""
    w = _several_batches_and_a_ragged_tail()
    src, z = tmp_path / "in.mrc", tmp_path / "o.zip"
    src.write_bytes(w.tobytes())
    e = {"SIM_DEVICES": "2", "MRCZ_BATCH_CHUNKS": "1"}
    opts, vopts, im = {"b8": (["-b", "8"], [], False), "eps": (["-e", "0.01"], [], False), "int": (["-s", "int"], ["-s", "int"], True)}[mode]
    r = _run([env["tar"], "-i", str(src), "-o", str(z), "-t", "zip", "-G", "2", "-k"] + opts, env=e)
    assert r.returncode == 0, r.stderr
    want_z = {"b8": lambda: oracle.compress(w.tobytes(), 8), "eps": lambda: oracle.compress(abs_round(w, EPS).tobytes(), 0), "int": lambda: oracle.compress_int(w.tobytes())}[mode]()
    assert z.read_bytes() == want_z                                          # the container is what it is without -k
    dec = np.frombuffer(oracle.uncompress(want_z, int_mode=im), np.uint32)
    side = open(str(z) + ".crc").read()
    assert side == _sidecar(dec, "int" if im else "float")
    r = _run([env["verify"], "-z", str(z), "-k"] + vopts)
    assert r.returncode == 0 and r.stdout == side
    # one device, one batch: the same sidecar
    r = _run([env["tar"], "-i", str(src), "-o", str(z), "-t", "zip", "-k"] + opts)
    assert r.returncode == 0 and open(str(z) + ".crc").read() == side


def test_mrc_tar_unzip_K(env, tmp_path):
    z, dec, crc, _ = env["b8"]
    back = tmp_path / "b.mrc"
    for e in ({}, {"SIM_DEVICES": "2", "MRCZ_BATCH_CHUNKS": "1"}):
        r = _run([env["tar"], "-i", z, "-o", str(back), "-t", "unzip", "-G", "0", "-K", crc], env=e)
        assert r.returncode == 0 and "file expected %08x got %08x" % ((zlib.crc32(dec.tobytes()),) * 2) in r.stdout, (r.returncode, r.stderr)
        assert back.read_bytes() == dec.tobytes()
        back.unlink()
    bz, bdec = env["bad"]
    want, got = ref.chunk_crcs(dec), ref.chunk_crcs(bdec)
    r = _run([env["tar"], "-i", bz, "-o", str(back), "-t", "unzip", "-K", crc], env={"MRCZ_BATCH_CHUNKS": "2"})
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "chunk 1 expected %08x got %08x\n" % (want[1][0], got[1][0]) in r.stdout and "chunk 0 " not in r.stdout and "chunk 2 " not in r.stdout
    assert back.read_bytes() == bdec.tobytes()                                # the output is written either way
    (tmp_path / "other.crc").write_text(_sidecar(dec[: CHK + 5]))
    r = _run([env["tar"], "-i", z, "-o", str(back), "-t", "unzip", "-K", str(tmp_path / "other.crc")])
    assert r.returncode == 255
    r = _run([env["tar"], "-i", z, "-o", str(back), "-t", "unzip", "-K", str(tmp_path / "nothing.crc")])
    assert r.returncode == 255


def test_without_k_the_pipeline_enqueues_no_digest(env, tmp_path):
    """opt-in: without -k no sidecar is written and the container is the oracle's; -k with unzip is refused"""
    w = util.gauss_words(70001, seed=3)
    src, z = tmp_path / "in.mrc", tmp_path / "o.zip"
    src.write_bytes(w.tobytes())
    r = _run([env["tar"], "-i", str(src), "-o", str(z), "-t", "zip", "-b", "8"])
    assert r.returncode == 0 and not os.path.exists(str(z) + ".crc")
    assert z.read_bytes() == util.load_oracle().compress(w.tobytes(), 8)
    r = _run([env["tar"], "-i", str(src), "-o", str(z), "-t", "unzip", "-k"])
    assert r.returncode == 255                                                # -k goes with zip
