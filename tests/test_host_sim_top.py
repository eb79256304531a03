"""CPU-only: top-planes decode from the command line (mrc_extract -P keep [-H]) linked against the SIMT-emulator build of the codec,
and the reader of MrcZipCodec.unzip_top / read_mrc_top (read_thinned_records) feeding the emulator.  The outputs must equal
oracle.uncompress(container) & mask(keep), byte for byte; the same with every dropped payload of the container replaced by 0xFF
on disk; the reader must not touch one byte of a dropped payload; bad arguments end with exit status 255, not a signal."""
import os
import subprocess

import numpy as np
import pytest

import top_ref as ref
import util
from top_ref import COMBOS

HOST = os.path.join(util.ROOT, "datacompressionfloat_amd", "host")
CHK = util.CHUNK
NX, NY, NZ, NSYMBT = 256, 128, 400, 80
D0 = (1024 + NSYMBT) // 4
N = D0 + NX * NY * NZ + 37                                  # three chunks, the last short and ragged, a tail behind the volume


def _volume():
    w = util.gauss_words(N, seed=41)
    w[0:4] = [NX, NY, NZ, 2]
    w[23] = NSYMBT
    w[4:23] = util.kat_words(19)                            # header words with bits in every plane: truncated like the rest
    w[D0 + 5: D0 + 12] = [0x7F800001, 0xFFC00000, 0x7F800000, 0x80000000, 0x00000100, 0x7F80FF00, 0x00012345]   # NaN whose payload is dropped, ...
    return w


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)


@pytest.fixture(scope="module")
def env(tmp_path_factory, oracle):
    sim = util.load_sim()
    ref.bind(sim.lib)
    d = tmp_path_factory.mktemp("top")
    link = ["-L" + util.SIM_DIR, "-lmrcz_sim", "-lpthread", "-lm", "-lstdc++", "-Wl,-rpath," + util.SIM_DIR]
    exe = str(d / "mrc_extract")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-o", exe, os.path.join(HOST, "mrc_extract.c")] + link)
    w = _volume()
    out = {"exe": exe, "dir": d, "sim": sim}
    for tag, bits in (("b8", 8), ("b0", 0)):
        z = oracle.compress(w.tobytes(), bits)
        (d / f"{tag}.zip").write_bytes(z)
        out[tag] = (str(d / f"{tag}.zip"), z, np.frombuffer(oracle.uncompress(z), np.uint32))
    return out


def _extract(env, zpath, keep, u16, tag):
    o = env["dir"] / f"{tag}.raw"
    r = _run([env["exe"], "-i", str(zpath), "-o", str(o), "-P", str(keep)] + (["-H"] if u16 else []))
    return r, (np.fromfile(o, np.uint16 if u16 else np.uint32) if r.returncode == 0 else None)


@pytest.mark.parametrize("keep,u16", COMBOS)
def test_mrc_extract_P_equals_the_full_decode_under_the_mask(env, keep, u16):
    for tag in ("b8", "b0"):
        zpath, z, full = env[tag]
        r, got = _extract(env, zpath, keep, u16, f"{tag}_{keep}_{int(u16)}")
        assert r.returncode == 0, r.stderr
        assert np.array_equal(got, ref.expected(full, keep, u16)), tag


@pytest.mark.parametrize("keep,u16", [(2, True), (3, False)])
def test_dropped_payloads_replaced_by_ff_on_disk(env, keep, u16):
    zpath, z, full = env["b8" if keep == 3 else "b0"]
    bad = z[:17] + ref.poison(z[17:], N, keep)
    assert bad != z
    p = env["dir"] / f"ff{keep}.zip"
    p.write_bytes(bad)
    r, got = _extract(env, p, keep, u16, f"ff{keep}")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(got, ref.expected(full, keep, u16))


class _Tracked:
    """a binary file that records every byte range read from it"""

    def __init__(self, path):
        self.f, self.pos, self.reads = open(path, "rb"), 0, []

    def seek(self, off, whence=0):
        self.pos = self.f.seek(off, whence)
        return self.pos

    def read(self, n=-1):
        b = self.f.read(n)
        self.reads.append((self.pos, self.pos + len(b)))
        self.pos += len(b)
        return b

    def close(self):
        self.f.close()


@pytest.mark.parametrize("keep,u16", [(2, True), (3, False)])
def test_the_python_reader_builds_thinned_records_and_reads_no_dropped_byte(env, keep, u16):
    """what unzip_top / read_mrc_top do with a path, piece by piece, the emulator in the place of the GPU"""
    import ctypes
    from datacompressionfloat_amd import read_thinned_records
    sim = env["sim"]
    zpath, z, full = env["b0" if keep == 2 else "b8"]
    rec = z[17:]
    offs = ref.offsets(rec, N)
    f = _Tracked(zpath)
    esz = 2 if u16 else 4
    out = util.aligned_empty(esz * (N + 8))
    off = 17
    for k, n in ((0, 2), (2, 1)):                           # pieces of two chunks, as a codec of max_batch_chunks = 2 reads them
        body, off = read_thinned_records(f, N, CHK, keep, k, n, start=off)
        assert body == ref.thin(sim.lib, rec[offs[k]: offs[k + n]], N, keep, first_chunk=k)
        r = util.aligned_empty(len(body) + 16)
        r[: len(body)] = np.frombuffer(body, np.uint8)
        cons = ctypes.c_uint64()
        rc = sim.lib.mrcz_uncompress_top(sim.ctx, r.ctypes.data, len(body), N, CHK, k, n, keep, (ref.U16 if u16 else ref.F32) | ref.THINNED,
                                         out[esz * k * CHK:].ctypes.data, ctypes.byref(cons))
        assert rc == 0 and cons.value == len(body)
    assert off == len(z)
    f.close()
    got = out.view(np.uint16 if u16 else np.uint32)[:N]
    assert np.array_equal(got, ref.expected(full, keep, u16))
    vol = got[D0: D0 + NX * NY * NZ].reshape(NZ, NY, NX)    # what read_mrc_top returns
    assert np.array_equal(vol, ref.expected(full[D0: D0 + NX * NY * NZ], keep, u16).reshape(NZ, NY, NX))
    dropped = []                                            # byte ranges of the container that hold dropped payloads
    for c in range(3):
        ln = ref.lengths(rec[offs[c]: offs[c] + 16])
        dropped.append((17 + offs[c] + 16, 17 + offs[c] + 16 + sum(ln[: 4 - keep])))
    assert sum(b - a for a, b in dropped) >= (2 * N if keep == 2 else 1)     # -b 0 of noise: two RAW planes per chunk are left unread
    for a, b in f.reads:
        assert all(b <= da or a >= db for da, db in dropped), (a, b)
    # the walk without a known start gives the same records
    f = _Tracked(zpath)
    assert read_thinned_records(f, N, CHK, keep, 2, 1)[0] == ref.thin(sim.lib, rec[offs[2]:], N, keep, first_chunk=2)
    assert all(b - a == 16 for a, b in f.reads[:-1])
    f.close()


def test_bad_arguments_exit_255(env):
    zpath = env["b8"][0]
    o = str(env["dir"] / "bad.raw")
    cases = {
        "keep_1": ["-P", "1"], "keep_4": ["-P", "4"], "keep_0": ["-P", "0"], "junk": ["-P", "2x"], "empty": ["-P", ""], "negative": ["-P", "-2"],
        "H_with_3": ["-P", "3", "-H"], "H_alone": ["-H", "-w", "0:10"], "with_w": ["-P", "2", "-w", "0:10"], "with_z": ["-P", "2", "-z", "0:1"],
        "with_N": ["-P", "2", "-N", "2"], "with_B": ["-P", "2", "-B", zpath, "-S", "8"], "with_S": ["-P", "2", "-S", "8"], "int": ["-P", "2", "-s", "int"],
        "nothing": ["-P", "2", "-i", str(env["dir"] / "nothing.zip")],
    }
    for what, extra in cases.items():
        r = _run([env["exe"], "-i", zpath, "-o", o] + extra)
        assert r.returncode == 255, (what, r.returncode, r.stderr)          # an exit status, not a signal (< 0)
        assert "ERROR" in r.stderr, (what, r.stderr)
    z = env["b8"][1]
    cut = env["dir"] / "cut.zip"
    cut.write_bytes(z[: len(z) - 1000])                                        # the last kept payload ends early
    r = _run([env["exe"], "-i", str(cut), "-o", o, "-P", "2"])
    assert r.returncode == 255 and "ERROR" in r.stderr
