"""CPU-only: `mrc_tar -e`, `mrc_tarx -e` and `erasebytes -e` (the absolute-error mode through the C host pipeline and the
process-wide setter mrcz_workers_set_abs_error) linked against the SIMT-emulator build of the codec: containers equal the
oracle's -b 0 container of the rounded words, they decode to those words with no option, and the option combinations the
mode excludes end with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

import util
from abs_error_ref import abs_round, f32_toward_zero, max_abs_error

HOST = os.path.join(util.ROOT, "datacompressionfloat_amd", "host")


@pytest.fixture(scope="module")
def simbin(tmp_path_factory):
    util.load_sim()  # builds tests/sim/libmrcz_sim.so
    d = tmp_path_factory.mktemp("hostsim_abs")
    link = ["-L" + util.SIM_DIR, "-lmrcz_sim", "-lpthread", "-lm", "-lstdc++", "-Wl,-rpath," + util.SIM_DIR]
    out = {}
    for main in ("mrc_tar", "mrc_tarx"):
        out[main] = str(d / main)
        subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-o", out[main], os.path.join(HOST, main + ".c"),
                               os.path.join(HOST, "workers_gpu.c"), os.path.join(HOST, "common_gpu.c"), os.path.join(HOST, "adapt_gpu.c")] + link)
    out["erasebytes"] = str(d / "erasebytes")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-o", out["erasebytes"], os.path.join(HOST, "erasebytes.c")] + link)
    return out


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=e)


@pytest.mark.parametrize("n,eps,tail", [(100, 0.01, b""), (70001, 1e-3, b"xyz"), (300000, 0.25, b"")])
def test_mrc_tar_e_on_the_emulator(simbin, oracle, tmp_path, n, eps, tail):
    w = util.gauss_words(n, seed=n & 255)
    want = abs_round(w, f32_toward_zero(eps))
    src, z, back, er = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc", tmp_path / "e.mrc"
    src.write_bytes(w.tobytes() + tail)
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-e", repr(eps), "-t", "zip"])
    assert r.returncode == 0, r.stderr
    assert z.read_bytes() == oracle.compress(want.tobytes() + tail, 0)
    r = _run([simbin["mrc_tar"], "-i", str(z), "-o", str(back), "-t", "unzip", "-e", "5"])  # unzip ignores -e
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == want.tobytes()
    assert max_abs_error(w, want) <= float(f32_toward_zero(eps))
    r = _run([simbin["erasebytes"], "-i", str(src), "-o", str(er), "-e", repr(eps)])
    assert r.returncode == 0, r.stderr
    assert er.read_bytes() == want.tobytes()


def test_mrc_tar_e_over_several_batches_and_a_ragged_tail(simbin, oracle, tmp_path):
    """three chunks, one per batch, the last one partial: chunks past the first round their first 256 words too"""
    from test_host_sim import _several_batches_and_a_ragged_tail
    w = _several_batches_and_a_ragged_tail()
    eps = 0.05
    want = abs_round(w, f32_toward_zero(eps))
    src, z, back = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc"
    src.write_bytes(w.tobytes())
    env = {"MRCZ_BATCH_CHUNKS": "1"}
    assert _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-e", str(eps)], env).returncode == 0
    assert z.read_bytes() == oracle.compress(want.tobytes(), 0, threads=4)
    assert _run([simbin["mrc_tar"], "-i", str(z), "-o", str(back), "-t", "unzip"], env).returncode == 0
    assert back.read_bytes() == want.tobytes()


def test_mrc_tarx_e_on_the_emulator(simbin, oracle, tmp_path):
    ws = [util.gauss_words(50000, seed=31), util.poisson_words(40000, seed=32)]
    lst, outdir = tmp_path / "list.txt", tmp_path / "out"
    outdir.mkdir()
    names = []
    for i, w in enumerate(ws):
        p = tmp_path / f"f{i}.mrc"
        p.write_bytes(w.tobytes())
        names.append(p)
    lst.write_text("".join(f"{p}\n" for p in names))
    r = _run([simbin["mrc_tarx"], "-i", str(lst), "-t", "zip", "-o", str(outdir), "-n", "2", "-e", "0.5"])
    assert r.returncode == 0, r.stderr
    for p, w in zip(names, ws):
        z = outdir / (p.name + ".zip")
        assert z.read_bytes() == oracle.compress(abs_round(w, f32_toward_zero(0.5)).tobytes(), 0)


def test_excluded_combinations_and_bad_bounds_fail(simbin, tmp_path):
    src, z, lst = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "l.txt"
    src.write_bytes(util.gauss_words(1000).tobytes())
    lst.write_text(f"{src}\n")
    for extra in (["-e", "0.01", "-b", "8"], ["-e", "0.01", "-s", "int"], ["-e", "0"], ["-e", "-1"], ["-e", "nan"], ["-e", "inf"],
                  ["-e", "abc"], ["-e", "1e-50"]):
        r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-t", "zip"] + extra)
        assert r.returncode != 0 and "Usage" in r.stdout, extra
        r = _run([simbin["mrc_tarx"], "-i", str(lst), "-t", "zip", "-o", str(tmp_path)] + extra)
        assert r.returncode != 0 and "Usage" in r.stdout, extra
    for extra in (["-e", "0.01", "-b", "8"], ["-e", "0"], ["-e", "nan"]):
        assert _run([simbin["erasebytes"], "-i", str(src), "-o", str(z)] + extra).returncode != 0, extra
