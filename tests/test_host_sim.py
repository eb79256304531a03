"""CPU-only: the C host (run_compress / run_uncompress pipeline of host/workers_gpu.c, the file adapters and both
front-ends) linked against the SIMT-emulator build of the codec instead of libmrcz_hip.so.  Exercises the reader /
caller / writer threads, the event protocol of the asynchronous C ABI, the per-plane summary table and the
container bytes on inputs small enough for the emulator -- before any GPU minute is spent on them."""
import os
import subprocess

import numpy as np
import pytest

import util

HOST = os.path.join(util.ROOT, "datacompressionfloat_amd", "host")


@pytest.fixture(scope="module")
def simbin(tmp_path_factory):
    util.load_sim()  # builds tests/sim/libmrcz_sim.so
    d = tmp_path_factory.mktemp("hostsim")
    out = {}
    exe = d / "erroranalysis"
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-o", str(exe), os.path.join(HOST, "erroranalysis.c"),
                           "-L" + util.SIM_DIR, "-lmrcz_sim", "-lpthread", "-lm", "-lstdc++", "-Wl,-rpath," + util.SIM_DIR])
    out["erroranalysis"] = str(exe)
    for main in ("mrc_tar", "mrc_tarx"):
        exe = d / main
        subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-o", str(exe), os.path.join(HOST, main + ".c"),
                               os.path.join(HOST, "workers_gpu.c"), os.path.join(HOST, "common_gpu.c"), os.path.join(HOST, "adapt_gpu.c"),
                               "-L" + util.SIM_DIR, "-lmrcz_sim", "-lpthread", "-lm", "-lstdc++", "-Wl,-rpath," + util.SIM_DIR])
        out[main] = str(exe)
    return out


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=e)


@pytest.mark.parametrize("n,bits,tail", [(100, 0, b""), (70001, 8, b"xyz"), (300000, 12, b"")])
def test_mrc_tar_on_the_emulator(simbin, oracle, tmp_path, n, bits, tail):
    w = util.gauss_words(n, seed=n & 255)
    src, z, back = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc"
    src.write_bytes(w.tobytes() + tail)
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-b", str(bits), "-t", "zip"])
    assert r.returncode == 0, r.stderr
    assert z.read_bytes() == oracle.compress(w.tobytes() + tail, bits)
    assert "Whole File" in r.stdout and "Compression Summary Result Information" in r.stdout      # print_result, zip.c:401-466
    r = _run([simbin["mrc_tar"], "-i", str(z), "-o", str(back), "-t", "unzip"])
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == util.erase_expected(w, bits).tobytes()
    assert "Decompress Result Info Information" in r.stdout


def _run_through_fifos(args, feed=(), drain=(), env=None):
    """`args` with `cat` feeding each (file, fifo) of `feed` and draining each (fifo, file) of `drain`.  Every process has a
    timeout: a FIFO whose other end never opens fails the test instead of hanging it."""
    cats = [subprocess.Popen(["sh", "-c", 'exec cat "$0" > "$1"', str(src), str(fifo)]) for src, fifo in feed]
    cats += [subprocess.Popen(["sh", "-c", 'exec cat "$0" > "$1"', str(fifo), str(dst)]) for fifo, dst in drain]
    try:
        r = _run(args, env)
        for c in cats:
            assert c.wait(timeout=60) == 0
        return r
    finally:
        for c in cats:
            if c.poll() is None:
                c.kill()
                c.wait()


def _several_batches_and_a_ragged_tail():
    """three chunks (one per batch with MRCZ_BATCH_CHUNKS=1), the last one partial; zero planes with noisy stretches keep
    the emulator fast"""
    n = 2 * util.CHUNK + 12345
    w = np.zeros(n, np.uint32)
    w[:256] = util.kat_words(256)
    for c in range(3):
        a = c * util.CHUNK + 1000 * (c + 1)
        w[a: a + 3000] = util.gauss_words(3000, seed=40 + c, header=False)
    return w


def test_fallbacks_for_pipes(simbin, oracle, tmp_path):
    """Inputs that cannot be mapped are read with fread, outputs that cannot seek are written in order with fwrite: a
    container written into a FIFO, then decoded from a FIFO into a FIFO, over several batches of several output slices."""
    w = _several_batches_and_a_ragged_tail()
    data = w.tobytes() + b"xyz"
    src, z, back = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc"
    src.write_bytes(data)
    fin, fout = tmp_path / "in.fifo", tmp_path / "out.fifo"
    os.mkfifo(fin)
    os.mkfifo(fout)
    env = {"MRCZ_BATCH_CHUNKS": "1"}
    r = _run_through_fifos([simbin["mrc_tar"], "-i", str(src), "-o", str(fout), "-b", "8", "-t", "zip"], drain=[(fout, z)], env=env)
    assert r.returncode == 0, r.stderr
    assert "Compression Summary Result Information" in r.stdout                # the tables go to stdout, not into the data
    assert z.read_bytes() == oracle.compress(data, 8, threads=3)
    r = _run_through_fifos([simbin["mrc_tar"], "-i", str(fin), "-o", str(fout), "-t", "unzip"], feed=[(z, fin)], drain=[(fout, back)], env=env)
    assert r.returncode == 0, r.stderr
    assert "Decompress Result Info Information" in r.stdout
    assert back.read_bytes() == util.erase_expected(w, 8).tobytes()


def test_empty_and_tiny_inputs(simbin, tmp_path):
    src, z = tmp_path / "e.mrc", tmp_path / "e.zip"
    src.write_bytes(b"abc")                                       # fewer than 4 bytes: nothing is written (workers.c:757)
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-t", "zip"])
    assert r.returncode == 0 and z.read_bytes() == b""


def test_mrc_tarx_threads_share_one_engine(simbin, oracle, tmp_path):
    srcdir, zdir, udir = tmp_path / "s", tmp_path / "z", tmp_path / "u"
    for d in (srcdir, zdir, udir):
        d.mkdir()
    names, datas = [], {}
    for i, n in enumerate((5000, 40000, 257, 90000)):
        p = srcdir / f"f{i}.mrc"
        w = util.poisson_words(n, seed=i)
        p.write_bytes(w.tobytes())
        names.append(str(p))
        datas[f"f{i}"] = w
    lst = tmp_path / "l.txt"
    lst.write_text("\n".join(names) + "\n")
    r = _run([simbin["mrc_tarx"], "-i", str(lst), "-t", "zip", "-o", str(zdir), "-b", "4", "-n", "3"])
    assert r.returncode == 0, r.stderr
    zs = []
    for stem, w in datas.items():
        z = zdir / f"{stem}.mrc.zip"
        assert z.read_bytes() == oracle.compress(w.tobytes(), 4), stem
        zs.append(str(z))
    lst2 = tmp_path / "z.txt"
    lst2.write_text("\n".join(zs) + "\n")
    r = _run([simbin["mrc_tarx"], "-i", str(lst2), "-t", "unzip", "-o", str(udir), "-n", "2"])
    assert r.returncode == 0, r.stderr
    for stem, w in datas.items():
        assert (udir / f"{stem}.mrc").read_bytes() == util.erase_expected(w, 4).tobytes()
    # throughput mode: the codec runs, nothing is written (workers.c:39)
    tdir = tmp_path / "t"
    tdir.mkdir()
    r = _run([simbin["mrc_tarx"], "-i", str(lst), "-t", "zip", "-o", str(tdir), "-n", "2", "-d", "1"])
    assert r.returncode == 0 and all(os.path.getsize(tdir / f"{s}.mrc.zip") == 0 for s in datas)


def test_one_file_dealt_over_two_devices(simbin, oracle, tmp_path):
    """SURVEY 8(e) in the C host: the batches of ONE file are dealt round-robin to the visible devices (here two emulated
    ones, one chunk per batch), every device codes its chunk ranges on its own engine, the writer threads put the records back
    in file order: same container bytes as the oracle, and the same decoded file through the two-device decoder."""
    n = 2 * util.CHUNK + 30000                       # three chunks: device 0 gets chunks 0 and 2, device 1 chunk 1
    w = np.zeros(n, np.uint32)                       # all-zero planes keep the emulator fast; the header words and a noisy tail differ
    w[:256] = util.kat_words(256)
    w[util.CHUNK - 5000: util.CHUNK + 5000] = util.gauss_words(10000, seed=8, header=False)
    w[-20000:] = util.poisson_words(20000, seed=9)[-20000:]
    src, z, back = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc"
    src.write_bytes(w.tobytes())
    env = {"SIM_DEVICES": "2", "MRCZ_BATCH_CHUNKS": "1", "MRCZ_TRACE": "1"}
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip", "-G", "0"], env=env)   # -G 0: all visible devices
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("mrcz_create") == 2, r.stderr          # two engines were brought up
    ref = oracle.compress(w.tobytes(), 8, threads=3)
    assert z.read_bytes() == ref
    r = _run([simbin["mrc_tar"], "-i", str(z), "-o", str(back), "-t", "unzip", "-G", "2"], env=env)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == util.erase_expected(w, 8).tobytes()
    # one device only (the default, several devices are opt-in): the same bytes
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip"], env=env)
    assert r.returncode == 0 and r.stderr.count("mrcz_create") == 1 and z.read_bytes() == ref


def test_four_devices_and_a_short_last_batch(simbin, oracle, tmp_path):
    """Four emulated devices, one chunk per batch, five chunks: the batches wrap around the devices (device 0 codes batches 0
    and 4 in its two buffers), the last batch is a partial chunk, and the records come back in file order."""
    n = 4 * util.CHUNK + 4097
    w = np.zeros(n, np.uint32)
    w[:256] = util.kat_words(256)
    for c in range(5):                               # a noisy stretch in every chunk so that the five records differ
        a = c * util.CHUNK + 300 * (c + 1)
        m = min(3000, n - a)
        w[a: a + m] = util.gauss_words(3000, seed=30 + c, header=False)[:m]
    src, z, back = tmp_path / "in.mrc", tmp_path / "o.zip", tmp_path / "b.mrc"
    src.write_bytes(w.tobytes())
    env = {"SIM_DEVICES": "4", "MRCZ_BATCH_CHUNKS": "1", "MRCZ_TRACE": "1"}
    r = _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip", "-G", "4"], env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("mrcz_create") == 4, r.stderr
    ref = oracle.compress(w.tobytes(), 8, threads=5)
    assert z.read_bytes() == ref
    r = _run([simbin["mrc_tar"], "-i", str(z), "-o", str(back), "-t", "unzip", "-G", "4"], env=env)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == util.erase_expected(w, 8).tobytes()


def _damaged_containers(z: bytes):
    """a container cut inside its second chunk header / inside a payload, one whose first deflate stream is garbage, and one
    whose chunk header announces more bytes than four RAW planes can have"""
    h = np.frombuffer(z[17:33], "<u4")
    first_len = int(h[0] & 0x7fffffff)
    garbage = bytearray(z)
    garbage[33: 33 + min(first_len, 64)] = bytes((37 * i + 11) & 0xff for i in range(min(first_len, 64)))
    huge = bytearray(z)
    huge[17:21] = (0x7fffffff).to_bytes(4, "little")
    return {"cut in a chunk header": z[:17 + 7], "cut in a payload": z[: len(z) - len(z) // 3], "garbage deflate stream": bytes(garbage),
            "record longer than RAW planes": bytes(huge)}


def test_damaged_containers_end_with_an_error_status_not_a_signal(simbin, tmp_path):
    """The reference leaves with exit(-1) on what it cannot handle (workers.c:708-712); here the error is raised by a pipeline
    thread while the others still use the session: the process must end with a plain non-zero status (no SIGSEGV / SIGABRT
    out of the exit handlers), for mrc_tar and for a worker thread of mrc_tarx."""
    w = util.gauss_words(60000, seed=5)
    src, z = tmp_path / "in.mrc", tmp_path / "o.zip"
    src.write_bytes(w.tobytes())
    assert _run([simbin["mrc_tar"], "-i", str(src), "-o", str(z), "-b", "8", "-t", "zip"]).returncode == 0
    good = z.read_bytes()
    for what, bad in _damaged_containers(good).items():
        b = tmp_path / "bad.zip"
        b.write_bytes(bad)
        r = _run([simbin["mrc_tar"], "-i", str(b), "-o", str(tmp_path / "x.mrc"), "-t", "unzip"])
        assert r.returncode > 0, (what, r.returncode, r.stderr)          # > 0: an exit status; < 0 would be a signal
        assert "ERROR" in r.stderr, (what, r.stderr)
        lst = tmp_path / "l.txt"
        lst.write_text(str(b) + "\n")
        r = _run([simbin["mrc_tarx"], "-i", str(lst), "-t", "unzip", "-o", str(tmp_path), "-n", "2"])
        assert r.returncode > 0, (what, r.returncode, r.stderr)
    # two worker threads that both fail to open their output (directory missing, adapt.c:34-44): exit status, not a crash
    two = tmp_path / "two.txt"
    two.write_text(str(src) + "\n" + str(src) + "\n")
    r = _run([simbin["mrc_tarx"], "-i", str(two), "-t", "zip", "-o", str(tmp_path / "no" / "such" / "dir"), "-n", "2"])
    assert r.returncode > 0 and "fail open" in r.stderr, (r.returncode, r.stderr)
    # the orderly path still releases its sessions: one good run with the full teardown
    r = _run([simbin["mrc_tar"], "-i", str(z), "-o", str(tmp_path / "ok.mrc"), "-t", "unzip"], env={"MRCZ_FULL_TEARDOWN": "1"})
    assert r.returncode == 0 and (tmp_path / "ok.mrc").read_bytes() == util.erase_expected(w, 8).tobytes()


@pytest.mark.skipif(util.ref_binary("erroranalysis_c") is None, reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("k,nanat", [(1, 777), (2, 777), (7, 777), (5, 2), (6, None), (3, 0)])
def test_erroranalysis_matches_the_reference_tool(simbin, tmp_path, k, nanat):
    """erroranalysis (src/tool/erroranalysis.c) with the selection on the device: same lines on stdout as
    the reference's tool -- masked data (many equal errors: the relative-error and first-point tie rules decide), a few
    planted outliers, a NaN, files of different lengths."""
    ref = util.ref_binary("erroranalysis_c")
    w = util.gauss_words(50000, seed=k)
    dec = util.erase_expected(w, 14)
    f = dec.view(np.float32)
    f[1234] += 3.5
    f[40000] -= 3.5
    if nanat is not None:
        f[nanat] = np.float32(np.nan)          # a NaN difference is a wall in the reference's bubble passes
        f[nanat + 5000] = np.float32(np.nan)
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    a.write_bytes(w.tobytes())
    b.write_bytes(dec.tobytes()[: 4 * 49000])           # the decoded file is shorter: the tools stop there
    mine = _run([simbin["erroranalysis"], "-a", str(a), "-b", str(b), "-k", str(k)])
    theirs = _run([ref, "-a", str(a), "-b", str(b), "-k", str(k)])
    assert mine.returncode == 0 and theirs.returncode == 0, (mine.stderr, theirs.stderr)
    assert mine.stdout == theirs.stdout, (mine.stdout, theirs.stdout)
    assert len(mine.stdout.splitlines()) == k


@pytest.mark.skipif(util.ref_binary("erroranalysis_c") is None, reason="oracle/_ref not built (needs /root/reference)")
def test_erroranalysis_with_more_ties_and_nans_than_the_candidate_buffer(simbin, tmp_path):
    """The reference's tool takes any number of NaN differences and of points that tie for the top error (two identical
    files: every point ties at 0).  With the candidate buffer forced down to 64 records both must go through its growth
    path and still print the reference's lines."""
    ref = util.ref_binary("erroranalysis_c")
    w = util.gauss_words(20000, seed=3)
    a, b, c = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "c.bin"
    a.write_bytes(w.tobytes())
    b.write_bytes(w.tobytes())                              # identical: 20000 points tie
    d = util.erase_expected(w, 12)
    f = d.view(np.float32)
    f[500:20000:97] = np.float32(np.nan)                    # 202 NaN walls
    c.write_bytes(d.tobytes())
    for other, k in ((b, 4), (c, 6)):
        mine = _run([simbin["erroranalysis"], "-a", str(a), "-b", str(other), "-k", str(k)], env={"MRCZ_ERR_CAP": "64"})
        theirs = _run([ref, "-a", str(a), "-b", str(other), "-k", str(k)])
        assert mine.returncode == 0 and theirs.returncode == 0, (mine.stderr, theirs.stderr)
        assert mine.stdout == theirs.stdout, (mine.stdout, theirs.stdout)
