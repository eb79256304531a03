"""GPU: the selection kernels of erroranalysis (k_err_hist, k_err_collect in csrc/mrcz_tools.hip) through mrcz_err_hist and
mrcz_err_collect of libmrcz_hip.so, and bin/erroranalysis.  The expectations are those of tests/test_sim_erroranalysis.py: the
numpy statement tests/erroranalysis_ref.py over the catalogue tests/erroranalysis_cases.py, plus an array that takes every thread
through several grid-stride steps and one file of two batches at the shipped batch size whose lines are known by construction.
Every comparison is equality of bit patterns, counts or stdout text; nothing here needs oracle/_ref."""
import os
import subprocess

import numpy as np
import pytest

import erroranalysis_cases as cases
import erroranalysis_ref as ref
import util
from test_sim_erroranalysis import run_knobs, write_case

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "datacompressionfloat_amd", "bin", "erroranalysis")
KNOBS = ({}, {"MRCZ_ERR_BATCH": "4099"}, {"MRCZ_ERR_BATCH": "4099", "MRCZ_ERR_CAP": "64"})


@pytest.fixture(scope="module")
def abi():
    from datacompressionfloat_amd import _lib
    a = cases.Abi(_lib.load())
    yield a
    a.close()


@pytest.fixture(scope="module")
def grid():
    a, b, K = cases.grid_stride()
    assert len(a) == 3 * 2048 * 256 + 77
    return a, b, K


def collect_checks(abi, a, b, K):
    n, kth = len(a), cases.first_kth_key(a, b, K)
    for thr in (kth, 0, cases.INF, ref.NAN_KEY):
        for count_in in (0, 7):
            cases.check_collect(abi, a, b, thr, count_in=count_in, pieces=2 if n >= 3 else 1)
    assert cases.check_collect(abi, a, b, 0, base_index=(1 << 33) + 5) == n
    cases.check_collect(abi, a, b, 0, count_in=7, cap=7 + n // 2, pieces=2 if n >= 3 else 1)      # fewer slots than matches
    cases.check_collect(abi, a, b, 0, cap=n)                                                     # exactly as many
    cases.check_collect(abi, a, b, 0, cap=max(n - 1, 0))                                         # one too few
    cases.check_collect(abi, a, b, 0, count_in=9, cap=4)                                         # full before the call


@pytest.mark.parametrize("name", cases.NAMES)
def test_err_hist(abi, name):
    a, b, K = cases.points(name)
    cases.check_hist(abi, a, b, K, split_passes=(0, 1, 2))


@pytest.mark.parametrize("name", cases.NAMES)
def test_err_collect(abi, name):
    collect_checks(abi, *cases.points(name))


def test_err_hist_over_several_grid_stride_steps(abi, grid):
    a, b, _ = grid
    for K in (1, 100, 300, 100000):
        cases.check_hist(abi, a, b, K, split_passes=(0, 1, 2) if K == 100 else ())


def test_err_collect_over_several_grid_stride_steps(abi, grid):
    a, b, K = grid
    kth = cases.first_kth_key(a, b, K)
    many = int(cases.F(1.5 * 2.0 ** -11)[0])                 # about a fifth of the natural errors lies above it
    for thr in (kth, cases.INF, ref.NAN_KEY):
        cases.check_collect(abi, a, b, thr, count_in=7, base_index=(1 << 33) + 5, pieces=2)
    found = cases.check_collect(abi, a, b, many)
    assert 10000 < found < len(a) // 2
    cases.check_collect(abi, a, b, many, count_in=7, cap=1000, pieces=2)
    cases.check_collect(abi, a, b, many, cap=found - 1)


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_tool_prints_the_statements_lines(tmp_path, name):
    """as shipped, in ragged batches of 4099 floats, and in such batches with a candidate buffer of 64 records"""
    want = cases.expected_lines(name)
    for knobs, (rc, out, err) in zip(KNOBS, run_knobs(EXE, write_case(tmp_path, name), KNOBS, timeout=120)):
        assert rc == 0, (knobs, err)
        assert out == want, (knobs, out, want)


def test_two_batches_at_the_shipped_batch_size(tmp_path):
    """64 Mi + 70 001 points: the batch loop runs twice, the second batch is short, and after the wall at index 3 the range starts
    at 4, so its batches are [4, 64 Mi + 4) and the rest.  The lines are known by construction (cases.two_batches)."""
    a, b, want = cases.two_batches()
    assert len(a) == (64 << 20) + 70001 > cases.BATCH
    natural = ref.err_key(a[1 << 20: 2 << 20], b[1 << 20: 2 << 20])
    assert int(natural.max()) < int(cases.F(2.0 ** -11)[0])
    pa, pb = tmp_path / "a.bin", tmp_path / "b.bin"
    a.tofile(pa)
    b.tofile(pb)
    for k, pts in sorted(want.items()):
        r = subprocess.run([EXE, "-a", str(pa), "-b", str(pb), "-k", str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        expect = ref.print_points([p[0] for p in pts], [p[1] for p in pts])
        assert len(pts) == k and r.stdout == expect, (k, r.stdout, expect)
