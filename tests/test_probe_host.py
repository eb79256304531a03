"""CPU-only, no emulator: choose(), the pure-Python pick of a row of MrcZipCodec.sweep: the row of smallest container_bytes that
meets every constraint given, the earlier row on a tie, None when nothing is feasible."""
import math
import os

import pytest

import util

LIB = os.path.join(util.ROOT, "datacompressionfloat_amd", "lib", "libmrcz_hip.so")


@pytest.fixture(scope="module")
def choose():
    if not os.path.exists(LIB):           # importing the package needs its library (there is no CPU fallback)
        import sys
        sys.path.insert(0, util.ROOT)
        import __graft_entry__ as g
        g.build()
    from datacompressionfloat_amd import choose
    return choose


def row(tag, nbytes, max_err, rmse, psnr):
    return {"setting": tag, "container_bytes": nbytes, "max_err": max_err, "rmse": rmse, "psnr_db": psnr}


ROWS = [row(("bits", 0), 1000, 0.0, 0.0, math.inf),
        row(("bits", 8), 700, 0.001, 0.0004, 90.0),
        row(("bits", 12), 500, 0.02, 0.006, 66.0),
        row(("abs", 0.01), 500, 0.01, 0.005, 68.0),       # as small as the row before it, and later
        row(("bits", 16), 300, 0.3, 0.1, 42.0),
        row(("int",), 250, 0.5, 0.29, 33.0),
        row(("bits", 32), 40, 25.0, 10.4, 2.0)]


def test_no_constraint_gives_the_smallest(choose):
    assert choose(ROWS)["setting"] == ("bits", 32)
    assert choose(ROWS[:1]) is ROWS[0]


def test_single_constraints(choose):
    assert choose(ROWS, max_err=0.5)["setting"] == ("int",)
    assert choose(ROWS, max_err=0.49)["setting"] == ("bits", 16)
    assert choose(ROWS, max_err=0.0)["setting"] == ("bits", 0)               # a bound is met when equal
    assert choose(ROWS, max_rmse=0.0055)["setting"] == ("abs", 0.01)
    assert choose(ROWS, max_rmse=0.1)["setting"] == ("bits", 16)
    assert choose(ROWS, min_psnr=66.0)["setting"] == ("bits", 12)            # the tie in bytes goes to the earlier row
    assert choose(ROWS, min_psnr=67.0)["setting"] == ("abs", 0.01)
    assert choose(ROWS, min_psnr=1e9)["setting"] == ("bits", 0)              # inf meets any finite demand


def test_ties_go_to_the_earlier_row(choose):
    assert choose(ROWS, max_err=0.02)["setting"] == ("bits", 12)
    swapped = ROWS[:2] + [ROWS[3], ROWS[2]] + ROWS[4:]
    assert choose(swapped, max_err=0.02)["setting"] == ("abs", 0.01)
    assert choose(swapped, max_err=0.02) is swapped[2]                       # the row itself, not a copy


def test_combined_constraints(choose):
    assert choose(ROWS, max_err=0.5, max_rmse=0.2)["setting"] == ("bits", 16)
    assert choose(ROWS, max_err=0.02, max_rmse=0.0055)["setting"] == ("abs", 0.01)
    assert choose(ROWS, max_err=0.02, max_rmse=0.0055, min_psnr=80.0)["setting"] == ("bits", 8)
    assert choose(ROWS, max_err=1.0, min_psnr=40.0)["setting"] == ("bits", 16)


def test_nothing_feasible(choose):
    assert choose([]) is None
    assert choose(ROWS[1:], max_err=0.0) is None
    assert choose(ROWS[1:], min_psnr=91.0) is None
    assert choose(ROWS, max_err=0.5, min_psnr=50.0, max_rmse=0.00001)["setting"] == ("bits", 0)
    assert choose(ROWS[1:], max_err=0.5, min_psnr=50.0, max_rmse=0.00001) is None
    nan = [row(("bits", 4), 10, math.nan, math.nan, math.nan)]                # a row without finite points meets no bound ...
    assert choose(nan, max_err=1.0) is None and choose(nan, min_psnr=0.0) is None
    assert choose(nan) is nan[0]                                              # ... and any absence of bounds
