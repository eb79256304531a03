"""CPU-only: the C-ABI shared library loads and exports every symbol include/mrcz_hip.h declares;
the host mirror refuses to work without it (no CPU fallback)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import util

HDR = os.path.join(util.ROOT, "include", "mrcz_hip.h")
LIB = os.path.join(util.ROOT, "datacompressionfloat_amd", "lib", "libmrcz_hip.so")
WORKERS = os.path.join(util.ROOT, "datacompressionfloat_amd", "lib", "libmrcz_workers.so")


def _declared():
    src = open(HDR).read()
    return sorted(set(re.findall(r"\b(mrcz_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(LIB):
        sys.path.insert(0, util.ROOT)
        import __graft_entry__ as g
        g.build()
    return LIB


def test_header_declares_expected_symbols():
    from datacompressionfloat_amd import _lib
    assert set(_lib.EXPORTS) <= set(_declared())


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built)
    for name in _declared():
        assert hasattr(lib, name), name


def test_library_is_gfx950_only(built):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", f"--input={built}"],
                         capture_output=True, text=True)
    if out.returncode == 0 and out.stdout.strip():
        targets = [t for t in out.stdout.split() if "amdgcn" in t]
        assert targets and all("gfx950" in t for t in targets), targets


def test_library_reads_no_tuning_environment(built):
    # the device library reads two environment variables: a diagnostic and a test knob.  Tuning choices are constants in the
    # source; experiments build another library and load it through MRCZ_LIB_PATH.
    names = set(m.decode() for m in re.findall(rb"MRCZ_[A-Z0-9_]+", open(built, "rb").read()))
    assert names <= {"MRCZ_TRACE", "MRCZ_SCRATCH_BYTES"}, sorted(names)


def test_host_library_reads_no_tuning_environment(built):
    # the host pipeline (run_compress / run_uncompress) reads a diagnostic, the batch size and the devices a file is dealt
    # to; its input, output and thread choices have one path each, not a switch.
    names = set(m.decode() for m in re.findall(rb"MRCZ_[A-Z0-9_]+", open(WORKERS, "rb").read()))
    assert names <= {"MRCZ_TRACE", "MRCZ_BATCH_CHUNKS", "MRCZ_DEVICES", "MRCZ_DEVICE_ALIAS"}, sorted(names)


def test_bound_is_pure_host_arithmetic(built):
    lib = ctypes.CDLL(built)
    lib.mrcz_records_bound.restype = ctypes.c_uint64
    lib.mrcz_records_bound.argtypes = [ctypes.c_uint64]
    assert lib.mrcz_records_bound(0) == 64
    assert lib.mrcz_records_bound(6291456) == 16 + 4 * 6291456 + 64
    assert lib.mrcz_records_bound(6291457) == 32 + 4 * 6291457 + 64


def test_no_gpu_means_loud_failure(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = ctypes.CDLL(built)
    ctx = ctypes.c_void_p()
    lib.mrcz_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_uint32]
    assert lib.mrcz_create(ctypes.byref(ctx), 0, 1) != 0  # MRCZ_EHIP: never a silent CPU path
    from datacompressionfloat_amd import MrcZipCodec, MrczError
    with pytest.raises(MrczError):
        MrcZipCodec(0)
