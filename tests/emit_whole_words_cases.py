"""Inputs shared by test_gpu_emit_whole_words.py and its emulator twin test_sim_emit_whole_words.py.

The compressor does not zero its output: every dword of a payload is stored in full once, or it is a boundary word that
k_clear_boundaries zeroes before the emit kernels OR into it.  The parity tests hand the codec a fresh (on the emulator:
zeroed) buffer, where a word that is neither stored nor cleared can pass by luck, so every case here is compressed into a
buffer pre-filled with PATTERN.  Each input is chosen for one kind of boundary."""
import numpy as np

import util

PATTERN = 0xA5
SLACK = 256          # bytes behind mrcz_records_bound() that the codec must not touch either


def random_words(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)


def long_code_words() -> np.ndarray:
    """four frequent byte values (2-bit codes) around a stretch of 250 rare ones (10..12-bit codes) that fills whole tiles: those
    tiles' bits exceed k_emit's staging buffer (the input of test_sim.py's staging-buffer test)"""
    rng = np.random.default_rng(5)
    common = lambda n: rng.integers(0, 4, n, dtype=np.uint64).astype(np.uint32)
    rare = (4 + rng.integers(0, 250, 5000, dtype=np.uint64)).astype(np.uint32)
    return np.concatenate([common(12000), rare, common(40000)])


# name -> (words, bits).  Built lazily: the large ones cost a second of numpy each.
SMALL = {}
for _b in (0, 8, 12, 23):     # ~9 coded blocks in the mantissa plane, ten segments: pair starts, block headers, END_BLOCK words
    SMALL[f"gauss300k_b{_b}"] = (lambda b=_b: (util.gauss_words(300000, seed=1234), b))
for _n in (1, 63, 64, 65, 4095, 4097, 100001):   # ragged tiles, one-word payloads (first word == last word)
    SMALL[f"gauss{_n}_b8"] = (lambda n=_n: (util.gauss_words(n, seed=n), 8))
SMALL["random200k_b0"] = lambda: (random_words(200000, 17), 0)                # stored blocks and RAW planes beside bit-aligned headers
SMALL["constant200k_b0"] = lambda: (np.full(200000, 0x41200000, np.uint32), 0)   # one block of long runs: parts without a symbol start
SMALL["stored_then_coded_b0"] = lambda: (np.concatenate([random_words(34000, 11), np.full(40000, 0x41200000, np.uint32)]), 0)
SMALL["long_codes_b0"] = lambda: (long_code_words(), 0)                       # the staging buffer's halving path

# one chunk + 1000 floats: payloads of adjacent planes and the second chunk's header share dwords
CHUNK_PLUS = lambda: (util.gauss_words(util.CHUNK + 1000, seed=1234), 8)


def check(got: np.ndarray, olen: int, ref_records: bytes, name):
    """got = the whole pre-filled output buffer after the call"""
    assert olen == len(ref_records), (name, olen, len(ref_records))
    rec = got[:olen]
    exp = np.frombuffer(ref_records, np.uint8)
    if not np.array_equal(rec, exp):
        bad = np.flatnonzero(rec != exp)
        raise AssertionError(f"{name}: {len(bad)} record bytes differ from the oracle, first at {bad[0]} of {olen}: "
                             f"got {rec[bad[0]]:#x}, expected {exp[bad[0]]:#x}")
    tail = got[olen:]
    assert len(tail) >= SLACK and bool(np.all(tail == PATTERN)), f"{name}: bytes behind the returned length were written"
