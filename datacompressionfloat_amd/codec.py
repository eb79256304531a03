"""Host mirror of the reference's chunk-codec seam for Python callers.

Mirrors /root/reference/src/include/workers.h:30-31 (run_compress / run_uncompress) and the file
header I/O of src/core/common.c:117-148 with the same argument meaning: `bits` is bitsToMask
(0..32), containers start with the 17-byte header, decode output is 4*floor(fsz/4) bytes.
Device memory comes from torch; all arithmetic happens in libmrcz_hip.so.
"""
import ctypes
import io
import os
import struct

import numpy as np
import torch

from . import _lib
from ._lib import (DIGEST_ABS, DIGEST_INT8, DIGEST_MASK, DIGEST_NONE, PROBE_ABS, PROBE_INT8, PROBE_MASK, TOP_F32, TOP_THINNED, TOP_U16,
                   MrczBinGeom, MrczBoxGeom, MrczCompare, MrczDigest)

CHUNK_FLOATS = 6 * 1048576  # src/include/constant.h:25
FILE_HEADER_BYTES = 17      # src/core/common.c:137-148
MRC_HEADER_BYTES = 1024     # MRC2014: the fixed header before the extended header (nsymbt bytes) and the data

_LIB = _lib.load()  # raises MrczLibraryMissing: no CPU fallback


class MrczError(RuntimeError):
    pass


_FLT_MAX = float(np.finfo(np.float32).max)


def abs_bound(eps) -> float:
    """An absolute-error bound as the codec takes it: float32, rounded toward zero so that the bound also holds for the value
    given.  Raises MrczError unless it is finite and > 0."""
    e = float(eps)
    if not (np.isfinite(e) and e > 0):
        raise MrczError("absolute error bound must be finite and > 0")
    f = np.float32(min(e, _FLT_MAX))
    if float(f) > e:
        f = np.nextafter(f, np.float32(0))
    if not f > 0:
        raise MrczError("absolute error bound below the smallest float32")
    return float(f)


def pack_file_header(fsz: int) -> bytes:
    """write_mrczip_header (src/core/common.c:137-148): u64 fsz, u32 chk, i8 type, i8 ztypes[4]."""
    return struct.pack("<QIb4b", fsz, CHUNK_FLOATS, 0, 0, 0, 0, 0)


def unpack_file_header(buf: bytes):
    """read_mrczip_header (src/core/common.c:117-134) -> (fsz, chk, type, ztypes)."""
    if len(buf) < FILE_HEADER_BYTES:
        raise MrczError("container shorter than the 17-byte header")
    fsz, chk, typ, z0, z1, z2, z3 = struct.unpack("<QIb4b", bytes(buf[:FILE_HEADER_BYTES]))
    return fsz, chk, typ, (z0, z1, z2, z3)


def crc32_combine(crc_a: int, crc_b: int, nbytes_b: int) -> int:
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B) (mrcz_crc32_combine: host arithmetic, no GPU)"""
    return int(_LIB.mrcz_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, nbytes_b))


SIDECAR_MAGIC = "mrcz-digest crc32 1"


def format_sidecar(nfl: int, chk: int, mode: str, file_crc: int, chunk_crcs) -> str:
    """the digest sidecar of a container: text, one line per chunk"""
    if mode not in ("float", "int"):
        raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
    lines = [SIDECAR_MAGIC, f"words {nfl} chunk {chk} chunks {len(chunk_crcs)} mode {mode}", f"file {file_crc & 0xFFFFFFFF:08x}"]
    lines += [f"{c} {v & 0xFFFFFFFF:08x}" for c, v in enumerate(chunk_crcs)]
    return "\n".join(lines) + "\n"


def parse_sidecar(text) -> dict:
    """{"words", "chunk", "chunks", "mode", "file", "crcs"} of a sidecar; MrczError for anything that is not one"""
    if isinstance(text, (bytes, bytearray)):
        try:
            text = bytes(text).decode("ascii")
        except UnicodeDecodeError:
            raise MrczError("not a digest sidecar: not text")
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    hexw = lambda t: len(t) == 8 and all(ch in "0123456789abcdef" for ch in t)
    num = lambda t: t.isascii() and t.isdigit() and len(t) <= 20
    if len(lines) < 3 or lines[0] != SIDECAR_MAGIC:
        raise MrczError("not a digest sidecar: first line is not '" + SIDECAR_MAGIC + "'")
    t = lines[1].split(" ")
    if len(t) != 8 or t[0::2] != ["words", "chunk", "chunks", "mode"] or not all(num(v) for v in t[1:7:2]) or t[7] not in ("float", "int"):
        raise MrczError("damaged digest sidecar: line 2")
    nfl, chk, nch = int(t[1]), int(t[3]), int(t[5])
    if chk == 0 or nch != (nfl + chk - 1) // chk:
        raise MrczError("damaged digest sidecar: words, chunk and chunks disagree")
    f = lines[2].split(" ")
    if len(f) != 2 or f[0] != "file" or not hexw(f[1]):
        raise MrczError("damaged digest sidecar: line 3")
    if len(lines) != 3 + nch:
        raise MrczError(f"damaged digest sidecar: {len(lines) - 3} chunk lines for {nch} chunks")
    crcs = []
    for c, line in enumerate(lines[3:]):
        p = line.split(" ")
        if len(p) != 2 or p[0] != str(c) or not hexw(p[1]):
            raise MrczError(f"damaged digest sidecar: chunk line {c}")
        crcs.append(int(p[1], 16))
    return {"words": nfl, "chunk": chk, "chunks": nch, "mode": t[7], "file": int(f[1], 16), "crcs": crcs}


def choose(rows, max_err=None, max_rmse=None, min_psnr=None):
    """the row of MrcZipCodec.sweep with the smallest container_bytes among those that meet every constraint given (max_err >=
    row max_err, max_rmse >= row rmse, min_psnr <= row psnr_db); the earlier row on a tie; None when no row meets them.  Pure
    host arithmetic."""
    best = None
    for r in rows:
        if max_err is not None and not r["max_err"] <= max_err:
            continue
        if max_rmse is not None and not r["rmse"] <= max_rmse:
            continue
        if min_psnr is not None and not r["psnr_db"] >= min_psnr:
            continue
        if best is None or r["container_bytes"] < best["container_bytes"]:
            best = r
    return best


def read_thinned_records(f, nfl: int, chk: int, keep: int, first_chunk: int = 0, nchunks: int = None, start: int = None):
    """the thinned records of chunks [first_chunk, first_chunk + nchunks) of the container open as binary file `f`:
    per chunk its 16-byte header and, behind it, the payloads of its `keep` top byte planes, which are the tail of the record
    (mrcz_record_top_span).  Host arithmetic and reads only, no GPU: the headers are read 16 bytes at a time, the kept payloads
    with one read per chunk, and no byte of a dropped payload is read.  `start` = the byte offset in `f` of chunk first_chunk's
    record when the caller knows it (else the headers of the chunks before are walked).  Returns (bytes, offset of the record of
    chunk first_chunk + nchunks)."""
    nch = (nfl + chk - 1) // chk
    if nchunks is None:
        nchunks = nch - first_chunk
    if keep not in (2, 3) or first_chunk < 0 or nchunks < 0 or first_chunk + nchunks > nch:
        raise MrczError("keep must be 2 or 3 and the chunks inside the file")
    size, skip, kept = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()

    def header(c, off):
        f.seek(off)
        h = f.read(16)
        if len(h) < 16 or _LIB.mrcz_record_top_span(h, min(chk, nfl - c * chk), keep, ctypes.byref(skip), ctypes.byref(kept)) != 0:
            raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
        return h

    off = FILE_HEADER_BYTES if start is None else start
    for c in range(first_chunk if start is None else 0):
        header(c, off)
        off += skip.value + kept.value
    out = bytearray()
    for c in range(first_chunk, first_chunk + nchunks):
        out += header(c, off)
        f.seek(off + skip.value)
        body = f.read(kept.value)
        if len(body) != kept.value:
            raise MrczError("truncated container: the records end early")
        out += body
        off += skip.value + kept.value
    return bytes(out), off


class MrcZipCodec:
    """One codec context (HIP stream + workspace) on one GPU."""

    def __init__(self, device=0, max_batch_chunks=64):
        if not torch.cuda.is_available():
            raise MrczError("no HIP device visible: the codec has no CPU path")
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        self.max_batch_chunks = max_batch_chunks
        self._ctx = ctypes.c_void_p()
        rc = _LIB.mrcz_create(ctypes.byref(self._ctx), self.device.index, max_batch_chunks)
        if rc != 0:
            raise MrczError(f"mrcz_create failed ({rc})")

    def close(self):
        if self._ctx:
            _LIB.mrcz_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what, rc):
        msg = _LIB.mrcz_last_error(self._ctx)
        return MrczError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_timing(self, on: bool):
        _LIB.mrcz_set_timing(self._ctx, 1 if on else 0)

    def last_timings(self):
        names = (ctypes.c_char_p * 32)()
        ms = (ctypes.c_float * 32)()
        n = _LIB.mrcz_last_timings(self._ctx, names, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    def last_fallbacks(self) -> int:
        """streams of the last uncompress call that needed the sequential general-distance decoder"""
        return int(_LIB.mrcz_debug_fallbacks(self._ctx))

    def last_chain_fallbacks(self) -> int:
        """streams of the last uncompress call whose block chain did not close in parallel and that were decoded block after
        block instead (static blocks, headers outside the candidate pattern, more blocks or segments than the per-stream
        limits; includes the streams counted by last_fallbacks)"""
        return int(_LIB.mrcz_debug_chain_fallbacks(self._ctx))

    @staticmethod
    def records_bound(nfloats: int) -> int:
        return int(_LIB.mrcz_records_bound(nfloats))

    # ---- device-resident API (what bench.py times) ----
    def compress_device(self, words: torch.Tensor, bits: int, first_chunk: int = 0, out: torch.Tensor = None, int_mode: bool = False,
                        abs_err=None):
        """words: cuda tensor of 32-bit elements (int32/float32/uint32 view), chunk-aligned start.
        int_mode = the reference's "-s int" (src/core/workers.c:125-175): bits is ignored.
        abs_err = eps: absolute-error mode (mrcz_compress_chunks_abs), every decoded float within eps of the original; needs
        bits == 0 and no int_mode.
        Returns (records uint8 cuda tensor view, plane_bytes[4])."""
        assert words.is_cuda and words.is_contiguous() and words.element_size() == 4
        if abs_err is not None:
            if bits != 0 or int_mode:
                raise MrczError("abs_err excludes bits != 0 and the int mode")
            abs_err = abs_bound(abs_err)
        n = words.numel()
        cap = self.records_bound(n)
        if out is None:
            out = torch.empty(cap, dtype=torch.uint8, device=words.device)
        assert out.is_cuda and out.numel() >= cap
        torch.cuda.current_stream(words.device).synchronize()
        olen = ctypes.c_uint64()
        planes = (ctypes.c_uint64 * 4)()
        if int_mode:
            rc = _LIB.mrcz_compress_chunks_int8(self._ctx, words.data_ptr(), n, first_chunk, out.data_ptr(), out.numel(),
                                                ctypes.byref(olen), planes)
        elif abs_err is not None:
            rc = _LIB.mrcz_compress_chunks_abs(self._ctx, words.data_ptr(), n, first_chunk, abs_err, out.data_ptr(), out.numel(),
                                               ctypes.byref(olen), planes)
        else:
            rc = _LIB.mrcz_compress_chunks(self._ctx, words.data_ptr(), n, first_chunk, bits, out.data_ptr(), out.numel(),
                                           ctypes.byref(olen), planes)
        if rc != 0:
            raise self._err("mrcz_compress_chunks", rc)
        return out[: olen.value], [int(p) for p in planes]

    def uncompress_device(self, records: torch.Tensor, nfloats: int, chk: int = CHUNK_FLOATS, out: torch.Tensor = None,
                          int_mode: bool = False, first_chunk: int = 0):
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        if out is None:
            out = torch.empty(nfloats, dtype=torch.int32, device=records.device)
        assert out.is_cuda and out.numel() >= nfloats and out.element_size() == 4
        torch.cuda.current_stream(records.device).synchronize()
        consumed = ctypes.c_uint64()
        if int_mode:
            rc = _LIB.mrcz_uncompress_chunks_int8(self._ctx, records.data_ptr(), records.numel(), nfloats, chk, first_chunk, out.data_ptr(),
                                                  ctypes.byref(consumed))
        else:
            rc = _LIB.mrcz_uncompress_chunks(self._ctx, records.data_ptr(), records.numel(), nfloats, chk, out.data_ptr(),
                                             ctypes.byref(consumed))
        if rc != 0:
            raise self._err("mrcz_uncompress_chunks", rc)
        return out[:nfloats], int(consumed.value)

    def uncompress_range_device(self, records: torch.Tensor, nfloats_file: int, w0: int, w1: int, chk: int = CHUNK_FLOATS,
                                first_chunk: int = 0, out: torch.Tensor = None, int_mode: bool = False):
        """words [w0, w1) of a file of nfloats_file floats.  `records` (cuda uint8) = the chunk records of chunks first_chunk,
        first_chunk + 1, ... (first_chunk <= w0 // chk; records before the window's first chunk are only walked).  Only the
        chunks that cover the window are decoded.  Returns (words int32 cuda tensor, record bytes consumed)."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        n = w1 - w0
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.int32, device=records.device)
        assert out.is_cuda and out.numel() >= n and out.element_size() == 4
        torch.cuda.current_stream(records.device).synchronize()
        consumed = ctypes.c_uint64()
        rc = _LIB.mrcz_uncompress_range(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, w0, w1,
                                        out.data_ptr(), 1 if int_mode else 0, ctypes.byref(consumed))
        if rc != 0:
            raise self._err("mrcz_uncompress_range", rc)
        return out[:n], int(consumed.value)

    def uncompress_top_device(self, records: torch.Tensor, nfloats_file: int, keep: int = 2, dtype=torch.bfloat16, first_chunk: int = 0,
                              nchunks: int = None, thinned: bool = False, out: torch.Tensor = None, chk: int = CHUNK_FLOATS):
        """top-planes decode (mrcz_uncompress_top): the words of chunks [first_chunk, first_chunk + nchunks) of a file of
        nfloats_file floats (default: every chunk from first_chunk on) with only their `keep` (2 or 3) most significant byte
        planes; the low planes are neither read nor decoded.  `records` (cuda uint8) = the ordinary records of those chunks, or
        with thinned=True their thinned records (read_thinned_records).  dtype torch.float32: every word & (0xFFFFFFFF <<
        8 (4 - keep)); torch.bfloat16 (keep 2 only): the same value in two bytes.  This is TRUNCATION toward zero, not the
        round-to-nearest of Tensor.to(torch.bfloat16); NaN payload bits in the dropped planes are lost (a NaN whose only set
        mantissa bits were there becomes +-Inf); file words 0..255 (the MRC header) are truncated like the rest.  Returns a
        1-D cuda tensor of that dtype (`out`, 16-byte aligned, or allocated)."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        if dtype not in (torch.bfloat16, torch.float32):
            raise MrczError("dtype must be torch.bfloat16 or torch.float32")
        if keep not in (2, 3) or (dtype == torch.bfloat16 and keep != 2):
            raise MrczError("keep must be 2 or 3, and torch.bfloat16 holds two planes: keep == 2")
        if nchunks is None:
            nchunks = max((nfloats_file + chk - 1) // chk - first_chunk, 0)
        n = max(min(nchunks * chk, nfloats_file - first_chunk * chk), 0)
        if out is None:
            out = torch.empty(max(n, 1), dtype=dtype, device=records.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == dtype and out.numel() >= n
        torch.cuda.current_stream(records.device).synchronize()
        flags = (TOP_U16 if dtype == torch.bfloat16 else TOP_F32) | (TOP_THINNED if thinned else 0)
        consumed = ctypes.c_uint64()
        rc = _LIB.mrcz_uncompress_top(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, nchunks, keep, flags,
                                      out.data_ptr(), ctypes.byref(consumed))
        if rc != 0:
            raise self._err("mrcz_uncompress_top", rc)
        return out.reshape(-1)[:n]

    def uncompress_boxes_device(self, records: torch.Tensor, nfloats_file: int, geom: MrczBoxGeom, origins, first_chunk: int = 0,
                                nchunks: int = None, out: torch.Tensor = None, int_mode: bool = False, chk: int = CHUNK_FLOATS):
        """box decode (mrcz_uncompress_boxes): `records` (cuda uint8) = the chunk records of chunks [first_chunk, first_chunk +
        nchunks) of a file of nfloats_file floats (default: every chunk from first_chunk on); `origins` = (N, 3) box corners
        x, y, z.  Writes the box voxels that lie in those chunks and every out-of-volume voxel (geom.fill_bits) into `out`, an
        (N, bz, by, bx) int32 cuda tensor (allocated when None); other voxels are left as they are.  Only the chunks a box
        touches are decoded.  Returns (out, chunks decoded)."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        org = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1, 3))
        n = len(org)
        if nchunks is None:
            nchunks = max((nfloats_file + chk - 1) // chk - first_chunk, 0)
        shape = (n, geom.bz, geom.by, geom.bx)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=records.device)
        assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= n * geom.bz * geom.by * geom.bx
        torch.cuda.current_stream(records.device).synchronize()
        decoded = ctypes.c_uint64()
        rc = _LIB.mrcz_uncompress_boxes(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, nchunks,
                                        ctypes.byref(geom), org.ctypes.data, n, out.data_ptr(), 1 if int_mode else 0,
                                        ctypes.byref(decoded))
        if rc != 0:
            raise self._err("mrcz_uncompress_boxes", rc)
        return out, int(decoded.value)

    def uncompress_binned_device(self, records: torch.Tensor, nfloats_file: int, geom: MrczBinGeom, acc: torch.Tensor, first_chunk: int = 0,
                                 nchunks: int = None, int_mode: bool = False, chk: int = CHUNK_FLOATS):
        """binned decode, one step (mrcz_uncompress_binned): `records` (cuda uint8) = the chunk records of chunks [first_chunk,
        first_chunk + nchunks) of a file of nfloats_file floats (default: every chunk from first_chunk on).  Folds the voxels of
        the chunks of mrcz_bin_chunks' [c0, c1) among them into `acc`, an (mz, my, mx) float64 cuda tensor of partial sums (no
        zeroing needed); the other chunks are only walked.  Steps cover [c0, c1) in increasing chunk order, each chunk once;
        then binned_finish_device.  Returns chunks decoded."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        nbins = (geom.nz // geom.fz) * (geom.ny // geom.fy) * (geom.nx // geom.fx) if min(geom.fx, geom.fy, geom.fz) else 0
        assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= nbins
        if nchunks is None:
            nchunks = max((nfloats_file + chk - 1) // chk - first_chunk, 0)
        torch.cuda.current_stream(records.device).synchronize()
        decoded = ctypes.c_uint64()
        rc = _LIB.mrcz_uncompress_binned(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, nchunks,
                                         ctypes.byref(geom), acc.data_ptr(), 1 if int_mode else 0, ctypes.byref(decoded))
        if rc != 0:
            raise self._err("mrcz_uncompress_binned", rc)
        return int(decoded.value)

    def binned_finish_device(self, geom: MrczBinGeom, acc: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """the binned volume (mrcz_binned_finish): (float)(acc / (fx fy fz)) as an (mz, my, mx) float32 cuda tensor (`out`, or
        allocated when None)"""
        shape = (geom.nz // geom.fz, geom.ny // geom.fy, geom.nx // geom.fx) if min(geom.fx, geom.fy, geom.fz) else (0, 0, 0)
        assert acc.is_cuda and acc.dtype == torch.float64 and acc.is_contiguous() and acc.numel() >= shape[0] * shape[1] * shape[2]
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=acc.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= shape[0] * shape[1] * shape[2]
        torch.cuda.current_stream(acc.device).synchronize()
        rc = _LIB.mrcz_binned_finish(self._ctx, ctypes.byref(geom), acc.data_ptr(), out.data_ptr())
        if rc != 0:
            raise self._err("mrcz_binned_finish", rc)
        return out

    def uncompress_compare_device(self, records: torch.Tensor, nfloats_file: int, orig: torch.Tensor, acc: torch.Tensor, first_chunk: int = 0,
                                  nchunks: int = None, abs_err=None, rel_err=None, chk: int = CHUNK_FLOATS, int_mode: bool = False):
        """compare decode, one step (mrcz_uncompress_compare): `records` (cuda uint8) = the chunk records of chunks [first_chunk,
        first_chunk + nchunks) of a file of nfloats_file floats (default: every chunk from first_chunk on); `orig` (cuda, 4-byte
        elements) = the original's words of exactly those chunks.  Assigns chunk c's summary to record c of `acc`, a cuda uint8
        tensor of ceil(nfloats_file / chk) * sizeof(MrczCompare) bytes (no zeroing needed).  abs_err / rel_err: the bounds
        counted in n_over_abs / n_over_rel (None: off).  Steps cover the chunks in any order, each once; then
        compare_finish_device."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        if nchunks is None:
            nchunks = max((nfloats_file + chk - 1) // chk - first_chunk, 0)
        nwords = max(min(nchunks * chk, nfloats_file - first_chunk * chk), 0)
        assert orig.is_cuda and orig.is_contiguous() and orig.element_size() == 4 and orig.numel() >= nwords
        nch = (nfloats_file + chk - 1) // chk
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.is_contiguous() and acc.numel() >= nch * ctypes.sizeof(MrczCompare)
        torch.cuda.current_stream(records.device).synchronize()
        rc = _LIB.mrcz_uncompress_compare(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, nchunks,
                                          orig.data_ptr(), -1.0 if abs_err is None else float(abs_err),
                                          -1.0 if rel_err is None else float(rel_err), 1 if int_mode else 0, acc.data_ptr())
        if rc != 0:
            raise self._err("mrcz_uncompress_compare", rc)

    def compare_finish_device(self, acc: torch.Tensor, first_chunk: int, nchunks: int) -> MrczCompare:
        """the fold of chunk records [first_chunk, first_chunk + nchunks) of `acc` (mrcz_compare_finish) as an MrczCompare"""
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.numel() >= (first_chunk + nchunks) * ctypes.sizeof(MrczCompare)
        total = MrczCompare()
        rc = _LIB.mrcz_compare_finish(self._ctx, acc.data_ptr(), first_chunk, nchunks, ctypes.byref(total))
        if rc != 0:
            raise self._err("mrcz_compare_finish", rc)
        return total

    @staticmethod
    def _compare_dict(rec: MrczCompare) -> dict:
        return {k: getattr(rec, k) for k, _ in MrczCompare._fields_}

    def verify(self, container_or_path, original, abs_err=None, rel_err=None, mode: str = "float", per_chunk: bool = False):
        """how well a container reproduces `original` (bytes, a path, or a cuda tensor of the file's words), without holding the
        decoded volume: the container's records are read and compared in pieces of at most max_batch_chunks chunks, a host
        original is uploaded in the same pieces.  Returns the file's MrczCompare fields as a dict with the derived mean_err,
        rmse, psnr_db (inf when rmse == 0) and ok: no header word differs and, if a bound was given, no point exceeds it and no
        NaN / Inf word differs (the verdict of mrc_verify).  per_chunk: (dict, list of the chunks' dicts)."""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        with self._open(container_or_path) as f:
            nfl, chk = self._container_header(f)
            f.seek(0)
            fsz = unpack_file_header(f.read(FILE_HEADER_BYTES))[0]
            dev = isinstance(original, torch.Tensor)
            if dev:
                assert original.is_cuda and original.is_contiguous() and original.element_size() == 4
                osz = original.numel() * 4
                src = None
            else:
                src = io.BytesIO(original) if isinstance(original, (bytes, bytearray, memoryview)) else open(original, "rb")
                osz = src.seek(0, os.SEEK_END)
            try:
                if osz != fsz and not (dev and osz == nfl * 4):
                    raise MrczError(f"the original holds {osz} bytes, the container records {fsz}")
                nch = (nfl + chk - 1) // chk
                offs, off, size_ = [], FILE_HEADER_BYTES, ctypes.c_uint64()
                for c in range(nch):
                    offs.append(off)
                    f.seek(off)
                    h = f.read(16)
                    if len(h) < 16 or _LIB.mrcz_record_size(h, min(chk, nfl - c * chk), ctypes.byref(size_)) != 0:
                        raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
                    off += size_.value
                offs.append(off)
                rsz = ctypes.sizeof(MrczCompare)
                acc = torch.empty(max(nch, 1) * rsz, dtype=torch.uint8, device=self.device)
                step = max(int(self.max_batch_chunks), 1)
                for k in range(0, nch, step):
                    e = min(k + step, nch)
                    f.seek(offs[k])
                    body = f.read(offs[e] - offs[k])
                    if len(body) != offs[e] - offs[k]:
                        raise MrczError("truncated container: the records end early")
                    rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
                    w0, w1 = k * chk, min(e * chk, nfl)
                    if dev:
                        org = original.reshape(-1)[w0:w1]
                    else:
                        src.seek(4 * w0)
                        org = torch.frombuffer(bytearray(src.read(4 * (w1 - w0))), dtype=torch.int32).to(self.device)
                    self.uncompress_compare_device(rec, nfl, org, acc, first_chunk=k, nchunks=e - k, abs_err=abs_err, rel_err=rel_err, chk=chk,
                                                   int_mode=(mode == "int"))
                    del rec, org
                t = self._compare_dict(self.compare_finish_device(acc, 0, nch))
            finally:
                if src is not None:
                    src.close()
        n = t["n_finite"]
        t["mean_err"] = t["sum_err"] / n if n else 0.0
        t["rmse"] = float(np.sqrt(t["sum_err2"] / n)) if n else 0.0
        t["psnr_db"] = float("inf") if t["rmse"] == 0 else float(20.0 * np.log10((t["orig_max"] - t["orig_min"]) / t["rmse"]))
        bounded = abs_err is not None or rel_err is not None
        t["ok"] = t["n_header_diff"] == 0 and (not bounded or (t["n_over_abs"] == 0 and t["n_over_rel"] == 0 and t["n_special_diff"] == 0))
        if not per_chunk:
            return t
        raw = acc.cpu().numpy().tobytes()
        return t, [self._compare_dict(MrczCompare.from_buffer_copy(raw[c * rsz: (c + 1) * rsz])) for c in range(nch)]

    # ---- probe: the size and the error of a compress setting, nothing written ----
    def probe_device(self, words: torch.Tensor, bits: int = 0, first_chunk: int = 0, int_mode: bool = False, abs_err=None, acc: torch.Tensor = None,
                     err_abs=None, err_rel=None):
        """what compress_device(words, bits, first_chunk, int_mode=..., abs_err=...) would write and how well it would decode,
        without writing it (mrcz_probe_chunks): `words` as there, the same argument checks.  Returns (record bytes, plane_bytes[4],
        acc): the first two are exactly what compress_device returns as len(records) and plane_bytes; record first_chunk + i of
        `acc` (a cuda uint8 tensor of (first_chunk + chunks of words) * sizeof(MrczCompare) bytes, allocated when None, no zeroing
        needed) is the MrczCompare of chunk i as uncompress_compare_device would assign it for that container against `words`,
        with the bounds err_abs / err_rel counted in n_over_abs / n_over_rel (None: off).  Then compare_finish_device."""
        assert words.is_cuda and words.is_contiguous() and words.element_size() == 4
        if abs_err is not None:
            if bits != 0 or int_mode:
                raise MrczError("abs_err excludes bits != 0 and the int mode")
            abs_err = abs_bound(abs_err)
        n = words.numel()
        nch = first_chunk + (n + CHUNK_FLOATS - 1) // CHUNK_FLOATS
        rsz = ctypes.sizeof(MrczCompare)
        if acc is None:
            acc = torch.empty(max(nch, 1) * rsz, dtype=torch.uint8, device=words.device)
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.is_contiguous() and acc.numel() >= nch * rsz
        torch.cuda.current_stream(words.device).synchronize()
        olen = ctypes.c_uint64()
        planes = (ctypes.c_uint64 * 4)()
        xform = PROBE_INT8 if int_mode else PROBE_ABS if abs_err is not None else PROBE_MASK
        rc = _LIB.mrcz_probe_chunks(self._ctx, words.data_ptr(), n, first_chunk, xform, 0 if int_mode else bits, abs_err or 0.0,
                                    -1.0 if err_abs is None else float(err_abs), -1.0 if err_rel is None else float(err_rel), acc.data_ptr(),
                                    ctypes.byref(olen), planes)
        if rc != 0:
            raise self._err("mrcz_probe_chunks", rc)
        return int(olen.value), [int(p) for p in planes], acc

    def sweep(self, original, settings=None, per_chunk: bool = False):
        """the table a lossy setting is chosen from: for every setting the size of the container it would give and the error of
        what that container would decode to, from one read of `original` (bytes, a path, or a cuda tensor of the file's words)
        and without writing a container.  settings = a list of ("bits", b), ("abs", eps) and ("int",); default all 33 mask levels.
        A host original is read and uploaded once, in pieces of at most max_batch_chunks chunks, and every setting is probed on
        each resident piece (probe_device), so a file larger than device memory streams through.  Returns one dict per setting:
        setting, container_bytes (17 + record bytes; 0 for a file of fewer than 4 bytes, where zip_bytes returns b""), ratio (file
        bytes / container bytes), plane_bytes, the MrczCompare fields of the file, and mean_err, rmse, psnr_db as verify derives
        them.  per_chunk: each dict also holds "chunks", the list of the chunks' MrczCompare dicts."""
        if settings is None:
            settings = [("bits", b) for b in range(33)]
        kws = []
        for st in settings:
            st = tuple(st)
            if len(st) == 2 and st[0] == "bits" and 0 <= int(st[1]) <= 32:
                kws.append(dict(bits=int(st[1])))
            elif len(st) == 2 and st[0] == "abs":
                kws.append(dict(abs_err=abs_bound(st[1])))
            elif st == ("int",):
                kws.append(dict(int_mode=True))
            else:
                raise MrczError(f"setting {st!r}: want ('bits', 0..32), ('abs', eps) or ('int',)")
        dev = isinstance(original, torch.Tensor)
        if dev:
            assert original.is_cuda and original.is_contiguous() and original.element_size() == 4
            src, fsz = None, original.numel() * 4
        else:
            src = io.BytesIO(original) if isinstance(original, (bytes, bytearray, memoryview)) else open(os.fspath(original), "rb")
            fsz = src.seek(0, os.SEEK_END)
        try:
            nfl = fsz // 4
            nch = (nfl + CHUNK_FLOATS - 1) // CHUNK_FLOATS
            rsz = ctypes.sizeof(MrczCompare)
            accs = [torch.empty(max(nch, 1) * rsz, dtype=torch.uint8, device=self.device) for _ in kws]
            size = [0] * len(kws)
            planes = [[0, 0, 0, 0] for _ in kws]
            step = max(int(self.max_batch_chunks), 1)
            for k in range(0, nch, step):
                w0, w1 = k * CHUNK_FLOATS, min((k + step) * CHUNK_FLOATS, nfl)
                if dev:
                    piece = original.reshape(-1)[w0:w1]
                else:
                    src.seek(4 * w0)
                    piece = torch.frombuffer(bytearray(src.read(4 * (w1 - w0))), dtype=torch.int32).to(self.device)
                for i, kw in enumerate(kws):
                    n, pl, _ = self.probe_device(piece, first_chunk=k, acc=accs[i], **kw)
                    size[i] += n
                    planes[i] = [a + b for a, b in zip(planes[i], pl)]
                del piece
            rows = []
            for i, st in enumerate(settings):
                t = self._compare_dict(self.compare_finish_device(accs[i], 0, nch))
                n = t["n_finite"]
                t["mean_err"] = t["sum_err"] / n if n else 0.0
                t["rmse"] = float(np.sqrt(t["sum_err2"] / n)) if n else 0.0
                t["psnr_db"] = float("inf") if t["rmse"] == 0 else float(20.0 * np.log10((t["orig_max"] - t["orig_min"]) / t["rmse"]))
                cb = FILE_HEADER_BYTES + size[i] if nfl else 0
                row = {"setting": tuple(st), "container_bytes": cb, "ratio": fsz / cb if cb else 0.0, "plane_bytes": planes[i], **t}
                if per_chunk:
                    raw = accs[i].cpu().numpy().tobytes()
                    row["chunks"] = [self._compare_dict(MrczCompare.from_buffer_copy(raw[c * rsz: (c + 1) * rsz])) for c in range(nch)]
                rows.append(row)
        finally:
            if src is not None:
                src.close()
        return rows

    def uncompress_digest_device(self, records: torch.Tensor, nfloats_file: int, acc: torch.Tensor, first_chunk: int = 0, nchunks: int = None,
                                 chk: int = CHUNK_FLOATS, int_mode: bool = False):
        """digest decode, one step (mrcz_uncompress_digest): `records` (cuda uint8) = the chunk records of chunks [first_chunk,
        first_chunk + nchunks) of a file of nfloats_file floats (default: every chunk from first_chunk on).  Assigns the CRC-32 of
        what chunk c decodes to to record c of `acc`, a cuda uint8 tensor of ceil(nfloats_file / chk) * sizeof(MrczDigest) bytes
        (no zeroing needed).  Steps cover the chunks in any order, each once; then digest_finish_device."""
        assert records.is_cuda and records.dtype == torch.uint8 and records.is_contiguous()
        if nchunks is None:
            nchunks = max((nfloats_file + chk - 1) // chk - first_chunk, 0)
        nch = (nfloats_file + chk - 1) // chk
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.is_contiguous() and acc.numel() >= nch * ctypes.sizeof(MrczDigest)
        torch.cuda.current_stream(records.device).synchronize()
        rc = _LIB.mrcz_uncompress_digest(self._ctx, records.data_ptr(), records.numel(), nfloats_file, chk, first_chunk, nchunks,
                                         1 if int_mode else 0, acc.data_ptr())
        if rc != 0:
            raise self._err("mrcz_uncompress_digest", rc)

    def digest_words_device(self, words: torch.Tensor, xform=None, bits: int = 0, abs_err=None, first_chunk: int = 0, acc: torch.Tensor = None,
                            chk: int = CHUNK_FLOATS) -> torch.Tensor:
        """the chunk digests of words that are on the device (mrcz_digest_words): `words` (cuda, 4-byte elements) holds a file's
        words from chunk first_chunk on.  xform None: the CRC-32 of the words as they are (a plain file); "mask" (bits), "abs"
        (abs_err) or "int": of what a container written from them in that mode will decode to.  Returns `acc` (allocated when
        None): record first_chunk + i is chunk i of `words`; then digest_finish_device."""
        assert words.is_cuda and words.is_contiguous() and words.element_size() == 4
        x = {None: DIGEST_NONE, "none": DIGEST_NONE, "mask": DIGEST_MASK, "int": DIGEST_INT8, "abs": DIGEST_ABS}.get(xform, -1)
        if x < 0:
            raise MrczError("xform must be None, 'mask', 'abs' or 'int'")
        eps = abs_bound(abs_err) if x == DIGEST_ABS else 0.0
        nch = first_chunk + (words.numel() + chk - 1) // chk
        if acc is None:
            acc = torch.empty(max(nch, 1) * ctypes.sizeof(MrczDigest), dtype=torch.uint8, device=words.device)
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.is_contiguous() and acc.numel() >= nch * ctypes.sizeof(MrczDigest)
        torch.cuda.current_stream(words.device).synchronize()
        rc = _LIB.mrcz_digest_words(self._ctx, words.data_ptr(), words.numel(), first_chunk, chk, x, bits, eps, acc.data_ptr())
        if rc != 0:
            raise self._err("mrcz_digest_words", rc)
        return acc

    def digest_finish_device(self, acc: torch.Tensor, first_chunk: int, nchunks: int, per_chunk: bool = False):
        """(crc32, nbytes) of chunks [first_chunk, first_chunk + nchunks) of `acc` together (mrcz_digest_finish); per_chunk: also
        the list of the chunks' crc32"""
        rsz = ctypes.sizeof(MrczDigest)
        assert acc.is_cuda and acc.dtype == torch.uint8 and acc.numel() >= (first_chunk + nchunks) * rsz
        total = MrczDigest()
        rc = _LIB.mrcz_digest_finish(self._ctx, acc.data_ptr(), first_chunk, nchunks, ctypes.byref(total))
        if rc != 0:
            raise self._err("mrcz_digest_finish", rc)
        if not per_chunk:
            return total.crc32, total.nbytes
        raw = acc[first_chunk * rsz: (first_chunk + nchunks) * rsz].cpu().numpy().tobytes()
        return total.crc32, total.nbytes, [MrczDigest.from_buffer_copy(raw[c * rsz: (c + 1) * rsz]).crc32 for c in range(nchunks)]

    def _record_offsets(self, f, nfl: int, chk: int):
        """byte offset in the container of every chunk record, and of the end of the last, from the 16-byte chunk headers"""
        offs, off, size_ = [], FILE_HEADER_BYTES, ctypes.c_uint64()
        for c in range((nfl + chk - 1) // chk):
            offs.append(off)
            f.seek(off)
            h = f.read(16)
            if len(h) < 16 or _LIB.mrcz_record_size(h, min(chk, nfl - c * chk), ctypes.byref(size_)) != 0:
                raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
            off += size_.value
        offs.append(off)
        return offs

    def _digest(self, container_or_path, mode: str):
        """(nfl, chk, file crc32, chunk crc32s) of a container, its records read and decoded in pieces of max_batch_chunks"""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        with self._open(container_or_path) as f:
            nfl, chk = self._container_header(f)
            nch = (nfl + chk - 1) // chk
            offs = self._record_offsets(f, nfl, chk)
            acc = torch.empty(max(nch, 1) * ctypes.sizeof(MrczDigest), dtype=torch.uint8, device=self.device)
            step = max(int(self.max_batch_chunks), 1)
            for k in range(0, nch, step):
                e = min(k + step, nch)
                f.seek(offs[k])
                body = f.read(offs[e] - offs[k])
                if len(body) != offs[e] - offs[k]:
                    raise MrczError("truncated container: the records end early")
                rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
                self.uncompress_digest_device(rec, nfl, acc, first_chunk=k, nchunks=e - k, chk=chk, int_mode=(mode == "int"))
                del rec
            crc, _, chunks = self.digest_finish_device(acc, 0, nch, per_chunk=True)
        return nfl, chk, crc, chunks

    def digest(self, container_or_path, mode: str = "float", per_chunk: bool = False):
        """zlib.crc32 of the file a container (bytes or a path) decodes to, without holding the decoded volume: the records are
        read and decoded in pieces of at most max_batch_chunks chunks.  per_chunk: (crc32, list of the chunks' crc32)."""
        _, _, crc, chunks = self._digest(container_or_path, mode)
        return (crc, chunks) if per_chunk else crc

    def write_sidecar(self, container_or_path, sidecar_path=None, mode: str = "float") -> str:
        """the digest sidecar of a container as text; written to sidecar_path when given"""
        nfl, chk, crc, chunks = self._digest(container_or_path, mode)
        text = format_sidecar(nfl, chk, mode, crc, chunks)
        if sidecar_path is not None:
            with open(sidecar_path, "w", newline="\n") as g:
                g.write(text)
        return text

    def check_sidecar(self, container_or_path, sidecar, mode: str = None) -> dict:
        """a container against a sidecar (its text as str with its newlines or as bytes, or a path as os.PathLike or one-line str): {"ok", "file_expected", "file_got", "differing": [(chunk, expected,
        got)]}.  mode None: the sidecar's.  MrczError when the sidecar is not one or belongs to a file of other words, chunk
        size or chunks than the container's header names."""
        if isinstance(sidecar, os.PathLike) or (isinstance(sidecar, str) and "\n" not in sidecar):   # a path; text has lines
            try:
                with open(sidecar, "rb") as g:
                    sidecar = g.read()
            except OSError as e:
                raise MrczError(f"cannot read the sidecar: {e}")
        sc = parse_sidecar(sidecar)
        with self._open(container_or_path) as f:
            nfl, chk = self._container_header(f)
        if (sc["words"], sc["chunk"]) != (nfl, chk):
            raise MrczError(f"the sidecar is of a file of {sc['words']} words in chunks of {sc['chunk']}, the container holds {nfl} in chunks of {chk}")
        _, _, crc, chunks = self._digest(container_or_path, mode or sc["mode"])
        bad = [(c, e, g) for c, (e, g) in enumerate(zip(sc["crcs"], chunks)) if e != g]
        return {"ok": not bad and crc == sc["file"], "file_expected": sc["file"], "file_got": crc, "differing": bad}

    def erase_bits_device(self, words: torch.Tensor, bits: int, first_word_index: int = 0):
        assert words.is_cuda and words.element_size() == 4
        torch.cuda.current_stream(words.device).synchronize()
        rc = _LIB.mrcz_erase_bits(self._ctx, words.data_ptr(), words.numel(), first_word_index, bits)
        if rc != 0:
            raise self._err("mrcz_erase_bits", rc)
        return words

    def erase_abs_device(self, words: torch.Tensor, eps, first_word_index: int = 0):
        """what a container of compress_device(abs_err=eps) decodes to, in place: words at file index >= 256 rounded
        (mrcz_erase_abs); `words` holds file words first_word_index, ..."""
        assert words.is_cuda and words.element_size() == 4
        eps = abs_bound(eps)
        torch.cuda.current_stream(words.device).synchronize()
        rc = _LIB.mrcz_erase_abs(self._ctx, words.data_ptr(), words.numel(), first_word_index, eps)
        if rc != 0:
            raise self._err("mrcz_erase_abs", rc)
        return words

    def generate_kat_device(self, words: torch.Tensor, first_index: int = 0):
        """fill `words` (cuda, 32-bit elements) with words [first_index, ...) of the SURVEY App. D integer generator"""
        assert words.is_cuda and words.is_contiguous() and words.element_size() == 4
        torch.cuda.current_stream(words.device).synchronize()
        rc = _LIB.mrcz_generate_kat_words(self._ctx, words.data_ptr(), first_index, words.numel())
        if rc != 0:
            raise self._err("mrcz_generate_kat_words", rc)
        return words

    # ---- file-image API: same bytes as `mrc_tar_c -t zip|unzip` reads/writes ----
    def zip_bytes(self, data: bytes, bits: int, mode: str = "float", abs_err=None) -> bytes:
        """run_compress on an in-memory file image (src/core/workers.c:690-881); mode = dataConvertedType ("float" | "int").
        abs_err = eps: absolute-error mode (mrc_tar -e), with bits = 0 and mode "float" only; decoding needs nothing."""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        if bits < 0 or bits > 32:
            raise MrczError("bits must be in 0..32 (src/core/workers.c:29-37 has 33 table entries)")
        if abs_err is not None:
            if bits != 0 or mode == "int":
                raise MrczError("abs_err excludes bits != 0 and mode 'int' (mrc_tar -e excludes -b and -s int)")
            abs_err = abs_bound(abs_err)
        fsz = len(data)
        nfl = fsz // 4
        if nfl == 0:
            return b""  # src/core/workers.c:757: nothing is written when the first read is empty
        host = torch.frombuffer(bytearray(data[: nfl * 4]), dtype=torch.int32)
        dev = host.to(self.device)
        rec, _ = self.compress_device(dev, bits, 0, int_mode=(mode == "int"), abs_err=abs_err)
        return pack_file_header(fsz) + rec.cpu().numpy().tobytes()

    def unzip_bytes(self, container: bytes, mode: str = "float") -> bytes:
        """read_mrczip_header + run_uncompress (src/core/workers.c:568-688); mode as for zip_bytes (the container does not
        record it: the reference needs -s int again on decode)."""
        fsz, chk, typ, ztypes = unpack_file_header(container)
        if any(z not in (0, 2, 4) for z in ztypes):
            raise MrczError("byte stream compressor types must be ZLIB_DEF (0), LZ4_DEF (2) or LZ4HC_DEF (4)")
        rc = _LIB.mrcz_set_ztypes(self._ctx, bytes(bytearray(z & 0xff for z in ztypes)))
        if rc != 0:
            raise self._err("mrcz_set_ztypes", rc)
        nfl = fsz // 4
        if chk == 0:
            raise MrczError("chunk size 0 in header (the reference divides by it, src/core/workers.c:589)")
        if nfl == 0:
            return b""
        rec = torch.frombuffer(bytearray(container[FILE_HEADER_BYTES:]), dtype=torch.uint8).to(self.device)
        out, _ = self.uncompress_device(rec, nfl, chk, int_mode=(mode == "int"))
        return out.cpu().numpy().tobytes()

    # ---- range decode: part of a container without reading or decoding the rest ----
    def _range_device(self, f, w0: int, w1: int, mode: str) -> torch.Tensor:
        """words [w0, w1) of the container open as binary file `f`: reads the file header, the 16-byte headers of the chunks
        before the window and the records of the chunks that cover it, nothing else"""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        f.seek(0)
        fsz, chk, typ, ztypes = unpack_file_header(f.read(FILE_HEADER_BYTES))
        if any(z not in (0, 2, 4) for z in ztypes):
            raise MrczError("byte stream compressor types must be ZLIB_DEF (0), LZ4_DEF (2) or LZ4HC_DEF (4)")
        if chk == 0:
            raise MrczError("chunk size 0 in header (the reference divides by it, src/core/workers.c:589)")
        nfl = fsz // 4
        if not 0 <= w0 < w1 <= nfl:
            raise MrczError(f"window [{w0}, {w1}) is empty or outside the file's {nfl} words")
        rc = _LIB.mrcz_set_ztypes(self._ctx, bytes(bytearray(z & 0xff for z in ztypes)))
        if rc != 0:
            raise self._err("mrcz_set_ztypes", rc)
        c_lo, c_hi = w0 // chk, (w1 + chk - 1) // chk
        off, start, size = FILE_HEADER_BYTES, 0, ctypes.c_uint64()
        for c in range(c_hi):
            if c == c_lo:
                start = off
            f.seek(off)
            h = f.read(16)
            if len(h) < 16 or _LIB.mrcz_record_size(h, min(chk, nfl - c * chk), ctypes.byref(size)) != 0:
                raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
            off += size.value
        f.seek(start)
        body = f.read(off - start)
        if len(body) != off - start:
            raise MrczError("truncated container: the records of the window end early")
        rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
        out, _ = self.uncompress_range_device(rec, nfl, w0, w1, chk, first_chunk=c_lo, int_mode=(mode == "int"))
        return out

    def _container_header(self, f):
        """(floats of the file, chunk size) from the 17-byte file header; sets the context's compressor types"""
        f.seek(0)
        fsz, chk, typ, ztypes = unpack_file_header(f.read(FILE_HEADER_BYTES))
        if any(z not in (0, 2, 4) for z in ztypes):
            raise MrczError("byte stream compressor types must be ZLIB_DEF (0), LZ4_DEF (2) or LZ4HC_DEF (4)")
        if chk == 0:
            raise MrczError("chunk size 0 in header (the reference divides by it, src/core/workers.c:589)")
        rc = _LIB.mrcz_set_ztypes(self._ctx, bytes(bytearray(z & 0xff for z in ztypes)))
        if rc != 0:
            raise self._err("mrcz_set_ztypes", rc)
        return fsz // 4, chk

    def _mrc_volume(self, f):
        """(data_word0, nx, ny, nz) of the float32 (mode 2) MRC volume in the container open as `f`: the MRC header (nx, ny, nz,
        mode at bytes 0-15, nsymbt at 92-95) comes from the decoded first 256 words, the data start at byte 1024 + nsymbt (whether
        the file holds all of it is the caller's check)"""
        f.seek(0)
        fsz = unpack_file_header(f.read(FILE_HEADER_BYTES))[0]
        if fsz // 4 < MRC_HEADER_BYTES // 4:
            raise MrczError("file shorter than an MRC header")
        hdr = self._range_device(f, 0, MRC_HEADER_BYTES // 4, "float").cpu().numpy().tobytes()
        nx, ny, nz, mode = struct.unpack("<4i", hdr[:16])
        (nsymbt,) = struct.unpack("<i", hdr[92:96])
        if mode != 2:
            raise MrczError(f"MRC mode {mode}: only mode 2 (float32) volumes can be read as slabs or boxes")
        if nx <= 0 or ny <= 0 or nz <= 0 or nsymbt < 0 or nsymbt % 4:
            raise MrczError(f"implausible MRC header: nx={nx} ny={ny} nz={nz} nsymbt={nsymbt}")
        return (MRC_HEADER_BYTES + nsymbt) // 4, nx, ny, nz

    def _open(self, container_or_path):
        if isinstance(container_or_path, (bytes, bytearray, memoryview)):
            return io.BytesIO(container_or_path)
        return open(os.fspath(container_or_path), "rb")

    def unzip_range(self, container_or_path, w0: int, w1: int, mode: str = "float") -> bytes:
        """bytes 4*w0 .. 4*w1 of what unzip_bytes returns, from a container in memory or a path; for a path only the covering
        chunk records are read from the file."""
        with self._open(container_or_path) as f:
            return self._range_device(f, w0, w1, mode).cpu().numpy().tobytes()

    def read_mrc_slab(self, path, z0: int, z1: int) -> torch.Tensor:
        """sections [z0, z1) of a compressed float32 (mode 2) MRC volume as a (z1 - z0, ny, nx) float32 cuda tensor.  The MRC
        header (nx, ny, nz, mode at bytes 0-15, nsymbt at 92-95) comes from the decoded first 256 words; the data start at
        byte 1024 + nsymbt."""
        with self._open(path) as f:
            f.seek(0)
            fsz = unpack_file_header(f.read(FILE_HEADER_BYTES))[0]
            d0, nx, ny, nz = self._mrc_volume(f)
            if not 0 <= z0 < z1 <= nz:
                raise MrczError(f"sections [{z0}, {z1}) outside 0..{nz}")
            sec = nx * ny
            w0 = d0 + z0 * sec
            w1 = w0 + (z1 - z0) * sec
            if w1 > fsz // 4:
                raise MrczError("the MRC header describes more data than the file holds")
            out = self._range_device(f, w0, w1, "float")
        return out.view(torch.float32).reshape(z1 - z0, ny, nx)

    def read_mrc_boxes(self, path_or_bytes, centers, size, fill: float = 0.0, mode: str = "float") -> torch.Tensor:
        """boxes around particle centres of a compressed float32 (mode 2) MRC volume, as an (N, bz, by, bx) float32 cuda tensor.
        `centers` = (N, 3) x, y, z (integer or float, as pickers write them); `size` = an int or (bx, by, bz).  Box i starts at
        round(c) - size // 2 per axis (round(v) = floor(v + 0.5)); voxels outside the volume are `fill`.  Reads the file
        header, the headers of the chunks up to the last one a box touches, and the records of the touched chunks (one read
        and one decode call per run of them); each touched chunk is decoded once, no other is."""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        bx, by, bz = (int(size),) * 3 if np.ndim(size) == 0 else tuple(int(v) for v in size)
        if min(bx, by, bz) < 1:
            raise MrczError(f"box size {(bx, by, bz)}: every side must be at least 1")
        cen = np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(-1, 3))
        n = len(cen)
        with self._open(path_or_bytes) as f:
            nfl, chk = self._container_header(f)
            d0, nx, ny, nz = self._mrc_volume(f)
            if d0 + nx * ny * nz > nfl:
                raise MrczError("the MRC header describes more data than the file holds")
            fill_bits = int(np.array([fill], np.float32).view(np.uint32)[0])
            geom = MrczBoxGeom(d0, nx, ny, nz, bx, by, bz, fill_bits)
            org = np.zeros((n, 3), np.int32)
            if _LIB.mrcz_box_origins(ctypes.byref(geom), cen.ctypes.data, n, org.ctypes.data) != 0:
                raise MrczError("a centre is not finite or its box corner lies outside int32")
            nch = (nfl + chk - 1) // chk
            covered = np.zeros(nch, np.uint8)
            if _LIB.mrcz_boxes_chunks(ctypes.byref(geom), org.ctypes.data, n, nfl, chk, covered.ctypes.data) != 0:
                raise MrczError("box geometry refused")
            out = torch.empty((n, bz, by, bx), dtype=torch.int32, device=self.device)
            idx = np.flatnonzero(covered)
            # record offsets from the chunk headers, up to the last covered chunk (nothing behind it is read)
            offs, off, size_ = [], FILE_HEADER_BYTES, ctypes.c_uint64()
            for c in range(int(idx[-1]) + 1 if len(idx) else 0):
                offs.append(off)
                f.seek(off)
                h = f.read(16)
                if len(h) < 16 or _LIB.mrcz_record_size(h, min(chk, nfl - c * chk), ctypes.byref(size_)) != 0:
                    raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
                off += size_.value
            offs.append(off)
            # one read and one decode call per maximal run of covered chunks
            runs = np.split(idx, np.flatnonzero(np.diff(idx) != 1) + 1) if len(idx) else []
            for run in runs:
                c0, c1 = int(run[0]), int(run[-1]) + 1
                f.seek(offs[c0])
                body = f.read(offs[c1] - offs[c0])
                if len(body) != offs[c1] - offs[c0]:
                    raise MrczError("truncated container: the records of the boxes' chunks end early")
                rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
                self.uncompress_boxes_device(rec, nfl, geom, org, first_chunk=c0, nchunks=c1 - c0, out=out, int_mode=(mode == "int"),
                                             chk=chk)
            if not runs:  # every box outside the volume: the fill alone
                self.uncompress_boxes_device(torch.empty(16, dtype=torch.uint8, device=self.device), nfl, geom, org, nchunks=0,
                                             out=out, chk=chk)
        return out.view(torch.float32)

    def read_mrc_binned(self, path_or_bytes, factor, mode: str = "float") -> torch.Tensor:
        """a compressed float32 (mode 2) MRC volume average-pooled by `factor` (an int or (fx, fy, fz)), as an (mz, my, mx) =
        (nz // fz, ny // fy, nx // fx) float32 cuda tensor; voxels of a trailing remainder of an axis are ignored.  Each mean is
        the float64 sum of the bin's voxels in file order over fx fy fz, narrowed to float32 (mrcz_uncompress_binned).  Reads the
        file header, the chunk headers up to the last chunk the bins use, then the records of the used chunks in pieces of at
        most max_batch_chunks chunks, one decode call per piece: neither host nor device holds the whole container, and the
        device holds no buffer of the volume's size."""
        if mode not in ("float", "int"):
            raise MrczError("mode must be 'float' or 'int' (mrc_tar -s)")
        f3 = (int(factor),) * 3 if np.ndim(factor) == 0 else tuple(int(v) for v in factor)
        if len(f3) != 3:
            raise MrczError(f"bin factor {factor}: want an int or (fx, fy, fz)")
        fx, fy, fz = f3
        with self._open(path_or_bytes) as f:
            nfl, chk = self._container_header(f)
            d0, nx, ny, nz = self._mrc_volume(f)
            if d0 + nx * ny * nz > nfl:
                raise MrczError("the MRC header describes more data than the file holds")
            if not (1 <= fx <= nx and 1 <= fy <= ny and 1 <= fz <= nz) or fx * fy * fz > 1 << 31:
                raise MrczError(f"bin factor {(fx, fy, fz)} outside 1 .. {(nx, ny, nz)} (or a bin of more than 2^31 voxels)")
            geom = MrczBinGeom(d0, nx, ny, nz, fx, fy, fz)
            c0, c1 = ctypes.c_uint64(), ctypes.c_uint64()
            if _LIB.mrcz_bin_chunks(ctypes.byref(geom), nfl, chk, ctypes.byref(c0), ctypes.byref(c1)) != 0:
                raise MrczError("bin geometry refused")
            c0, c1 = int(c0.value), int(c1.value)
            # record offsets from the chunk headers, up to c1 (nothing behind it is read)
            offs, off, size_ = [], FILE_HEADER_BYTES, ctypes.c_uint64()
            for c in range(c1):
                offs.append(off)
                f.seek(off)
                h = f.read(16)
                if len(h) < 16 or _LIB.mrcz_record_size(h, min(chk, nfl - c * chk), ctypes.byref(size_)) != 0:
                    raise MrczError(f"damaged or truncated container: chunk header {c} at byte {off}")
                off += size_.value
            offs.append(off)
            acc = torch.empty((nz // fz, ny // fy, nx // fx), dtype=torch.float64, device=self.device)
            step = max(int(self.max_batch_chunks), 1)
            for k in range(c0, c1, step):
                e = min(k + step, c1)
                f.seek(offs[k])
                body = f.read(offs[e] - offs[k])
                if len(body) != offs[e] - offs[k]:
                    raise MrczError("truncated container: the records of the binned chunks end early")
                rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
                self.uncompress_binned_device(rec, nfl, geom, acc, first_chunk=k, nchunks=e - k, int_mode=(mode == "int"), chk=chk)
                del rec
        return self.binned_finish_device(geom, acc)

    # ---- top-planes decode: bfloat16-precision reads that leave the low byte planes on the disk ----
    def _top_words(self, f, keep: int, dtype) -> torch.Tensor:
        """every word of the container open as `f` under the mask of `keep` planes, as a 1-D cuda tensor of `dtype`: thinned
        records read and decoded in pieces of at most max_batch_chunks chunks"""
        nfl, chk = self._container_header(f)
        nch = (nfl + chk - 1) // chk
        out = torch.empty(max(nfl, 1), dtype=dtype, device=self.device)
        step, off = max(int(self.max_batch_chunks), 1), FILE_HEADER_BYTES
        for k in range(0, nch, step):
            e = min(k + step, nch)
            body, off = read_thinned_records(f, nfl, chk, keep, k, e - k, start=off)
            rec = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(self.device)
            dst = out[k * chk:]
            if dst.data_ptr() % 16 == 0:
                self.uncompress_top_device(rec, nfl, keep, dtype, first_chunk=k, nchunks=e - k, thinned=True, out=dst, chk=chk)
            else:  # a chunk size whose pieces do not start on 16 bytes: through a buffer of the piece's own
                piece = self.uncompress_top_device(rec, nfl, keep, dtype, first_chunk=k, nchunks=e - k, thinned=True, chk=chk)
                dst[: piece.numel()] = piece
            del rec
        return out[:nfl]

    def unzip_top(self, container_or_path, keep: int = 2, dtype=torch.bfloat16) -> torch.Tensor:
        """all floor(fsz / 4) words of a container (bytes or a path) with only their `keep` top byte planes, as a 1-D cuda tensor
        of `dtype` (uncompress_top_device: truncation, the header words included).  Of a path only the file header, the 16-byte
        chunk headers and the kept payloads are read."""
        with self._open(container_or_path) as f:
            return self._top_words(f, keep, dtype)

    def read_mrc_top(self, path, keep: int = 2, dtype=torch.bfloat16) -> torch.Tensor:
        """a compressed float32 (mode 2) MRC volume at reduced precision, as an (nz, ny, nx) cuda tensor of `dtype`
        (uncompress_top_device: bfloat16 by truncation for keep 2).  The MRC header comes from a range decode of the first 256
        words, as in read_mrc_slab; the voxels from thinned records, so the low byte planes of the file are never read."""
        with self._open(path) as f:
            nfl, _ = self._container_header(f)
            d0, nx, ny, nz = self._mrc_volume(f)
            if d0 + nx * ny * nz > nfl:
                raise MrczError("the MRC header describes more data than the file holds")
            words = self._top_words(f, keep, dtype)
        return words[d0: d0 + nx * ny * nz].reshape(nz, ny, nx)
