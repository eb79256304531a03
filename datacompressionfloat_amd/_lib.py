"""ctypes binding of the C ABI declared in include/mrcz_hip.h (no torch types cross it)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MRCZ_LIB_PATH: developer knob (tools/ab_*.py time several builds of the kernels in one GPU call); it still is a HIP build
LIB_PATH = os.environ.get("MRCZ_LIB_PATH") or os.path.join(_HERE, "lib", "libmrcz_hip.so")


class MrczLibraryMissing(ImportError):
    pass


class MrczBoxGeom(ctypes.Structure):
    """mrcz_box_geom_t: a float32 volume of nx x ny x nz words from file word data_word0, boxes of bx x by x bz voxels"""
    _fields_ = [("data_word0", ctypes.c_uint64), ("nx", ctypes.c_uint32), ("ny", ctypes.c_uint32), ("nz", ctypes.c_uint32),
                ("bx", ctypes.c_uint32), ("by", ctypes.c_uint32), ("bz", ctypes.c_uint32), ("fill_bits", ctypes.c_uint32)]


class MrczBinGeom(ctypes.Structure):
    """mrcz_bin_geom_t: a float32 volume of nx x ny x nz words from file word data_word0, binned by fx x fy x fz"""
    _fields_ = [("data_word0", ctypes.c_uint64), ("nx", ctypes.c_uint32), ("ny", ctypes.c_uint32), ("nz", ctypes.c_uint32),
                ("fx", ctypes.c_uint32), ("fy", ctypes.c_uint32), ("fz", ctypes.c_uint32)]


class MrczCompare(ctypes.Structure):
    """mrcz_compare_t: the error summary of one chunk, or of a whole file, against the original"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("n", "n_header_diff", "n_diff", "n_finite", "n_special_diff", "n_over_abs", "n_over_rel",
                                               "first_over", "max_err_index", "max_rel_index")] + \
               [(k, ctypes.c_double) for k in ("max_err", "max_rel", "sum_err", "sum_abs_err", "sum_err2", "orig_min", "orig_max",
                                               "orig_sum", "orig_sum2")]


class MrczDigest(ctypes.Structure):
    """mrcz_digest_t: the CRC-32 of what one chunk, or a whole file, decodes to"""
    _fields_ = [("crc32", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("nbytes", ctypes.c_uint64)]


DIGEST_NONE, DIGEST_MASK, DIGEST_INT8, DIGEST_ABS = 0, 1, 2, 3  # MRCZ_DIGEST_*
TOP_F32, TOP_U16, TOP_THINNED = 0, 1, 4                         # MRCZ_TOP_*
PROBE_MASK, PROBE_ABS, PROBE_INT8 = 0, 1, 2                     # MRCZ_PROBE_*


def load():
    if not os.path.exists(LIB_PATH):
        raise MrczLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the codec."
        )
    lib = ctypes.CDLL(LIB_PATH)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.mrcz_create.restype = i32
    lib.mrcz_create.argtypes = [ctypes.POINTER(vp), i32, u32]
    lib.mrcz_destroy.restype = None
    lib.mrcz_destroy.argtypes = [vp]
    lib.mrcz_last_error.restype = ctypes.c_char_p
    lib.mrcz_last_error.argtypes = [vp]
    lib.mrcz_stream.restype = vp
    lib.mrcz_stream.argtypes = [vp]
    lib.mrcz_records_bound.restype = u64
    lib.mrcz_records_bound.argtypes = [u64]
    lib.mrcz_compress_chunks.restype = i32
    lib.mrcz_compress_chunks.argtypes = [vp, vp, u64, u64, i32, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_uncompress_chunks.restype = i32
    lib.mrcz_uncompress_chunks.argtypes = [vp, vp, u64, u64, u32, vp, ctypes.POINTER(u64)]
    lib.mrcz_compress_chunks_int8.restype = i32
    lib.mrcz_compress_chunks_int8.argtypes = [vp, vp, u64, u64, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_uncompress_chunks_int8.restype = i32
    lib.mrcz_uncompress_chunks_int8.argtypes = [vp, vp, u64, u64, u32, u64, vp, ctypes.POINTER(u64)]
    lib.mrcz_compress_chunks_abs.restype = i32
    lib.mrcz_compress_chunks_abs.argtypes = [vp, vp, u64, u64, ctypes.c_float, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_record_size.restype = i32
    lib.mrcz_record_size.argtypes = [vp, u32, ctypes.POINTER(u64)]
    lib.mrcz_records_index.restype = i32
    lib.mrcz_records_index.argtypes = [vp, u64, u64, u32, ctypes.POINTER(u64)]
    lib.mrcz_uncompress_range.restype = i32
    lib.mrcz_uncompress_range.argtypes = [vp, vp, u64, u64, u32, u64, u64, u64, vp, i32, ctypes.POINTER(u64)]
    geom = ctypes.POINTER(MrczBoxGeom)
    lib.mrcz_box_origins.restype = i32
    lib.mrcz_box_origins.argtypes = [geom, vp, u32, vp]
    lib.mrcz_boxes_chunks.restype = i32
    lib.mrcz_boxes_chunks.argtypes = [geom, vp, u32, u64, u32, vp]
    lib.mrcz_uncompress_boxes.restype = i32
    lib.mrcz_uncompress_boxes.argtypes = [vp, vp, u64, u64, u32, u64, u64, geom, vp, u32, vp, i32, ctypes.POINTER(u64)]
    bgeom = ctypes.POINTER(MrczBinGeom)
    lib.mrcz_bin_chunks.restype = i32
    lib.mrcz_bin_chunks.argtypes = [bgeom, u64, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_uncompress_binned.restype = i32
    lib.mrcz_uncompress_binned.argtypes = [vp, vp, u64, u64, u32, u64, u64, bgeom, vp, i32, ctypes.POINTER(u64)]
    lib.mrcz_binned_finish.restype = i32
    lib.mrcz_binned_finish.argtypes = [vp, bgeom, vp, vp]
    lib.mrcz_uncompress_compare.restype = i32
    lib.mrcz_uncompress_compare.argtypes = [vp, vp, u64, u64, u32, u64, u64, vp, ctypes.c_double, ctypes.c_double, i32, vp]
    lib.mrcz_compare_finish.restype = i32
    lib.mrcz_compare_finish.argtypes = [vp, vp, u64, u64, ctypes.POINTER(MrczCompare)]
    lib.mrcz_probe_chunks.restype = i32
    lib.mrcz_probe_chunks.argtypes = [vp, vp, u64, u64, i32, i32, ctypes.c_float, ctypes.c_double, ctypes.c_double, vp, ctypes.POINTER(u64),
                                      ctypes.POINTER(u64)]
    lib.mrcz_crc32_combine.restype = u32
    lib.mrcz_crc32_combine.argtypes = [u32, u32, u64]
    lib.mrcz_uncompress_digest.restype = i32
    lib.mrcz_uncompress_digest.argtypes = [vp, vp, u64, u64, u32, u64, u64, i32, vp]
    for f in (lib.mrcz_digest_words, lib.mrcz_digest_words_async):
        f.restype = i32
        f.argtypes = [vp, vp, u64, u64, u32, i32, i32, ctypes.c_float, vp]
    lib.mrcz_digest_finish.restype = i32
    lib.mrcz_digest_finish.argtypes = [vp, vp, u64, u64, ctypes.POINTER(MrczDigest)]
    lib.mrcz_record_top_span.restype = i32
    lib.mrcz_record_top_span.argtypes = [vp, u32, i32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.mrcz_uncompress_top.restype = i32
    lib.mrcz_uncompress_top.argtypes = [vp, vp, u64, u64, u32, u64, u64, i32, i32, vp, ctypes.POINTER(u64)]
    lib.mrcz_generate_kat_words.restype = i32
    lib.mrcz_generate_kat_words.argtypes = [vp, vp, u64, u64]
    lib.mrcz_set_ztypes.restype = i32
    lib.mrcz_set_ztypes.argtypes = [vp, ctypes.c_char_p]
    lib.mrcz_erase_bits.restype = i32
    lib.mrcz_erase_bits.argtypes = [vp, vp, u64, u64, i32]
    lib.mrcz_erase_abs.restype = i32
    lib.mrcz_erase_abs.argtypes = [vp, vp, u64, u64, ctypes.c_float]
    lib.mrcz_set_timing.restype = i32
    lib.mrcz_set_timing.argtypes = [vp, i32]
    lib.mrcz_last_timings.restype = i32
    lib.mrcz_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float), i32]
    lib.mrcz_debug_fallbacks.restype = ctypes.c_int64
    lib.mrcz_debug_fallbacks.argtypes = [vp]
    lib.mrcz_debug_chain_fallbacks.restype = ctypes.c_int64
    lib.mrcz_debug_chain_fallbacks.argtypes = [vp]
    lib.mrcz_debug_emit_splits.restype = ctypes.c_int64
    lib.mrcz_debug_emit_splits.argtypes = [vp]
    return lib


# every symbol include/mrcz_hip.h declares (checked by tests/test_abi.py without a GPU)
EXPORTS = [
    "mrcz_create", "mrcz_destroy", "mrcz_last_error", "mrcz_stream", "mrcz_records_bound",
    "mrcz_compress_chunks", "mrcz_uncompress_chunks", "mrcz_erase_bits", "mrcz_set_timing",
    "mrcz_last_timings", "mrcz_debug_blocks", "mrcz_debug_fallbacks", "mrcz_debug_chain_fallbacks", "mrcz_debug_emit_splits", "mrcz_debug_inflate_phases", "mrcz_debug_candidates", "mrcz_device_count", "mrcz_dev_malloc", "mrcz_dev_free",
    "mrcz_host_malloc", "mrcz_host_free", "mrcz_copy_h2d", "mrcz_copy_d2h",
    "mrcz_event_create", "mrcz_event_destroy", "mrcz_event_record", "mrcz_stream_wait_event", "mrcz_event_sync",
    "mrcz_copy_h2d_async", "mrcz_copy_d2h_async", "mrcz_compress_chunks_async", "mrcz_uncompress_chunks_async",
    "mrcz_set_ztypes", "mrcz_generate_kat_words", "mrcz_err_hist", "mrcz_err_collect", "mrcz_compress_chunks_int8", "mrcz_uncompress_chunks_int8", "mrcz_compress_chunks_int8_async", "mrcz_uncompress_chunks_int8_async",
    "mrcz_record_size", "mrcz_records_index", "mrcz_uncompress_range", "mrcz_uncompress_range_async",
    "mrcz_box_origins", "mrcz_boxes_chunks", "mrcz_uncompress_boxes",
    "mrcz_bin_chunks", "mrcz_uncompress_binned", "mrcz_binned_finish",
    "mrcz_compress_chunks_abs", "mrcz_compress_chunks_abs_async", "mrcz_erase_abs",
    "mrcz_uncompress_compare", "mrcz_compare_finish",
    "mrcz_probe_chunks", "mrcz_probe_chunks_async",
    "mrcz_crc32_combine", "mrcz_uncompress_digest", "mrcz_digest_words", "mrcz_digest_words_async", "mrcz_digest_finish",
    "mrcz_record_top_span", "mrcz_uncompress_top", "mrcz_uncompress_top_async",
]
