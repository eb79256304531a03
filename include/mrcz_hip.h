/*
 * mrcz_hip.h -- C ABI of the MI355X (gfx950) float32 mask + byte-plane + DEFLATE(Z_RLE) codec.
 *
 * This is the device-level boundary that sits UNDER the reference's own chunk-codec seam
 * (run_compress / run_uncompress, /root/reference/src/include/workers.h:30-31 -- see mrcz_workers.h
 * for the drop-in replacement of that seam).  It replaces, for a batch of chunks that is already
 * resident in HBM:
 *
 *   reference function                               file:line                      here
 *   -----------------------------------------------  -----------------------------  ---------------------
 *   apply_mask + split_float_to_byte_stream          src/core/workers.c:82-101,     mrcz_compress_chunks
 *                                                    src/core/workers.c:180-203
 *   mzlib_def (deflate(Z_FULL_FLUSH) per plane,      src/core/zip.c:164-196         mrcz_compress_chunks
 *     RAW test, pack_header)                         src/core/zip.c:381-391
 *   chunk record writer of run_compress              src/core/workers.c:837-850     mrcz_compress_chunks
 *   uncompress_byte_stream + mzlib_inf               src/core/workers.c:52-80,      mrcz_uncompress_chunks
 *                                                    src/core/zip.c:262-284
 *   merge_byte_to_float_stream                       src/core/workers.c:423-442     mrcz_uncompress_chunks
 *
 * Plain pointers and sizes only; no torch types.  All device pointers are ordinary HIP device
 * allocations (hipMalloc or a torch tensor's data_ptr()).  Functions return 0 on success and a
 * negative MRCZ_E* code on failure; they never fall back to the CPU.
 */
#ifndef MRCZ_HIP_H_
#define MRCZ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRCZ_CHUNK_FLOATS 6291456u /* src/include/constant.h:25 CHUNK_SIZE */
#define MRCZ_FILE_HEADER_BYTES 17  /* src/core/common.c:137-148 */

#define MRCZ_OK 0
#define MRCZ_EINVAL (-1)   /* bad argument (bits outside 0..32, NULL pointer, ...) */
#define MRCZ_ENOMEM (-2)   /* device allocation failed */
#define MRCZ_ECAP (-3)     /* output capacity too small */
#define MRCZ_EFORMAT (-4)  /* malformed container / deflate stream */
#define MRCZ_EHIP (-5)     /* HIP runtime error (see mrcz_last_error) */

typedef struct mrcz_ctx mrcz_ctx_t;

/* Create a codec context on HIP device `device` owning one stream and a workspace sized for
 * batches of up to `max_batch_chunks` chunks (0 = default 64).  Thread-safety: one context per
 * calling thread (the reference's workers call run_compress concurrently on different files,
 * src/main/mrc_tarx.c:134-176; give each its own context). */
int mrcz_create(mrcz_ctx_t **ctx, int device, uint32_t max_batch_chunks);
void mrcz_destroy(mrcz_ctx_t *ctx);
const char *mrcz_last_error(const mrcz_ctx_t *ctx);
/* HIP stream (hipStream_t) all work of this context is enqueued on; for external event timing. */
void *mrcz_stream(mrcz_ctx_t *ctx);

/* Worst-case bytes of chunk records for nfloats input floats (16 B per chunk + 4 B per float). */
uint64_t mrcz_records_bound(uint64_t nfloats);

/*
 * Compress `nfloats` float32 words that start a chunk boundary of a file.
 *   d_in           device pointer, 16-byte aligned, nfloats 32-bit words
 *   first_chunk    index within the FILE of the first chunk in d_in (chunk 0 keeps its first 256
 *                  words unmasked, src/core/workers.c:90-94,777,804)
 *   bits           low bits to erase, 0..32 (src/core/workers.c:29-37)
 *   d_out          device pointer, receives the chunk records back to back exactly as
 *                  run_compress writes them after the 17-byte file header
 *                  (src/core/workers.c:837-850): 16-byte header + 4 payloads per chunk
 *   out_cap        capacity of d_out in bytes (>= mrcz_records_bound(nfloats))
 *   out_len        (host) total bytes written
 *   plane_bytes    (host, optional, 4 x u64) per-plane sum of payload+4 bytes, i.e. what the
 *                  reference accumulates in mzip_t.zfsz (src/core/zip.c:193-194)
 * Synchronous with respect to the host on return (results are final).
 */
int mrcz_compress_chunks(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk,
                         int bits, void *d_out, uint64_t out_cap, uint64_t *out_len,
                         uint64_t plane_bytes[4]);

/*
 * Decompress chunk records (no file header) holding `nfloats` floats in chunks of `chk` floats
 * (hd->chk, src/core/workers.c:577-578; only chk == MRCZ_CHUNK_FLOATS or a single smaller chunk
 * layout is produced by the reference).
 *   d_records/len  device pointer + byte length of the records
 *   d_out          device pointer, 16-byte aligned, receives nfloats 32-bit words
 *   consumed       (host, optional) bytes of d_records actually consumed
 */
int mrcz_uncompress_chunks(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats,
                           uint32_t chk, void *d_out, uint64_t *consumed);

/* Compressor types of the four byte streams of the containers the context will decode, as the 17-byte file header records
 * them (ztypes[4], src/core/common.c:143-146; enum src/include/mrczip.h:37-40): 0 = ZLIB_DEF (what every writer of the
 * reference produces, workers.c:719), 2 = LZ4_DEF, 4 = LZ4HC_DEF (decoder tolerance: the reference's reader accepts them,
 * workers.c:584, zip.c:69-86,306-318).  Default all 0; stays in force until set again.  Anything else: MRCZ_EFORMAT. */
int mrcz_set_ztypes(mrcz_ctx_t *ctx, const signed char ztypes[4]);

/* Plain-C device memory helpers so that C host code (the C files under datacompressionfloat_amd/host) needs no HIP
 * headers: device buffers, pinned host buffers, synchronous copies on the context's stream. */
int mrcz_device_count(void);
int mrcz_dev_malloc(mrcz_ctx_t *ctx, void **d_ptr, uint64_t bytes);
int mrcz_dev_free(mrcz_ctx_t *ctx, void *d_ptr);
int mrcz_host_malloc(mrcz_ctx_t *ctx, void **h_ptr, uint64_t bytes); /* pinned */
int mrcz_host_free(mrcz_ctx_t *ctx, void *h_ptr);
int mrcz_copy_h2d(mrcz_ctx_t *ctx, void *d_dst, const void *h_src, uint64_t bytes);
int mrcz_copy_d2h(mrcz_ctx_t *ctx, void *h_dst, const void *d_src, uint64_t bytes);

/*
 * Asynchronous forms, for pipelines that overlap file I/O, PCIe copies and the codec (the chunk scheduler of
 * host/workers_gpu.c, which replaces the one-chunk-at-a-time loops of src/core/workers.c:779-855 and :592-672).
 * A context owns three HIP streams -- compute, upload, download -- and events order work across them:
 *
 *   mrcz_copy_h2d_async(c, MRCZ_STREAM_UPLOAD, d_in, h_pinned, n);  mrcz_event_record(c, MRCZ_STREAM_UPLOAD, up);
 *   mrcz_stream_wait_event(c, MRCZ_STREAM_COMPUTE, up);
 *   mrcz_compress_chunks_async(c, d_in, nfloats, first_chunk, bits, d_rec, cap, h_res5);
 *   mrcz_event_record(c, MRCZ_STREAM_COMPUTE, done);   ...   mrcz_event_sync(c, done);   // h_res5[0] = bytes written
 *
 * Nothing here blocks the host except mrcz_event_sync.  Result words are written to PINNED host memory
 * (mrcz_host_malloc) in stream order: compress h_result5 = { bytes written, plane_bytes[4] }, uncompress h_result3 =
 * { record bytes consumed, error count (non-zero = MRCZ_EFORMAT), streams decoded sequentially }.  Calls on one
 * context must be issued by one thread at a time (the workspace is reused in stream order).
 */
#define MRCZ_STREAM_COMPUTE 0
#define MRCZ_STREAM_UPLOAD 1
#define MRCZ_STREAM_DOWNLOAD 2
typedef struct mrcz_event mrcz_event_t;
int mrcz_event_create(mrcz_ctx_t *ctx, mrcz_event_t **ev);
void mrcz_event_destroy(mrcz_ctx_t *ctx, mrcz_event_t *ev);
int mrcz_event_record(mrcz_ctx_t *ctx, int stream_id, mrcz_event_t *ev);      /* ev = everything enqueued so far on that stream */
int mrcz_stream_wait_event(mrcz_ctx_t *ctx, int stream_id, mrcz_event_t *ev); /* later work of that stream starts after ev */
int mrcz_event_sync(mrcz_ctx_t *ctx, mrcz_event_t *ev);                       /* the host waits for ev */
int mrcz_copy_h2d_async(mrcz_ctx_t *ctx, int stream_id, void *d_dst, const void *h_src, uint64_t bytes);
int mrcz_copy_d2h_async(mrcz_ctx_t *ctx, int stream_id, void *h_dst, const void *d_src, uint64_t bytes);
int mrcz_compress_chunks_async(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int bits,
                               void *d_out, uint64_t out_cap, uint64_t *h_result5);
int mrcz_uncompress_chunks_async(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats, uint32_t chk,
                                 void *d_out, uint64_t *h_result3);

/*
 * "-s int" mode of the reference (src/core/workers.c:125-175 encode, :444-511 decode; selected by `mrc_tar -s int`,
 * call sites workers.c:782-787, 604-609, 646-650).  Encode: every word past the file's first 256 is replaced by
 * (char)round(x) in its low byte (upper bytes zero), then the same plane split / DEFLATE / container; the mask level
 * plays no role.  Decode: the same container, then word = (float)(signed char) of its plane-0 byte past the header
 * words.  The container does not record the mode: the caller must ask for it again, as with the reference.
 */
int mrcz_compress_chunks_int8(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk,
                              void *d_out, uint64_t out_cap, uint64_t *out_len, uint64_t plane_bytes[4]);
int mrcz_uncompress_chunks_int8(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats, uint32_t chk,
                                uint64_t first_chunk, void *d_out, uint64_t *consumed);
int mrcz_compress_chunks_int8_async(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk,
                                    void *d_out, uint64_t out_cap, uint64_t *h_result5);
int mrcz_uncompress_chunks_int8_async(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats, uint32_t chk,
                                      uint64_t first_chunk, void *d_out, uint64_t *h_result3);

/*
 * Absolute-error mode: every decoded float lies within eps of the original (|x - x'| <= eps in exact arithmetic), with as
 * many low bits zeroed per word as that bound allows.  eps is a float32, finite and > 0 (else MRCZ_EINVAL); a caller that
 * holds a double converts it toward zero, so that the bound also holds for the value it was given.  With
 * q = floor(log2(eps)) and E = bits(eps), every word w past the file's first 256 (as -b treats them) becomes:
 *   e = (w >> 23) & 0xff == 0xff (Inf, NaN)   w
 *   mag = w & 0x7fffffff <= E (|x| <= eps)    0 (+0.0)
 *   otherwise                                 b = clamp(q - (max(e, 1) - 150) + 1, 0, 23);
 *                                             r = (mag + (b ? 1 << (b - 1) : 0)) & ~((1 << b) - 1)   (nearest, ties away from 0)
 *                                             r >= 0x7f800000 (would round to Inf): r = mag & ~((1 << (b - 1)) - 1);
 *                                             (w & 0x80000000) | r
 * then the same plane split / DEFLATE / container as bits = 0.  Nothing is recorded in the container and nothing is needed
 * to decode it: every decoder (mrcz_uncompress_chunks, range, boxes, binned, the reference's reader) returns the rounded
 * words.  mrcz_erase_abs applies the same rounding in place to words [256, nwords) of a file (d_words holds words
 * first_word_index ..): the expected decode, as mrcz_erase_bits is for bits.
 */
int mrcz_compress_chunks_abs(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, float eps,
                             void *d_out, uint64_t out_cap, uint64_t *out_len, uint64_t plane_bytes[4]);
int mrcz_compress_chunks_abs_async(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, float eps,
                                   void *d_out, uint64_t out_cap, uint64_t *h_result5);
int mrcz_erase_abs(mrcz_ctx_t *ctx, void *d_words, uint64_t nwords, uint64_t first_word_index, float eps);

/*
 * Range decode: words [w0, w1) of a file without decoding the rest.  Nothing in the container changes: every chunk record
 * starts with a 16-byte header holding its four payload lengths, so where chunk c's record begins follows from the headers
 * of chunks 0 .. c-1 alone, and the chunks decode independently.  Only the chunks that cover the window are decoded (whole),
 * and only the window's words are merged back into floats.
 *   mrcz_record_size      bytes of one chunk record (header included) from its 16-byte header, for a chunk of n floats;
 *                         MRCZ_EFORMAT for lengths no record of such a chunk can have
 *   mrcz_records_index    (host memory) byte offset, from the first record, of every chunk record of a file of nfloats floats
 *                         in chunks of chk: offsets[0 .. nchunks], offsets[nchunks] = end of the last record.  Reads 16 bytes
 *                         per chunk; MRCZ_EFORMAT if the records end early
 *   mrcz_uncompress_range d_records/len = the records of chunks first_chunk, first_chunk + 1, ... of a file of nfloats_file
 *                         floats (first_chunk <= w0 / chk; records before the window's first chunk are only walked);
 *                         d_out (16-byte aligned) receives the w1 - w0 words; int_mode = the "-s int" decode
 *                         (mrcz_uncompress_chunks_int8).  mrcz_set_ztypes applies.  w0 >= w1, w1 > nfloats_file or
 *                         first_chunk past the window: MRCZ_EINVAL; records that end before the window's last chunk:
 *                         MRCZ_EFORMAT (never read past len).  consumed = bytes of d_records up to the end of the last
 *                         record decoded.
 */
int mrcz_record_size(const void *h_header16, uint32_t n, uint64_t *bytes);
int mrcz_records_index(const void *h_records, uint64_t len, uint64_t nfloats, uint32_t chk, uint64_t *offsets);
int mrcz_uncompress_range(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                          uint64_t first_chunk, uint64_t w0, uint64_t w1, void *d_out, int int_mode, uint64_t *consumed);
int mrcz_uncompress_range_async(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                                uint64_t first_chunk, uint64_t w0, uint64_t w1, void *d_out, int int_mode, uint64_t *h_result3);

/*
 * Box decode: a batch of equal-sized boxes (particle sub-volumes) of a float32 volume, decoding only the chunks the boxes touch.
 * The volume is nx x ny x nz words starting at file word data_word0 (an MRC file: 256 + nsymbt / 4); voxel (x, y, z) is file
 * word data_word0 + (z * ny + y) * nx + x.  Box i has origin (corner) (x0, y0, z0) = origins[3 i .. 3 i + 2]; output word
 * [i][k][j][l] (nboxes x bz x by x bx words) is voxel (x0 + l, y0 + j, z0 + k), or fill_bits where that voxel lies outside the
 * volume.  Boxes may overlap each other and may lie partly or wholly outside the volume.
 *   mrcz_box_origins      (host) origins of boxes centred on centres[3 i .. 3 i + 2] (x, y, z, as particle pickers write
 *                         them): round(c) - size / 2 per axis, round(v) = floor(v + 0.5).  MRCZ_EINVAL for a centre that is
 *                         not finite or an origin outside int32
 *   mrcz_boxes_chunks     (host) covered[c] = 1 iff an in-volume voxel of some box lies in chunk c, else 0, for every chunk
 *                         c < ceil(nfloats_file / chk)
 *   mrcz_uncompress_boxes d_records/len = the records of chunks [first_chunk, first_chunk + nchunks) of the file (d_records
 *                         may be NULL when nchunks = 0).  Writes every box voxel that lies in those chunks, and every
 *                         out-of-volume voxel, into d_out (16-byte aligned); leaves every other voxel untouched, so one call
 *                         per run of covered chunks gives what one call over the whole span gives.  Covered chunks are
 *                         decoded once, the others only walked (16-byte header).  int_mode and mrcz_set_ztypes apply as in
 *                         range decode.  MRCZ_EINVAL: a zero size, a volume that does not fit in nfloats_file, a NULL
 *                         pointer, first_chunk + nchunks past the file; MRCZ_EFORMAT: records that end before the last
 *                         chunk's record does (never read past len).  chunks_decoded (optional) = covered chunks decoded.
 *                         nboxes = 0 does nothing.  Synchronous.
 */
typedef struct mrcz_box_geom {
    uint64_t data_word0;  /* file word of voxel (0, 0, 0) */
    uint32_t nx, ny, nz;  /* volume, each >= 1 */
    uint32_t bx, by, bz;  /* box size, each >= 1 */
    uint32_t fill_bits;   /* word written for out-of-volume voxels */
} mrcz_box_geom_t;
int mrcz_box_origins(const mrcz_box_geom_t *g, const double *h_centers, uint32_t nboxes, int32_t *h_origins);
int mrcz_boxes_chunks(const mrcz_box_geom_t *g, const int32_t *h_origins, uint32_t nboxes, uint64_t nfloats_file, uint32_t chk,
                      uint8_t *covered);
int mrcz_uncompress_boxes(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                          uint64_t first_chunk, uint64_t nchunks, const mrcz_box_geom_t *g, const int32_t *h_origins,
                          uint32_t nboxes, void *d_out, int int_mode, uint64_t *chunks_decoded);

/*
 * Binned decode: a float32 volume average-pooled by (fx, fy, fz), decoded chunk by chunk without a buffer of the volume's size.
 * The volume is as in box decode (voxel (x, y, z) = file word data_word0 + (z * ny + y) * nx + x).  The output is
 * mz x my x mx = (nz / fz) x (ny / fy) x (nx / fx) float32 (integer division: the voxels of a trailing remainder of any axis
 * are ignored).  Output voxel (X, Y, Z) is the mean of its fx * fy * fz voxels: they are widened to double and added in file
 * order (z, then y, then x), the sum starting from the first voxel; then (float)(sum / (double)(fx * fy * fz)).  So factor
 * (1, 1, 1) gives back every non-NaN word bit for bit, and the result does not depend on how the chunks are cut into calls.
 *   mrcz_bin_chunks         (host) chunks [c0, c1) hold the used voxels: from the chunk of the first to the chunk of the last
 *   mrcz_uncompress_binned  d_records/len = the records of chunks [first_chunk, first_chunk + nchunks) of the file.  Chunks
 *                           of [c0, c1) among them are decoded once, in runs of up to max_batch_chunks, and their voxels
 *                           folded into d_acc (mz * my * mx doubles, the caller's, 16-byte aligned: the partial sums); the
 *                           other chunks are only walked (16-byte header).  int_mode and mrcz_set_ztypes apply as in range
 *                           decode.  chunks_decoded (optional) = chunks decoded.  Synchronous.
 *   mrcz_binned_finish      d_out[i] = (float)(d_acc[i] / (fx * fy * fz)), mz * my * mx floats.  Synchronous.
 * Contract: a binned volume is one or more mrcz_uncompress_binned calls that together cover [c0, c1) in increasing chunk order,
 * each chunk once, then one mrcz_binned_finish.  d_acc needs no zeroing (a bin's first voxel assigns its sum); between the
 * calls it must be left alone.  MRCZ_EINVAL: a factor of 0 or larger than its dimension, a volume that does not fit in
 * nfloats_file, a bin of more than 2^31 voxels, a NULL pointer, first_chunk + nchunks past the file; MRCZ_EFORMAT: records that
 * end before the last chunk's record does (never read past len).
 */
typedef struct mrcz_bin_geom {
    uint64_t data_word0;  /* file word of voxel (0, 0, 0) */
    uint32_t nx, ny, nz;  /* volume, each >= 1 */
    uint32_t fx, fy, fz;  /* bin factors, 1 <= f <= dimension */
} mrcz_bin_geom_t;
int mrcz_bin_chunks(const mrcz_bin_geom_t *g, uint64_t nfloats_file, uint32_t chk, uint64_t *c0, uint64_t *c1);
int mrcz_uncompress_binned(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                           uint64_t first_chunk, uint64_t nchunks, const mrcz_bin_geom_t *g, double *d_acc,
                           int int_mode, uint64_t *chunks_decoded);
int mrcz_binned_finish(mrcz_ctx_t *ctx, const mrcz_bin_geom_t *g, const double *d_acc, float *d_out);

/*
 * Compare decode: how well a container reproduces its original, decoded chunk by chunk without a buffer of the volume's size and
 * without writing the decoded words anywhere.  Per data word (file word >= 256), with a the original and b the decoded word
 * read as float32:  d = (double)b - (double)a,  err = |d|,  rel = |(double)a| > 1e-3 ? err / |(double)a| : 0  (the rule of the
 * reference's QA tool, src/tool/erroranalysis.c, in double).  Each is one correctly rounded IEEE operation.  A point counts in
 * the error fields when a and b are both finite; words where either is NaN or +-Inf are compared by bit pattern.  err > eps_abs
 * and rel > eps_rel are strict; a bound that is negative or NaN switches its check off.  The 256 header words are compared by
 * bit pattern alone.
 *   mrcz_uncompress_compare  d_records/len = the records of chunks [first_chunk, first_chunk + nchunks) of a file of nfloats_file
 *                            words; d_orig (16-byte aligned, device) = the original's words of exactly those chunks:
 *                            min(nchunks * chk, nfloats_file - first_chunk * chk) words.  The chunks are decoded once, in runs
 *                            of up to max_batch_chunks, and chunk c's summary is assigned to d_acc[c] (absolute chunk number:
 *                            d_acc is the caller's, ceil(nfloats_file / chk) records, device, needs no zeroing).  int_mode and
 *                            mrcz_set_ztypes apply as in binned decode.  Synchronous.
 *   mrcz_compare_finish      folds d_acc[first_chunk .. first_chunk + nchunks) into *h_total (host memory): counts added, maxima
 *                            with the lowest index on ties, first_over the minimum, the sums added in increasing chunk order
 *                            in double, starting from the first chunk's value.  nchunks == 0 gives the summary of no words.
 * Contract: a file is one or more mrcz_uncompress_compare calls that cover its chunks, in any order, each chunk once, each with
 * its own slice of the original (so a file larger than device memory streams through), then one mrcz_compare_finish.  The bits
 * of d_acc[c], the sums included, depend on chunk c's words and the bounds only: not on max_batch_chunks, on how the chunks are
 * split over calls, or on first_chunk (the order in which a chunk's points are added is fixed by their place in the chunk; no
 * atomics).  MRCZ_EINVAL: a NULL pointer, a misaligned d_orig, first_chunk + nchunks past the file; MRCZ_EFORMAT: chk of 0 or
 * above MRCZ_CHUNK_FLOATS, malformed streams, records that end before the last chunk's record does (never read past len).
 * nchunks == 0 is MRCZ_OK and touches nothing.
 */
typedef struct mrcz_compare {       /* one chunk's summary, or a whole file's */
    uint64_t n;               /* data words compared: file words >= 256 of the chunk */
    uint64_t n_header_diff;   /* file words < 256 whose bit patterns differ */
    uint64_t n_diff;          /* data words whose bit patterns differ */
    uint64_t n_finite;        /* data words where original and decoded are both finite: the points of all fields below */
    uint64_t n_special_diff;  /* data words where either is NaN or +-Inf and the bit patterns differ */
    uint64_t n_over_abs;      /* finite points with err > eps_abs */
    uint64_t n_over_rel;      /* finite points with rel > eps_rel */
    uint64_t first_over;      /* lowest file word index counted in n_over_abs, n_over_rel or n_special_diff; UINT64_MAX: none */
    uint64_t max_err_index;   /* lowest file word index that attains max_err; UINT64_MAX when n_finite == 0 */
    uint64_t max_rel_index;   /* likewise for max_rel */
    double   max_err, max_rel;                    /* 0 when n_finite == 0 */
    double   sum_err, sum_abs_err, sum_err2;      /* sums of d, |d|, d * d */
    double   orig_min, orig_max, orig_sum, orig_sum2;  /* of the original at the finite points; +Inf / -Inf / 0 / 0 when none */
} mrcz_compare_t;
int mrcz_uncompress_compare(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                            uint64_t first_chunk, uint64_t nchunks, const void *d_orig, double eps_abs, double eps_rel,
                            int int_mode, mrcz_compare_t *d_acc);
int mrcz_compare_finish(mrcz_ctx_t *ctx, const mrcz_compare_t *d_acc, uint64_t first_chunk, uint64_t nchunks,
                        mrcz_compare_t *h_total);

/*
 * Digest decode: the standard CRC-32 (zlib, gzip, PNG, crc32(1): reflected polynomial 0xEDB88320, initial value and final xor
 * 0xFFFFFFFF) of the bytes a container decodes to, per chunk and for the file, decoded chunk by chunk without a buffer of the
 * volume's size and without writing the decoded words anywhere.  The container holds no checksum; this is the fixity check of an
 * archive whose original is gone.  Chunk c's digest is zlib.crc32 of its decoded words as the file holds them (little-endian,
 * 4 n_c bytes); the file's digest is zlib.crc32 of all floor(fsz / 4) words, i.e. of the restored file.
 *   mrcz_crc32_combine      crc32(A || B) from crc32(A), crc32(B) and |B| in bytes (any 64-bit count).  Pure host arithmetic:
 *                           no context, no GPU.
 *   mrcz_uncompress_digest  d_records/len = the records of chunks [first_chunk, first_chunk + nchunks) of a file of nfloats_file
 *                           words.  The chunks are decoded once, in runs of up to max_batch_chunks, and chunk c's digest is
 *                           assigned to d_acc[c] (absolute chunk number: d_acc is the caller's, ceil(nfloats_file / chk)
 *                           records, device, needs no zeroing).  int_mode and mrcz_set_ztypes apply as in compare decode.
 *                           Synchronous.
 *   mrcz_digest_words       the same records for words that are already on the device: d_words (16-byte aligned) holds the
 *                           file's words from chunk first_chunk on, nwords of them, in chunks of chk.  xform = MRCZ_DIGEST_NONE:
 *                           the CRC-32 of the words as they are (a plain file).  MRCZ_DIGEST_MASK (bits, 0..32), MRCZ_DIGEST_ABS
 *                           (eps, as mrcz_compress_chunks_abs) and MRCZ_DIGEST_INT8: the digest of what a container written
 *                           from these words by mrcz_compress_chunks / _abs / _int8 WILL decode to (file words < 256 keep their
 *                           bits, as there), without compressing or decoding anything: the value to record when the archive is
 *                           made.  Synchronous; mrcz_digest_words_async enqueues on the compute stream and returns.
 *   mrcz_digest_finish      copies d_acc[first_chunk .. first_chunk + nchunks) once and combines the records on the host in chunk
 *                           order into *h_total (host memory); h_total->nbytes is the sum.  nchunks == 0 gives { 0, 0, 0 }, the
 *                           CRC-32 of no bytes.
 * Contract: as compare decode.  A file is one or more mrcz_uncompress_digest calls that cover its chunks, in any order, each
 * chunk once, then one mrcz_digest_finish.  CRC is exact arithmetic: the bits of d_acc[c] depend on chunk c's decoded words only.
 * MRCZ_EINVAL: a NULL pointer, a misaligned pointer, first_chunk + nchunks past the file, an unknown xform, bits outside 0..32, an
 * eps that is not finite and > 0, (digest_words) chk of 0 or above MRCZ_CHUNK_FLOATS; MRCZ_EFORMAT: (uncompress_digest) chk of 0
 * or above MRCZ_CHUNK_FLOATS, malformed streams, records that end before the last chunk's record does (never read past len).
 * nchunks == 0 / nwords == 0 is MRCZ_OK and touches nothing.
 */
#define MRCZ_DIGEST_NONE 0
#define MRCZ_DIGEST_MASK 1
#define MRCZ_DIGEST_INT8 2
#define MRCZ_DIGEST_ABS 3
typedef struct mrcz_digest {  /* one chunk's digest, or a whole file's */
    uint32_t crc32;
    uint32_t reserved;        /* 0 */
    uint64_t nbytes;          /* bytes digested */
} mrcz_digest_t;
uint32_t mrcz_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t nbytes_b);
int mrcz_uncompress_digest(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                           uint64_t first_chunk, uint64_t nchunks, int int_mode, mrcz_digest_t *d_acc);
int mrcz_digest_words(mrcz_ctx_t *ctx, const void *d_words, uint64_t nwords, uint64_t first_chunk, uint32_t chk, int xform,
                      int bits, float eps, mrcz_digest_t *d_acc);
int mrcz_digest_words_async(mrcz_ctx_t *ctx, const void *d_words, uint64_t nwords, uint64_t first_chunk, uint32_t chk, int xform,
                            int bits, float eps, mrcz_digest_t *d_acc);
int mrcz_digest_finish(mrcz_ctx_t *ctx, const mrcz_digest_t *d_acc, uint64_t first_chunk, uint64_t nchunks,
                       mrcz_digest_t *h_total);

/*
 * Probe: what a compress setting costs and what it buys, before the first container exists.  For words that are on the device and
 * one setting it gives the exact size of the records and the error summary of what they would decode to, without writing, decoding
 * or allocating anything of the volume's size: the compressor's sizing passes (everything up to the payload lengths) run, the
 * layout and emit passes do not, and the error is folded over the original's words and the transform alone.
 *   mrcz_probe_chunks  d_in (16-byte aligned, only read) = nfloats words that start a chunk boundary of a file, first_chunk as in
 *                      mrcz_compress_chunks.  xform = MRCZ_PROBE_MASK (bits, 0..32), MRCZ_PROBE_ABS (eps, as
 *                      mrcz_compress_chunks_abs) or MRCZ_PROBE_INT8.  *out_len and plane_bytes (optional) are exactly what
 *                      mrcz_compress_chunks / _abs / _int8 return for the same arguments: record bytes, without the 17-byte file
 *                      header.  d_acc (optional, device, 8-byte aligned, needs no zeroing) receives record first_chunk + i for
 *                      chunk i of d_in: the mrcz_compare_t that mrcz_uncompress_compare would assign for the container written
 *                      with that setting, compared against d_in with the bounds eps_abs and eps_rel (negative or NaN: off).
 *                      Counts, extremes, indices, orig_min and orig_max are equal; the sums follow the same definition and the same
 *                      order of addition.  The bits of d_acc[c] depend on chunk c's words and the setting only: not on
 *                      max_batch_chunks, on how a file is cut into calls, or on first_chunk.  mrcz_compare_finish folds the
 *                      records.  Synchronous; mrcz_probe_chunks_async enqueues on the compute stream, h_result5 as
 *                      mrcz_compress_chunks_async.  A later compress call on the context is not disturbed.
 * MRCZ_EINVAL: an unknown xform, bits outside 0..32, an eps that is not finite and > 0, a NULL or misaligned d_in, a misaligned
 * d_acc, a NULL out_len.  nfloats == 0 is MRCZ_OK with *out_len = 0 and touches nothing.
 */
#define MRCZ_PROBE_MASK 0
#define MRCZ_PROBE_ABS 1
#define MRCZ_PROBE_INT8 2
int mrcz_probe_chunks(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int xform, int bits, float eps,
                      double eps_abs, double eps_rel, mrcz_compare_t *d_acc, uint64_t *out_len, uint64_t plane_bytes[4]);
int mrcz_probe_chunks_async(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int xform, int bits, float eps,
                            double eps_abs, double eps_rel, mrcz_compare_t *d_acc, uint64_t *h_result5);

/*
 * Top-planes decode: every word of a run of chunks at reduced precision, the low byte planes neither read nor decoded.  A chunk
 * record is its 16-byte header (the four payload lengths) followed by the payloads of byte planes 0, 1, 2, 3 of the chunk's words;
 * plane 3 is the sign and seven exponent bits of a float32, plane 2 its last exponent bit and top seven mantissa bits.  keep = 2
 * or 3 is the number of top planes kept, mask(keep) = 0xFFFFFFFF << 8 (4 - keep).  For every word of the chunks asked for, file
 * words 0 .. 255 included, the result is (what mrcz_uncompress_chunks returns) & mask(keep), exactly; nothing else is promised:
 *   - keep = 2 is the bfloat16 TRUNCATION of the float32 (toward zero; torch's .to(bfloat16) rounds to nearest): the relative
 *     error is below 2^-7 (keep 2) or 2^-15 (keep 3) for normal numbers;
 *   - NaN payload bits of the dropped planes are lost: a NaN whose only set mantissa bits were there becomes +-Inf;
 *   - the 256 header words are truncated like the rest (two planes cannot restore them): read the MRC header by range decode;
 *   - "-s int" containers keep their data in plane 0: there is no int_mode.  mrcz_set_ztypes applies to the kept planes.
 *   mrcz_record_top_span  (host arithmetic, the checks of mrcz_record_size on all four lengths) for the record of a chunk of n
 *                         floats whose 16-byte header is h_header16: skip = offset inside the record of the first kept payload
 *                         (16 + the lengths of the dropped planes), bytes = total length of the kept payloads.  MRCZ_EINVAL: a
 *                         NULL pointer, keep outside {2, 3}; MRCZ_EFORMAT: lengths no record of such a chunk can have.
 *   thinned record        the record's 16-byte header, unchanged, directly followed by its kept payloads: what a reader that
 *                         fetches [record + skip, record + skip + bytes) behind the header holds.
 *   mrcz_uncompress_top   d_records/len = the records of chunks [first_chunk, first_chunk + nchunks) of a file of nfloats_file
 *                         words: ordinary records (the dropped payloads are stepped over by their lengths, never read) or, with
 *                         MRCZ_TOP_THINNED, thinned records.  The chunks are decoded in runs of up to max_batch_chunks and their
 *                         words written contiguously to d_out (16-byte aligned): min(nchunks * chk, nfloats_file - first_chunk *
 *                         chk) elements, uint32 (MRCZ_TOP_F32: the dropped planes' bytes zero) or uint16 = word >> 16
 *                         (MRCZ_TOP_U16, keep 2 only: the bfloat16 bit pattern).  consumed (optional) = bytes of d_records
 *                         walked.  Synchronous; mrcz_uncompress_top_async enqueues on the compute stream, h_result3 as
 *                         mrcz_uncompress_chunks_async.
 * MRCZ_EINVAL: keep outside {2, 3}, MRCZ_TOP_U16 with keep 3, unknown flag bits, a NULL or misaligned pointer (d_records may be
 * NULL when nchunks == 0), first_chunk + nchunks past the file; MRCZ_EFORMAT: chk of 0 or above MRCZ_CHUNK_FLOATS, a header
 * length no record can have, malformed kept streams, records that end early (never read past len).  A malformed DROPPED payload
 * is by design no error: it is never looked at.  nchunks == 0 is MRCZ_OK and touches nothing.
 */
#define MRCZ_TOP_F32 0
#define MRCZ_TOP_U16 1
#define MRCZ_TOP_THINNED 4
int mrcz_record_top_span(const void *h_header16, uint32_t n, int keep, uint64_t *skip, uint64_t *bytes);
int mrcz_uncompress_top(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                        uint64_t first_chunk, uint64_t nchunks, int keep, int flags, void *d_out, uint64_t *consumed);
int mrcz_uncompress_top_async(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                              uint64_t first_chunk, uint64_t nchunks, int keep, int flags, void *d_out, uint64_t *h_result3);

/* apply_mask alone on device (the erasebytes restatement used by the GPU-side verification tools,
 * src/tool/erasebytes.c:109-134): words [256, nwords) of a file &= mask(bits).  In place. */
int mrcz_erase_bits(mrcz_ctx_t *ctx, void *d_words, uint64_t nwords, uint64_t first_word_index, int bits);

/*
 * erroranalysis on the device (the reference's QA tool src/tool/erroranalysis.c:188-219,347-495: absolute and relative error of
 * every point of a decoded file against the original, the K worst points).  The device selects; the ordering rules of the
 * reference (topK, erroranalysis.c:61-91) run on the host over the handful of points that can matter.
 *   mrcz_err_hist     histogram of the error keys (bit pattern of fabsf(n2 - n1); NaN = 0xffffffff) of n points: pass 0 bins key
 *                     bits 31..21, pass 1 bits 20..10 of the points whose bits 31..21 == prefix, pass 2 bits 9..0 of the points
 *                     whose bits 31..10 == prefix.  Accumulates across calls (a file in batches) until `reset`; hist (host,
 *                     2048 x u64, optional) receives the running histogram.  Three passes give the K-th largest key exactly.
 *   mrcz_err_collect  appends every point with key >= threshold_bits to d_points (16-byte records {u64 index, u32 n1, u32 n2},
 *                     device memory, cap_points records) starting at record count_in; returns the new count (it may exceed the
 *                     capacity: only the first cap_points records are stored).
 */
int mrcz_err_hist(mrcz_ctx_t *ctx, const void *d_orig, const void *d_dec, uint64_t n, int pass, uint32_t prefix, int reset,
                  uint64_t hist[2048]);
int mrcz_err_collect(mrcz_ctx_t *ctx, const void *d_orig, const void *d_dec, uint64_t n, uint64_t base_index, uint32_t threshold_bits,
                     void *d_points, uint64_t cap_points, uint64_t count_in, uint64_t *count_out);

/* Synthetic benchmark volumes generated on the device: words [first_index, first_index + nwords) of the integer generator
 * of SURVEY.md Appendix D (the known-answer inputs of the reference's containers; tests/util.py kat_words).  Lets a 64 GiB
 * volume exist without a host copy.  Synchronous. */
int mrcz_generate_kat_words(mrcz_ctx_t *ctx, void *d_words, uint64_t first_index, uint64_t nwords);

/* When on, every kernel launch is bracketed by HIP events on the context's stream (adds a host
 * synchronisation per launch: use for profiling, not for throughput runs). */
int mrcz_set_timing(mrcz_ctx_t *ctx, int on);

/* per-kernel elapsed milliseconds of the last compress / uncompress call (HIP events on the
 * context's stream); names are returned through `names` (static strings).  Returns count. */
int mrcz_last_timings(const mrcz_ctx_t *ctx, const char **names, float *ms, int max);

/* Inspection (tests): copy the block table of the last compressed batch to the host.
 * For stream s (= 4*chunk + plane) fills up to max_blocks entries; returns number of blocks. */
typedef struct {
    uint32_t start, end;  /* byte span of the block in the plane */
    uint32_t btype;       /* 0 stored, 1 static, 2 dynamic */
    uint32_t opt_len, static_len;
    uint32_t bitpos;      /* first bit of the block inside the plane's deflate stream */
} mrcz_block_info_t;
int mrcz_debug_blocks(mrcz_ctx_t *ctx, uint32_t stream, mrcz_block_info_t *blocks, uint32_t max_blocks);

/* Inspection (tests): number of streams of the last synchronous uncompress call (chunks, range or
 * boxes) that the parallel decoder handed to the sequential general-distance decoder (0 for streams
 * this codec or zlib Z_RLE wrote), and of streams decoded block after block because their block
 * chain did not close in parallel (a superset of the former).  Both are latched when the call
 * returns: a later compress call does not change them. */
int64_t mrcz_debug_fallbacks(const mrcz_ctx_t *ctx);
int64_t mrcz_debug_chain_fallbacks(mrcz_ctx_t *ctx);

/* Inspection (tests): tile parts of the last compress call whose coded bits exceeded the emit kernel's
 * staging buffer and were emitted in two halves (-1 on error). */
int64_t mrcz_debug_emit_splits(mrcz_ctx_t *ctx);

/* Inspection (profiling): enable/disable the in-kernel phase counters of the parallel inflate and
 * (if out != NULL) read the 20 counters of `stream` from the last call (shader clocks of thread 0):
 * [0] header+tables [1] staging [2] exit functions [3] composition [4] count walk [5] scans
 * [6] literal scatter walk [7] wait for the slowest wave [8] fill + flush [9] - [10] blocks
 * [11] windows [12..16] header sub-phases (first bits, code-length code, length decode, literal
 * table, distance table). */
int mrcz_debug_inflate_phases(mrcz_ctx_t *ctx, int enable, uint32_t stream, uint64_t out[20]);
/* (enable = 3 switches on the phase clocks of the Huffman construction kernel instead: out[0..7] of stream 0 = the slowest
 * tree's clocks per phase, out[16..19] of stream 0 and out[0..3] of stream 1 = their sums, out[12] of stream 1 = trees;
 * tests/tools_huff_profile.py prints them.  enable = 4 switches on k_chain's shader-clock stamps instead: 8 per stream, stream
 * s's at flat counter 8 s (out of `stream` k holds flat counters 20 k .. 20 k + 19); tools/jobs/chain_validate_phases.py
 * prints them.) */

/* Inspection (profiling): block-start candidates of the last batch of the last mrcz_uncompress_chunks call:
 * out[0] = positions that passed the signature scan and went to header validation, out[1] = validated candidates. */
int mrcz_debug_candidates(mrcz_ctx_t *ctx, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* MRCZ_HIP_H_ */
