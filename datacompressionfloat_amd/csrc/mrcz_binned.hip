/*
 * mrcz_binned.hip -- binned decode (include/mrcz_hip.h, mrcz_uncompress_binned): an average-pooled (fx x fy x fz) float32 volume
 * out of the chunk records, streaming the chunks through a context of fixed size.
 *
 * Included from mrcz_api.hip after the box decode (it uses the context, decode_batch, the staging buffer and walk_chunks there).
 * Per run of up to max_chunks consecutive chunks of [c0, c1) (mrcz_bin_chunks): decode_batch, k_merge_segments<false> into the
 * staging buffer, then k_bin_fold adds the run's file words [B0, B1) to the float64 partial sums of the bins (d_acc, one per
 * output voxel).  Other chunks are only walked (k_parse_records).  mrcz_binned_finish divides and narrows (k_binned_finish).
 *
 * The fold is sequential per bin and in file order: one thread owns one bin, reads its partial sum once, adds every voxel of
 * its rows that lies in [B0, B1) (a row is fx contiguous words) and writes the sum back once.  A bin's voxels in raster order
 * (k, j, l) are its voxels in file order, and the runs come in file order, so the sum is the same however the chunks are cut
 * into runs and calls.  The bin's first voxel starts the sum: the fold starts from -0.0, for which -0.0 + v == v for every v.
 */

namespace mrcz {

/* The bins (X, Y, Z) with Y in [y0, y0 + ny_run) and Z in [z0, ...), t = ((Z - z0) * ny_run + Y - y0) * mx + X, fold every one
 * of their voxels that lies in the file words [B0, B1) (= stage[0, B1 - B0)) into acc[(Z * my + Y) * mx + X]. */
__global__ __launch_bounds__(256) void k_bin_fold(const uint32_t *__restrict__ stage, uint64_t B0, uint64_t B1, mrcz_bin_geom_t g,
                                                  uint32_t mx, uint32_t my, uint32_t y0, uint32_t ny_run, uint32_t z0, uint64_t nbins,
                                                  double *__restrict__ acc)
{
    const uint64_t nx = g.nx, sec = nx * g.ny;
    /* sections [sa, sb) of the volume meet [B0, B1) (the host launches only when the run meets the used voxels) */
    const uint64_t sa = B0 > g.data_word0 ? (B0 - g.data_word0) / sec : 0, sb = (B1 - g.data_word0 + sec - 1u) / sec;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < nbins; t += (uint64_t)gridDim.x * 256u) {
        const uint64_t row = t / mx;
        const uint32_t X = (uint32_t)(t - row * mx), Y = y0 + (uint32_t)(row % ny_run), Z = z0 + (uint32_t)(row / ny_run);
        const uint64_t b = ((uint64_t)Z * my + Y) * mx + X;
        const uint64_t x0 = (uint64_t)X * g.fx, ya0 = (uint64_t)Y * g.fy, za0 = (uint64_t)Z * g.fz;
        const uint64_t fw = g.data_word0 + (za0 * g.ny + ya0) * nx + x0; /* file word of the bin's first voxel */
        const uint64_t ka = za0 > sa ? za0 : sa, kb = za0 + g.fz < sb ? za0 + g.fz : sb;
        double s = fw >= B0 ? -0.0 : 0.0;
        bool touched = false;
        for (uint64_t z = ka; z < kb; z++) {
            const uint64_t zw = g.data_word0 + z * sec; /* file word of section z */
            /* rows [ra, rb) of z meet [B0, B1); only the run's first and last sections divide */
            const uint64_t ra = B0 > zw ? (B0 - zw) / nx : 0, rb = B1 - zw >= sec ? g.ny : (B1 - zw + nx - 1u) / nx;
            const uint64_t ja = ya0 > ra ? ya0 : ra, jb = ya0 + g.fy < rb ? ya0 + g.fy : rb;
            for (uint64_t y = ja; y < jb; y++) {
                const uint64_t rw = zw + y * nx + x0; /* file word of the row's first voxel */
                if (rw >= B1 || rw + g.fx <= B0) continue;
                const uint32_t la = B0 > rw ? (uint32_t)(B0 - rw) : 0u, lb = B1 - rw < g.fx ? (uint32_t)(B1 - rw) : g.fx;
                if (!touched) {
                    touched = true;
                    if (fw < B0) s = acc[b]; /* the bin began in an earlier run */
                }
                const float *p = reinterpret_cast<const float *>(stage) + (rw - B0);
                for (uint32_t l = la; l < lb; l++) s += (double)p[l];
            }
        }
        if (touched) acc[b] = s;
    }
}

/* out[i] = (float)(acc[i] / n) for the nbins output voxels: IEEE division and round-to-nearest narrowing */
__global__ __launch_bounds__(256) void k_binned_finish(const double *__restrict__ acc, uint64_t nbins, double n, float *__restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nbins; i += (uint64_t)gridDim.x * 256u) out[i] = (float)(acc[i] / n);
}

} /* namespace mrcz */

/* ---- host side ---- */

/* factors within the volume, the volume in the file, a bin of at most 2^31 voxels */
static bool bin_geom_ok(const mrcz_bin_geom_t *g)
{
    if (!g || !g->nx || !g->ny || !g->nz) return false;
    if (!g->fx || !g->fy || !g->fz || g->fx > g->nx || g->fy > g->ny || g->fz > g->nz) return false;
    return (uint64_t)g->fx * g->fy * g->fz <= 0x80000000ull;
}
static bool bin_fits(const mrcz_bin_geom_t *g, uint64_t nfloats_file)
{
    if (g->data_word0 > nfloats_file) return false;
    const uint64_t room = nfloats_file - g->data_word0, sec = (uint64_t)g->nx * g->ny;
    return sec <= room && g->nz <= room / sec;
}

/* the file words [*u0, *u1) from the first used voxel to the last one, inclusive of everything between */
static void bin_used_words(const mrcz_bin_geom_t *g, uint64_t *u0, uint64_t *u1)
{
    const uint64_t mx = g->nx / g->fx, my = g->ny / g->fy, mz = g->nz / g->fz;
    *u0 = g->data_word0;
    *u1 = g->data_word0 + ((mz * g->fz - 1u) * g->ny + my * g->fy - 1u) * g->nx + mx * g->fx;
}

extern "C" int mrcz_bin_chunks(const mrcz_bin_geom_t *g, uint64_t nfloats_file, uint32_t chk, uint64_t *c0, uint64_t *c1)
{
    if (!c0 || !c1 || chk == 0 || !bin_geom_ok(g) || !bin_fits(g, nfloats_file)) return MRCZ_EINVAL;
    uint64_t u0, u1;
    bin_used_words(g, &u0, &u1);
    *c0 = u0 / chk;
    *c1 = (u1 - 1u) / chk + 1u;
    return MRCZ_OK;
}

/* the bins whose voxels meet the file words [B0, B1): slabs [*za, *zb), and rows [*ya, *yb) of them; false if there are none */
static bool bin_run_bins(const mrcz_bin_geom_t *g, uint64_t B0, uint64_t B1, uint32_t *za, uint32_t *zb, uint32_t *ya, uint32_t *yb)
{
    const uint64_t my = g->ny / g->fy, mz = g->nz / g->fz, sec = (uint64_t)g->nx * g->ny, d0 = g->data_word0;
    const uint64_t end = d0 + mz * g->fz * sec;
    const uint64_t a = B0 > d0 ? B0 : d0, b = B1 < end ? B1 : end; /* the run's words in the used slabs */
    if (a >= b) return false;
    *za = (uint32_t)((a - d0) / sec / g->fz);
    *zb = (uint32_t)((b - 1u - d0) / sec / g->fz + 1u);
    *ya = 0;
    *yb = (uint32_t)my;
    const uint64_t s0 = (a - d0) / sec, s1 = (b - 1u - d0) / sec;
    if (s0 == s1) { /* the run covers part of one section: its rows */
        const uint64_t r0 = (a - d0 - s0 * sec) / g->nx, r1 = (b - 1u - d0 - s0 * sec) / g->nx;
        *ya = (uint32_t)(r0 / g->fy);
        *yb = (uint32_t)(r1 / g->fy + 1u < my ? r1 / g->fy + 1u : my);
        if (*ya >= *yb) return false; /* only rows of the y remainder */
    }
    return true;
}

static uint32_t grid_for(uint64_t n)
{
    const uint64_t blocks = (n + 255u) / 256u;
    return (uint32_t)(blocks < 65536u * 16u ? (blocks ? blocks : 1u) : 65536u * 16u);
}

static int uncompress_binned_enqueue(mrcz_ctx *ctx, const uint8_t *rec, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                     uint64_t nchunks, const mrcz_bin_geom_t *g, uint64_t c0, uint64_t c1, double *acc, int int_mode, uint64_t *decoded)
{
    hipStream_t lstream = ctx->stream;
    const uint32_t mx = g->nx / g->fx, my = g->ny / g->fy;
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    const uint64_t end = first_chunk + nchunks, d_lo = first_chunk > c0 ? first_chunk : c0, d_hi = end < c1 ? end : c1;
    uint64_t c = first_chunk;
    if (d_lo < d_hi) {
        if (int rc = walk_chunks(ctx, rec, len, nfloats_file, chk, c, d_lo)) return rc;
        for (c = d_lo; c < d_hi;) {
            const uint32_t nb = (uint32_t)((d_hi - c) < ctx->max_chunks ? (d_hi - c) : ctx->max_chunks);
            const uint64_t bbase = c * chk, bfl = (nfloats_file - bbase) < (uint64_t)nb * chk ? (nfloats_file - bbase) : (uint64_t)nb * chk;
            if (int rc = decode_batch(ctx, rec, len, bfl, nb, chk)) return rc;
            LAUNCH("k_merge_segments", k_merge_segments<false>, dim3(512, nb), dim3(256), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx,
                   bfl, chk, ctx->stage, len, (uint64_t)4 * ctx->row_chunks * CHK, int_mode ? 1u : 0u, bbase, (int64_t)0, (uint64_t)0);
            uint32_t za, zb, ya, yb;
            if (bin_run_bins(g, bbase, bbase + bfl, &za, &zb, &ya, &yb)) {
                const uint64_t nbins = (uint64_t)(zb - za) * (yb - ya) * mx;
                LAUNCH("k_bin_fold", k_bin_fold, dim3(grid_for(nbins)), dim3(256), ctx->stage, bbase, bbase + bfl, *g, mx, my, ya, yb - ya, za, nbins, acc);
            }
            *decoded += nb;
            c += nb;
        }
    }
    /* the chunks behind the last run are walked too: records that end before the span does are refused */
    if (int rc = walk_chunks(ctx, rec, len, nfloats_file, chk, c, end)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->h_result, ctx->result, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_binned(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                                      uint64_t first_chunk, uint64_t nchunks, const mrcz_bin_geom_t *g, double *d_acc, int int_mode,
                                      uint64_t *chunks_decoded)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chunks_decoded) *chunks_decoded = 0;
    if (!bin_geom_ok(g)) return fail(ctx, MRCZ_EINVAL, "bin factor zero or larger than its dimension, or a bin of more than 2^31 voxels", hipSuccess);
    if (!bin_fits(g, nfloats_file)) return fail(ctx, MRCZ_EINVAL, "volume outside the file", hipSuccess);
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EFORMAT, "chunk size in header exceeds CHUNK_SIZE (constant.h:25)", hipSuccess);
    const uint64_t nchunks_file = (nfloats_file + chk - 1) / chk;
    if (first_chunk > nchunks_file || nchunks > nchunks_file - first_chunk) return fail(ctx, MRCZ_EINVAL, "chunks past the end of the file", hipSuccess);
    if (!d_acc || (nchunks && !d_records)) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (nchunks == 0) return MRCZ_OK;
    if (int rc = uncompress_prepare(ctx, d_records, chk, d_acc)) return rc;
    if (!ctx->stage) { /* k_merge_segments<false> writes a batch's words here for k_bin_fold */
        hipError_t e = hipMalloc((void **)&ctx->stage, (size_t)ctx->max_chunks * CHK * 4u);
        if (e != hipSuccess) { ctx->stage = NULL; return fail(ctx, MRCZ_ENOMEM, "staging buffer", e); }
    }
    uint64_t c0, c1, decoded = 0;
    (void)mrcz_bin_chunks(g, nfloats_file, chk, &c0, &c1);
    int rc = uncompress_binned_enqueue(ctx, (const uint8_t *)d_records, len, nfloats_file, chk, first_chunk, nchunks, g, c0, c1, d_acc, int_mode, &decoded);
    if (rc == MRCZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MRCZ_EHIP, "stream sync (uncompress binned)", hipSuccess);
    if (rc != MRCZ_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    latch_fallbacks(ctx);
    if (ctx->h_result[1]) return fail(ctx, MRCZ_EFORMAT, "malformed chunk records or deflate stream", hipSuccess);
    if (chunks_decoded) *chunks_decoded = decoded;
    return MRCZ_OK;
}

extern "C" int mrcz_binned_finish(mrcz_ctx_t *ctx, const mrcz_bin_geom_t *g, const double *d_acc, float *d_out)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (!bin_geom_ok(g)) return fail(ctx, MRCZ_EINVAL, "bin factor zero or larger than its dimension, or a bin of more than 2^31 voxels", hipSuccess);
    if (!d_acc || !d_out) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t lstream = ctx->stream;
    const uint64_t nbins = (uint64_t)(g->nx / g->fx) * (g->ny / g->fy) * (g->nz / g->fz);
    const double n = (double)((uint64_t)g->fx * g->fy * g->fz);
    LAUNCH("k_binned_finish", k_binned_finish, dim3(grid_for(nbins)), dim3(256), d_acc, nbins, n, d_out);
    HIPCHK(hipStreamSynchronize(ctx->stream), "stream sync (binned finish)");
    return MRCZ_OK;
}
