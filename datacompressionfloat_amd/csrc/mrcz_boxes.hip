/*
 * mrcz_boxes.hip -- box decode (include/mrcz_hip.h, mrcz_uncompress_boxes): equal-sized boxes of a float32 volume out of the
 * chunk records, decoding each chunk that a box touches once and no other.
 *
 * Included from mrcz_api.hip after the range decode (it uses the context, decode_batch and the launch macros there).  Per run of
 * up to max_chunks consecutive covered chunks: decode_batch, k_merge_segments<false> into a staging buffer of max_chunks x CHK
 * words (the plane buffer cannot take the words: segments may point into it), then k_gather_boxes copies the box rows that lie
 * in the run's file words [B0, B1) from staging to the output.  Uncovered chunks are only walked (k_parse_records).  One
 * k_fill_boxes per call writes the fill word into every out-of-volume voxel.
 *
 * Rows (fixed box i, k, j: bx output words, contiguous in the file and in the output) are the unit of both kernels.  A
 * workgroup takes one box plane (i, k), its four waves the plane's rows; 2^lpr_log2 consecutive lanes share a row, so a wave
 * copies 64 >> lpr_log2 rows at a time.  Output words go out in 16-byte groups aligned in the output; only the group at either
 * end of a row's span is stored word by word.  The staging words are read at any alignment.
 */

namespace mrcz {

/* output words [oa, ob) of the box array: from src[o + sdelta] (or the fill word), by `lanes` lanes of which this is `lane` */
template <bool FILL>
__device__ __forceinline__ void box_span(uint32_t *__restrict__ out, uint64_t oa, uint64_t ob, const uint32_t *__restrict__ src,
                                         int64_t sdelta, uint32_t fill, uint32_t lane, uint32_t lanes)
{
    const uint64_t g1 = (ob + 3u) >> 2;
    for (uint64_t g = (oa >> 2) + lane; g < g1; g += lanes) {
        const uint64_t o0 = g << 2;
        uint32_t *o = out + o0;
        if (o0 >= oa && o0 + 4u <= ob) {
            uint4 v;
            if (FILL) v = make_uint4(fill, fill, fill, fill);
            else __builtin_memcpy(&v, src + (uint64_t)((int64_t)o0 + sdelta), 16);
            *reinterpret_cast<uint4 *>(o) = v;
        } else {
            for (uint32_t q = 0; q < 4u; q++)
                if (o0 + q >= oa && o0 + q < ob) o[q] = FILL ? fill : src[(uint64_t)((int64_t)(o0 + q) + sdelta)];
        }
    }
}

/* The box planes (list[e], k) of the boxes in `list`, blockIdx.x = e * bz + k: every row part that lies in the volume and in
 * the file words [B0, B1) (= stage[0, B1 - B0)) is copied to the output.  A plane whose section misses [B0, B1) leaves at once,
 * a row that misses it after one test. */
__global__ __launch_bounds__(256) void k_gather_boxes(const uint32_t *__restrict__ stage, uint64_t B0, uint64_t B1,
                                                      const int32_t *__restrict__ org, const uint32_t *__restrict__ list,
                                                      mrcz_box_geom_t g, uint32_t lpr_log2, uint32_t *__restrict__ out)
{
    const uint32_t e = blockIdx.x / g.bz, k = blockIdx.x - e * g.bz;
    const uint32_t i = list[e];
    const int64_t x0 = org[3u * i], y0 = org[3u * i + 1u], z = (int64_t)org[3u * i + 2u] + k;
    if (z < 0 || z >= (int64_t)g.nz) return;
    const uint64_t sec = (uint64_t)g.nx * g.ny, zw = g.data_word0 + (uint64_t)z * sec; /* file word of section z */
    if (zw + sec <= B0 || zw >= B1) return;
    const int64_t la = x0 < 0 ? -x0 : 0, lb = (int64_t)g.nx - x0 < (int64_t)g.bx ? (int64_t)g.nx - x0 : (int64_t)g.bx;
    if (lb <= la) return; /* the box lies beside the volume in x */
    const uint32_t lanes = 1u << lpr_log2, lane = threadIdx.x & (lanes - 1u);
    const uint64_t pbase = ((uint64_t)i * g.bz + k) * g.by * g.bx; /* output word of the plane's first voxel */
    for (uint32_t j = threadIdx.x >> lpr_log2; j < g.by; j += 256u >> lpr_log2) {
        const int64_t y = y0 + j;
        if (y < 0 || y >= (int64_t)g.ny) continue;
        const int64_t rw = (int64_t)(zw + (uint64_t)y * g.nx) + x0; /* file word of row element l is rw + l */
        if (rw + lb <= (int64_t)B0 || rw + la >= (int64_t)B1) continue;
        const int64_t a = rw + la < (int64_t)B0 ? (int64_t)B0 - rw : la, b = rw + lb > (int64_t)B1 ? (int64_t)B1 - rw : lb;
        const uint64_t rbase = pbase + (uint64_t)j * g.bx;
        box_span<false>(out, rbase + (uint64_t)a, rbase + (uint64_t)b, stage, rw - (int64_t)B0 - (int64_t)rbase, 0u, lane, lanes);
    }
}

/* The out-of-volume voxels of the box planes (list[e], k), blockIdx.x = e * bz + k, get the fill word. */
__global__ __launch_bounds__(256) void k_fill_boxes(const int32_t *__restrict__ org, const uint32_t *__restrict__ list,
                                                    mrcz_box_geom_t g, uint32_t lpr_log2, uint32_t *__restrict__ out)
{
    const uint32_t e = blockIdx.x / g.bz, k = blockIdx.x - e * g.bz;
    const uint32_t i = list[e];
    const int64_t x0 = org[3u * i], y0 = org[3u * i + 1u], z = (int64_t)org[3u * i + 2u] + k;
    const bool zout = z < 0 || z >= (int64_t)g.nz;
    /* row elements [la, lb) lie in the volume in x, 0 <= la <= lb <= bx */
    int64_t la = x0 < 0 ? -x0 : 0, lb = (int64_t)g.nx - x0 < (int64_t)g.bx ? (int64_t)g.nx - x0 : (int64_t)g.bx;
    if (la > (int64_t)g.bx) la = g.bx;
    if (lb < la) lb = la;
    const uint32_t lanes = 1u << lpr_log2, lane = threadIdx.x & (lanes - 1u);
    const uint64_t pbase = ((uint64_t)i * g.bz + k) * g.by * g.bx;
    for (uint32_t j = threadIdx.x >> lpr_log2; j < g.by; j += 256u >> lpr_log2) {
        const int64_t y = y0 + j;
        const uint64_t rbase = pbase + (uint64_t)j * g.bx;
        if (zout || y < 0 || y >= (int64_t)g.ny) {
            box_span<true>(out, rbase, rbase + g.bx, NULL, 0, g.fill_bits, lane, lanes);
        } else {
            if (la > 0) box_span<true>(out, rbase, rbase + (uint64_t)la, NULL, 0, g.fill_bits, lane, lanes);
            if (lb < (int64_t)g.bx) box_span<true>(out, rbase + (uint64_t)lb, rbase + g.bx, NULL, 0, g.fill_bits, lane, lanes);
        }
    }
}

} /* namespace mrcz */

/* ---- host side ---- */

/* the volume fits in the file and no size is zero */
static bool box_geom_ok(const mrcz_box_geom_t *g, uint64_t nfloats_file)
{
    if (!g || !g->nx || !g->ny || !g->nz || !g->bx || !g->by || !g->bz) return false;
    if (g->data_word0 > nfloats_file) return false;
    const uint64_t room = nfloats_file - g->data_word0, sec = (uint64_t)g->nx * g->ny;
    return sec <= room && g->nz <= room / sec;
}

/* the part of box i inside the volume, as half-open voxel ranges; false if it is empty */
struct BoxClip { int64_t xa, xb, ya, yb, za, zb; };
static bool box_clip(const mrcz_box_geom_t *g, const int32_t *o, BoxClip *c)
{
    const int64_t x0 = o[0], y0 = o[1], z0 = o[2];
    c->xa = x0 < 0 ? 0 : x0; c->xb = x0 + g->bx < (int64_t)g->nx ? x0 + g->bx : (int64_t)g->nx;
    c->ya = y0 < 0 ? 0 : y0; c->yb = y0 + g->by < (int64_t)g->ny ? y0 + g->by : (int64_t)g->ny;
    c->za = z0 < 0 ? 0 : z0; c->zb = z0 + g->bz < (int64_t)g->nz ? z0 + g->bz : (int64_t)g->nz;
    return c->xa < c->xb && c->ya < c->yb && c->za < c->zb;
}

/* lanes per row (log2): a power of two >= the 16-byte output groups a row can touch, at most a wave */
static uint32_t box_lpr_log2(uint32_t bx)
{
    const uint32_t groups = (bx & 3u) ? (bx + 6u) / 4u : bx / 4u;
    uint32_t l = 0;
    while (l < 6u && (1u << l) < groups) l++;
    return l;
}

extern "C" int mrcz_box_origins(const mrcz_box_geom_t *g, const double *h_centers, uint32_t nboxes, int32_t *h_origins)
{
    if (!g || !g->bx || !g->by || !g->bz) return MRCZ_EINVAL;
    if (nboxes && (!h_centers || !h_origins)) return MRCZ_EINVAL;
    const uint32_t size[3] = {g->bx, g->by, g->bz};
    for (uint64_t k = 0; k < 3ull * nboxes; k++) {
        const double c = h_centers[k];
        if (!(c == c) || c > 4.0e9 || c < -4.0e9) return MRCZ_EINVAL; /* NaN, infinities and centres no int32 origin can have */
        const double o = floor(c + 0.5) - (double)(size[k % 3] / 2u);
        if (o < -2147483648.0 || o > 2147483647.0) return MRCZ_EINVAL;
        h_origins[k] = (int32_t)o;
    }
    return MRCZ_OK;
}

extern "C" int mrcz_boxes_chunks(const mrcz_box_geom_t *g, const int32_t *h_origins, uint32_t nboxes, uint64_t nfloats_file,
                                 uint32_t chk, uint8_t *covered)
{
    if (!covered || chk == 0 || !box_geom_ok(g, nfloats_file) || (nboxes && !h_origins)) return MRCZ_EINVAL;
    memset(covered, 0, (size_t)((nfloats_file + chk - 1) / chk));
    const uint64_t nx = g->nx, sec = nx * g->ny;
    for (uint32_t i = 0; i < nboxes; i++) {
        BoxClip b;
        if (!box_clip(g, h_origins + 3ull * i, &b)) continue;
        for (int64_t z = b.za; z < b.zb; z++) {
            const uint64_t s0 = g->data_word0 + (uint64_t)z * sec;
            const uint64_t first = s0 + (uint64_t)b.ya * nx + (uint64_t)b.xa, last = s0 + (uint64_t)(b.yb - 1) * nx + (uint64_t)b.xb - 1u;
            if (first / chk == last / chk) { covered[first / chk] = 1; continue; } /* the box's rows of this section in one chunk */
            for (int64_t y = b.ya; y < b.yb; y++) {                                  /* rows may skip whole chunks (nx > chk) */
                const uint64_t r0 = s0 + (uint64_t)y * nx + (uint64_t)b.xa, r1 = r0 + (uint64_t)(b.xb - b.xa) - 1u;
                for (uint64_t c = r0 / chk; c <= r1 / chk; c++) covered[c] = 1;
            }
        }
    }
    return MRCZ_OK;
}

/* is the whole box inside the volume (no fill word to write)? */
static bool box_whole(const mrcz_box_geom_t *g, const int32_t *o, const BoxClip &c)
{
    return c.xa == o[0] && c.xb == (int64_t)o[0] + g->bx && c.ya == o[1] && c.yb == (int64_t)o[1] + g->by && c.za == o[2] &&
           c.zb == (int64_t)o[2] + g->bz;
}

/* device words for the origins and the box lists of one call; grows, freed by mrcz_destroy */
static int ensure_boxbuf(mrcz_ctx *ctx, uint64_t words)
{
    if (words <= ctx->boxbuf_words) return MRCZ_OK;
    (void)hipFree(ctx->boxbuf);
    ctx->boxbuf_words = 0;
    hipError_t e = hipMalloc((void **)&ctx->boxbuf, (size_t)words * 4u);
    if (e != hipSuccess) { ctx->boxbuf = NULL; return fail(ctx, MRCZ_ENOMEM, "box lists", e); }
    ctx->boxbuf_words = words;
    return MRCZ_OK;
}

/* a run of covered chunks [c0, c0 + nb), decoded as one batch; its boxes are words [list0, list0 + nlist) of ctx->boxbuf */
struct BoxRun { uint64_t c0, list0, nlist; uint32_t nb; };

/* walk the records of chunks [c, c_end) (headers only), in batches of the workspace */
static int walk_chunks(mrcz_ctx *ctx, const uint8_t *rec, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t c, uint64_t c_end)
{
    hipStream_t lstream = ctx->stream;
    while (c < c_end) {
        const uint64_t nb = (c_end - c) < ctx->max_chunks ? (c_end - c) : ctx->max_chunks;
        const uint64_t bfl = (nfloats_file - c * chk) < nb * chk ? (nfloats_file - c * chk) : nb * chk;
        LAUNCH("k_parse_records", k_parse_records, dim3(1), dim3(64), rec, len, bfl, chk, ctx->dstreams, ctx->result, ctx->lz4_planes);
        c += nb;
    }
    return MRCZ_OK;
}

/* ctx->boxbuf holds the origins (3 nboxes words), the fill list (nfill) and the lists of the runs */
static int uncompress_boxes_enqueue(mrcz_ctx *ctx, const uint8_t *rec, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                    uint64_t nchunks, const mrcz_box_geom_t *g, uint32_t nboxes, uint64_t nfill, const BoxRun *runs,
                                    uint64_t nruns, uint32_t *out, int int_mode)
{
    hipStream_t lstream = ctx->stream;
    const int32_t *org = (const int32_t *)ctx->boxbuf;
    const uint32_t lpr = box_lpr_log2(g->bx);
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    if (nfill) LAUNCH("k_fill_boxes", k_fill_boxes, dim3((uint32_t)(nfill * g->bz)), dim3(256), org, ctx->boxbuf + 3ull * nboxes, *g, lpr, out);
    uint64_t c = first_chunk;
    for (uint64_t r = 0; r < nruns; r++) {
        if (int rc = walk_chunks(ctx, rec, len, nfloats_file, chk, c, runs[r].c0)) return rc;
        const uint32_t nb = runs[r].nb;
        const uint64_t bbase = runs[r].c0 * chk, bfl = (nfloats_file - bbase) < (uint64_t)nb * chk ? (nfloats_file - bbase) : (uint64_t)nb * chk;
        if (int rc = decode_batch(ctx, rec, len, bfl, nb, chk)) return rc;
        LAUNCH("k_merge_segments", k_merge_segments<false>, dim3(512, nb), dim3(256), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx, bfl,
               chk, ctx->stage, len, (uint64_t)4 * ctx->row_chunks * CHK, int_mode ? 1u : 0u, bbase, (int64_t)0, (uint64_t)0);
        if (runs[r].nlist)
            LAUNCH("k_gather_boxes", k_gather_boxes, dim3((uint32_t)(runs[r].nlist * g->bz)), dim3(256), ctx->stage, bbase, bbase + bfl, org,
                   ctx->boxbuf + runs[r].list0, *g, lpr, out);
        c = runs[r].c0 + nb;
    }
    /* the chunks behind the last run are walked too: records that end before the span does are refused */
    if (int rc = walk_chunks(ctx, rec, len, nfloats_file, chk, c, first_chunk + nchunks)) return rc;
    HIPCHK(hipMemcpyAsync(ctx->h_result, ctx->result, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_boxes(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                                     uint64_t first_chunk, uint64_t nchunks, const mrcz_box_geom_t *g, const int32_t *h_origins,
                                     uint32_t nboxes, void *d_out, int int_mode, uint64_t *chunks_decoded)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chunks_decoded) *chunks_decoded = 0;
    if (!box_geom_ok(g, nfloats_file)) return fail(ctx, MRCZ_EINVAL, "box size zero or volume outside the file", hipSuccess);
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EFORMAT, "chunk size in header exceeds CHUNK_SIZE (constant.h:25)", hipSuccess);
    const uint64_t nchunks_file = (nfloats_file + chk - 1) / chk;
    if (first_chunk > nchunks_file || nchunks > nchunks_file - first_chunk) return fail(ctx, MRCZ_EINVAL, "chunks past the end of the file", hipSuccess);
    if ((uint64_t)nboxes * g->bz > 0x7fffffffull) return fail(ctx, MRCZ_EINVAL, "more box planes than one launch takes (nboxes x bz >= 2^31)", hipSuccess);
    if (nboxes == 0) return MRCZ_OK;
    if (!h_origins || !d_out || (nchunks && !d_records)) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (nchunks) {
        if (int rc = uncompress_prepare(ctx, d_records, chk, d_out)) return rc;
    } else {
        if ((uintptr_t)d_out & 15u) return fail(ctx, MRCZ_EINVAL, "d_out must be 16-byte aligned", hipSuccess);
        HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    }
    if (!ctx->stage) { /* k_merge_segments<false> writes a batch's words here for k_gather_boxes */
        hipError_t e = hipMalloc((void **)&ctx->stage, (size_t)ctx->max_chunks * CHK * 4u);
        if (e != hipSuccess) { ctx->stage = NULL; return fail(ctx, MRCZ_ENOMEM, "box staging buffer", e); }
    }
    /* host: the covered chunks, cut into runs of at most max_chunks; the boxes with out-of-volume voxels (fill list); per run the
     * boxes whose z-extent in the volume meets the run's file words */
    uint8_t *covered = (uint8_t *)malloc((size_t)nchunks_file + (size_t)nboxes);
    BoxRun *runs = (BoxRun *)malloc(sizeof(BoxRun) * (size_t)(nchunks + 1u));
    BoxClip *clip = (BoxClip *)malloc(sizeof(BoxClip) * nboxes);
    if (!covered || !runs || !clip) { free(covered); free(runs); free(clip); return fail(ctx, MRCZ_ENOMEM, "host memory", hipSuccess); }
    uint8_t *inside = covered + nchunks_file;
    (void)mrcz_boxes_chunks(g, h_origins, nboxes, nfloats_file, chk, covered);
    uint64_t nruns = 0, nfill = 0, decoded = 0;
    for (uint32_t i = 0; i < nboxes; i++) {
        inside[i] = box_clip(g, h_origins + 3ull * i, &clip[i]) ? 1u : 0u;
        if (!inside[i] || !box_whole(g, h_origins + 3ull * i, clip[i])) nfill++;
    }
    const uint64_t sec = (uint64_t)g->nx * g->ny;
    uint64_t nwords = 3ull * nboxes + nfill;
    for (uint64_t c = first_chunk; c < first_chunk + nchunks;) {
        if (!covered[c]) { c++; continue; }
        uint64_t e = c;
        while (e < first_chunk + nchunks && covered[e] && e - c < ctx->max_chunks) e++;
        BoxRun &R = runs[nruns++];
        R.c0 = c; R.nb = (uint32_t)(e - c); R.list0 = nwords; R.nlist = 0;
        for (uint32_t i = 0; i < nboxes; i++)
            if (inside[i] && g->data_word0 + (uint64_t)clip[i].za * sec < e * chk && g->data_word0 + (uint64_t)clip[i].zb * sec > c * chk) R.nlist++;
        nwords += R.nlist;
        decoded += e - c;
        c = e;
    }
    uint32_t *h = (uint32_t *)malloc((size_t)nwords * 4u);
    if (!h) { free(covered); free(runs); free(clip); return fail(ctx, MRCZ_ENOMEM, "host memory", hipSuccess); }
    memcpy(h, h_origins, 12ull * nboxes);
    uint64_t w = 3ull * nboxes;
    for (uint32_t i = 0; i < nboxes; i++)
        if (!inside[i] || !box_whole(g, h_origins + 3ull * i, clip[i])) h[w++] = i;
    for (uint64_t r = 0; r < nruns; r++) {
        const uint64_t B0 = runs[r].c0 * chk, B1 = (runs[r].c0 + runs[r].nb) * chk;
        for (uint32_t i = 0; i < nboxes; i++)
            if (inside[i] && g->data_word0 + (uint64_t)clip[i].za * sec < B1 && g->data_word0 + (uint64_t)clip[i].zb * sec > B0) h[w++] = i;
    }
    free(covered);
    free(clip);
    int rc = ensure_boxbuf(ctx, nwords);
    if (rc == MRCZ_OK && hipMemcpyAsync(ctx->boxbuf, h, (size_t)nwords * 4u, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(ctx, MRCZ_EHIP, "copy box lists", hipSuccess);
    if (rc == MRCZ_OK)
        rc = uncompress_boxes_enqueue(ctx, (const uint8_t *)d_records, len, nfloats_file, chk, first_chunk, nchunks, g, nboxes, nfill, runs, nruns,
                                      (uint32_t *)d_out, int_mode);
    if (rc == MRCZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MRCZ_EHIP, "stream sync (uncompress boxes)", hipSuccess);
    if (rc != MRCZ_OK) (void)hipStreamSynchronize(ctx->stream); /* the list copy may still read h */
    free(h);
    free(runs);
    if (rc) return rc;
    latch_fallbacks(ctx);
    if (ctx->h_result[1]) return fail(ctx, MRCZ_EFORMAT, "malformed chunk records or deflate stream", hipSuccess);
    if (chunks_decoded) *chunks_decoded = decoded;
    return MRCZ_OK;
}
