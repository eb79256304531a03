/*
 * mrcz_compare.hip -- compare decode (include/mrcz_hip.h, mrcz_uncompress_compare): an error summary of every chunk of a container
 * against the original's words, streaming the chunks through a context of fixed size.
 *
 * Included from mrcz_api.hip after the binned decode (it uses the context, decode_batch and the staging buffer as that does).
 * Per run of up to max_chunks consecutive chunks: decode_batch, k_merge_segments<false> into the staging buffer, k_compare_fold
 * (CMP_WGS workgroups per chunk, each writes one CmpPart to its own slot of ctx->cmp_part with plain stores), k_compare_chunk
 * (one wave per chunk folds the chunk's CMP_WGS partials and assigns the chunk's mrcz_compare_t to d_acc[chunk]).
 *
 * The order in which a chunk's points are added is a function of their place in the chunk alone:
 *   group g = words 4g .. 4g + 3 of the chunk goes to thread (g mod 256) of workgroup ((g / 256) mod CMP_WGS); a thread takes its
 *   groups in increasing order, the words of a group in increasing order, every sum starting from +0.0 (a word that does not count
 *   adds +0.0, which changes no sum that started from +0.0);
 *   the 64 lanes of a wave are folded by the xor butterfly 32, 16, 8, 4, 2, 1 (cmp_merge is commutative, so every lane holds the
 *   same bits), the four waves of a workgroup in wave order by thread 0;
 *   k_compare_chunk: lane l folds partials l, l + 64, l + 128, ... in that order, then the same butterfly.
 * Nothing depends on the batch, the call or first_chunk, and there is no atomic: the bits of d_acc[c] are a function of chunk c's
 * words (and of the bounds).
 */

namespace mrcz {

constexpr uint32_t CMP_WGS = 256;          /* workgroups per chunk: a constant of the source (the summation order depends on it) */
constexpr uint32_t CMP_NONE = 0xffffffffu; /* no index (chunk-local word indices are < CHK) */

/* a partial summary of some words of one chunk; indices are word indices inside the chunk */
struct CmpPart {
    uint32_t n_header_diff, n_diff, n_finite, n_special_diff, n_over_abs, n_over_rel;
    uint32_t first_over, max_err_index, max_rel_index; /* CMP_NONE: none */
    float orig_min, orig_max;                          /* +Inf / -Inf: none */
    uint32_t pad_;
    double max_err, max_rel;                           /* -1: none */
    double sum_err, sum_abs_err, sum_err2, orig_sum, orig_sum2;
};

__device__ __forceinline__ float cmp_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

__device__ __forceinline__ void cmp_init(CmpPart &p)
{
    p.n_header_diff = p.n_diff = p.n_finite = p.n_special_diff = p.n_over_abs = p.n_over_rel = 0u;
    p.first_over = p.max_err_index = p.max_rel_index = CMP_NONE;
    p.orig_min = cmp_float(0x7f800000u);
    p.orig_max = cmp_float(0xff800000u);
    p.pad_ = 0u;
    p.max_err = p.max_rel = -1.0;
    p.sum_err = p.sum_abs_err = p.sum_err2 = p.orig_sum = p.orig_sum2 = 0.0;
}

/* a <- a and b folded: counts and sums added, extremes with the lower index on ties.  Commutative bit for bit. */
__device__ __forceinline__ void cmp_merge(CmpPart &a, const CmpPart &b)
{
    a.n_header_diff += b.n_header_diff; a.n_diff += b.n_diff; a.n_finite += b.n_finite;
    a.n_special_diff += b.n_special_diff; a.n_over_abs += b.n_over_abs; a.n_over_rel += b.n_over_rel;
    a.first_over = a.first_over < b.first_over ? a.first_over : b.first_over;
    if (b.max_err > a.max_err || (b.max_err == a.max_err && b.max_err_index < a.max_err_index)) { a.max_err = b.max_err; a.max_err_index = b.max_err_index; }
    if (b.max_rel > a.max_rel || (b.max_rel == a.max_rel && b.max_rel_index < a.max_rel_index)) { a.max_rel = b.max_rel; a.max_rel_index = b.max_rel_index; }
    a.orig_min = b.orig_min < a.orig_min ? b.orig_min : a.orig_min;
    a.orig_max = b.orig_max > a.orig_max ? b.orig_max : a.orig_max;
    a.sum_err += b.sum_err; a.sum_abs_err += b.sum_abs_err; a.sum_err2 += b.sum_err2;
    a.orig_sum += b.orig_sum; a.orig_sum2 += b.orig_sum2;
}

/* every lane's p <- the fold of the wave's 64 p */
__device__ __forceinline__ void cmp_wave_fold(CmpPart &p)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        CmpPart o;
        o.n_header_diff = __shfl_xor(p.n_header_diff, m); o.n_diff = __shfl_xor(p.n_diff, m); o.n_finite = __shfl_xor(p.n_finite, m);
        o.n_special_diff = __shfl_xor(p.n_special_diff, m); o.n_over_abs = __shfl_xor(p.n_over_abs, m); o.n_over_rel = __shfl_xor(p.n_over_rel, m);
        o.first_over = __shfl_xor(p.first_over, m); o.max_err_index = __shfl_xor(p.max_err_index, m); o.max_rel_index = __shfl_xor(p.max_rel_index, m);
        o.orig_min = __shfl_xor(p.orig_min, m); o.orig_max = __shfl_xor(p.orig_max, m);
        o.max_err = __shfl_xor(p.max_err, m); o.max_rel = __shfl_xor(p.max_rel, m);
        o.sum_err = __shfl_xor(p.sum_err, m); o.sum_abs_err = __shfl_xor(p.sum_abs_err, m); o.sum_err2 = __shfl_xor(p.sum_err2, m);
        o.orig_sum = __shfl_xor(p.orig_sum, m); o.orig_sum2 = __shfl_xor(p.orig_sum2, m);
        cmp_merge(p, o);
    }
}

/* one point: original word a and decoded word b at word i of the chunk; hdr = a file word < 256; live = inside the chunk.
 * No branch: a word that does not count adds zeros. */
__device__ __forceinline__ void cmp_point(CmpPart &p, uint32_t a, uint32_t b, uint32_t i, bool live, bool hdr, double eps_abs, double eps_rel)
{
    const bool diff = a != b;
    const bool data = live && !hdr;
    const bool fin = ((a & 0x7f800000u) != 0x7f800000u) && ((b & 0x7f800000u) != 0x7f800000u);
    const bool pt = data && fin;
    const bool spec = data && !fin && diff;
    p.n_header_diff += (live && hdr && diff) ? 1u : 0u;
    p.n_diff += (data && diff) ? 1u : 0u;
    p.n_finite += pt ? 1u : 0u;
    p.n_special_diff += spec ? 1u : 0u;
    const float fa = cmp_float(pt ? a : 0u), fb = cmp_float(pt ? b : 0u);
    const double da = (double)fa, d = (double)fb - da;
    const double err = fabs(d), mag = fabs(da);
    const double rel = mag > 1e-3 ? err / mag : 0.0;
    const bool oa = pt && err > eps_abs, orl = pt && rel > eps_rel; /* (a bound that is switched off arrives as +Inf) */
    p.n_over_abs += oa ? 1u : 0u;
    p.n_over_rel += orl ? 1u : 0u;
    if ((oa || orl || spec) && i < p.first_over) p.first_over = i;
    const double e = pt ? err : -2.0, r = pt ? rel : -2.0;
    if (e > p.max_err) { p.max_err = e; p.max_err_index = i; }
    if (r > p.max_rel) { p.max_rel = r; p.max_rel_index = i; }
    p.orig_min = pt && fa < p.orig_min ? fa : p.orig_min;
    p.orig_max = pt && fa > p.orig_max ? fa : p.orig_max;
    p.sum_err += d; p.sum_abs_err += err; p.sum_err2 += d * d;
    p.orig_sum += da; p.orig_sum2 += da * da;
}

/* grid (CMP_WGS, nb): workgroup (w, k) folds its groups of chunk k of the run (stage and orig hold the run's words from file word
 * bbase on, bfl of them) into part[k * CMP_WGS + w] */
__global__ __launch_bounds__(256) void k_compare_fold(const uint32_t *__restrict__ stage, const uint32_t *__restrict__ orig, uint64_t bbase, uint64_t bfl,
                                                      uint32_t chk, double eps_abs, double eps_rel, CmpPart *__restrict__ part)
{
    __shared__ CmpPart sh[4];
    const uint32_t k = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
    const uint64_t cb = (uint64_t)k * chk;                                    /* the chunk's first word in the run */
    const uint32_t cl = (uint32_t)(bfl - cb < chk ? bfl - cb : chk);          /* its words */
    const uint64_t fw = bbase + cb;                                           /* its first file word */
    const uint32_t nhdr = fw >= 256u ? 0u : (uint32_t)(256u - fw);            /* chunk words < nhdr are header words */
    const bool vec = (chk & 3u) == 0u;                                        /* then every chunk base is 16-byte aligned */
    const uint32_t *__restrict__ sp = stage + cb, *__restrict__ op = orig + cb;
    const uint32_t ngroups = (cl + 3u) >> 2;
    CmpPart p;
    cmp_init(p);
    for (uint32_t g = w * 256u + t; g < ngroups; g += CMP_WGS * 256u) {
        const uint32_t i = g << 2;
        uint4 a, b;
        if (vec && i + 4u <= cl) {
            a = *reinterpret_cast<const uint4 *>(op + i);
            b = *reinterpret_cast<const uint4 *>(sp + i);
        } else { /* the chunk's tail, or a chunk size that is no multiple of four */
            a.x = op[i]; b.x = sp[i];
            a.y = i + 1u < cl ? op[i + 1u] : 0u; b.y = i + 1u < cl ? sp[i + 1u] : 0u;
            a.z = i + 2u < cl ? op[i + 2u] : 0u; b.z = i + 2u < cl ? sp[i + 2u] : 0u;
            a.w = i + 3u < cl ? op[i + 3u] : 0u; b.w = i + 3u < cl ? sp[i + 3u] : 0u;
        }
        cmp_point(p, a.x, b.x, i, true, i < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.y, b.y, i + 1u, i + 1u < cl, i + 1u < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.z, b.z, i + 2u, i + 2u < cl, i + 2u < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.w, b.w, i + 3u, i + 3u < cl, i + 3u < nhdr, eps_abs, eps_rel);
    }
    cmp_wave_fold(p);
    if ((t & 63u) == 0u) sh[t >> 6] = p;
    __syncthreads();
    if (t == 0u) {
        cmp_merge(p, sh[1]);
        cmp_merge(p, sh[2]);
        cmp_merge(p, sh[3]);
        part[(uint64_t)k * CMP_WGS + w] = p;
    }
}

/* grid (nb), one wave: chunk k's CMP_WGS partials -> acc[c_first + k] */
__global__ __launch_bounds__(64) void k_compare_chunk(const CmpPart *__restrict__ part, uint64_t bbase, uint64_t bfl, uint32_t chk, uint64_t c_first,
                                                      mrcz_compare_t *__restrict__ acc)
{
    const uint32_t k = blockIdx.x, l = threadIdx.x;
    CmpPart p = part[(uint64_t)k * CMP_WGS + l];
    for (uint32_t j = l + 64u; j < CMP_WGS; j += 64u) cmp_merge(p, part[(uint64_t)k * CMP_WGS + j]);
    cmp_wave_fold(p);
    if (l != 0u) return;
    const uint64_t cb = (uint64_t)k * chk, cl = bfl - cb < chk ? bfl - cb : chk, fw = bbase + cb;
    const uint64_t nhdr = fw >= 256u ? 0u : (256u - fw < cl ? 256u - fw : cl);
    const uint64_t none = ~(uint64_t)0;
    mrcz_compare_t r;
    r.n = cl - nhdr;
    r.n_header_diff = p.n_header_diff; r.n_diff = p.n_diff; r.n_finite = p.n_finite; r.n_special_diff = p.n_special_diff;
    r.n_over_abs = p.n_over_abs; r.n_over_rel = p.n_over_rel;
    r.first_over = p.first_over == CMP_NONE ? none : fw + p.first_over;
    r.max_err_index = p.max_err_index == CMP_NONE ? none : fw + p.max_err_index;
    r.max_rel_index = p.max_rel_index == CMP_NONE ? none : fw + p.max_rel_index;
    r.max_err = p.max_err_index == CMP_NONE ? 0.0 : p.max_err;
    r.max_rel = p.max_rel_index == CMP_NONE ? 0.0 : p.max_rel;
    r.sum_err = p.sum_err; r.sum_abs_err = p.sum_abs_err; r.sum_err2 = p.sum_err2;
    r.orig_min = (double)p.orig_min; r.orig_max = (double)p.orig_max; r.orig_sum = p.orig_sum; r.orig_sum2 = p.orig_sum2;
    acc[c_first + k] = r;
}

} /* namespace mrcz */

/* ---- host side ---- */

static int uncompress_compare_enqueue(mrcz_ctx *ctx, const uint8_t *rec, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                      uint64_t nchunks, const uint32_t *orig, double eps_abs, double eps_rel, int int_mode, mrcz_compare_t *acc)
{
    hipStream_t lstream = ctx->stream;
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    const uint64_t end = first_chunk + nchunks;
    for (uint64_t c = first_chunk; c < end;) {
        const uint32_t nb = (uint32_t)((end - c) < ctx->max_chunks ? (end - c) : ctx->max_chunks);
        const uint64_t bbase = c * chk, bfl = (nfloats_file - bbase) < (uint64_t)nb * chk ? (nfloats_file - bbase) : (uint64_t)nb * chk;
        if (int rc = decode_batch(ctx, rec, len, bfl, nb, chk)) return rc;
        LAUNCH("k_merge_segments", k_merge_segments<false>, dim3(512, nb), dim3(256), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx,
               bfl, chk, ctx->stage, len, (uint64_t)4 * ctx->row_chunks * CHK, int_mode ? 1u : 0u, bbase, (int64_t)0, (uint64_t)0);
        LAUNCH("k_compare_fold", k_compare_fold, dim3(CMP_WGS, nb), dim3(256), ctx->stage, orig + (c - first_chunk) * chk, bbase, bfl, chk, eps_abs, eps_rel,
               ctx->cmp_part);
        LAUNCH("k_compare_chunk", k_compare_chunk, dim3(nb), dim3(64), ctx->cmp_part, bbase, bfl, chk, c, acc);
        c += nb;
    }
    HIPCHK(hipMemcpyAsync(ctx->h_result, ctx->result, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_compare(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                                       uint64_t first_chunk, uint64_t nchunks, const void *d_orig, double eps_abs, double eps_rel,
                                       int int_mode, mrcz_compare_t *d_acc)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EFORMAT, "chunk size in header exceeds CHUNK_SIZE (constant.h:25)", hipSuccess);
    const uint64_t nchunks_file = (nfloats_file + chk - 1) / chk;
    if (first_chunk > nchunks_file || nchunks > nchunks_file - first_chunk) return fail(ctx, MRCZ_EINVAL, "chunks past the end of the file", hipSuccess);
    if (!d_acc || (nchunks && (!d_records || !d_orig))) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (nchunks == 0) return MRCZ_OK;
    if (((uintptr_t)d_orig & 15u) || ((uintptr_t)d_acc & 7u)) return fail(ctx, MRCZ_EINVAL, "d_orig must be 16-byte and d_acc 8-byte aligned", hipSuccess);
    if (int rc = uncompress_prepare(ctx, d_records, chk, NULL)) return rc;
    if (!ctx->stage) { /* k_merge_segments<false> writes a batch's words here for k_compare_fold */
        hipError_t e = hipMalloc((void **)&ctx->stage, (size_t)ctx->max_chunks * CHK * 4u);
        if (e != hipSuccess) { ctx->stage = NULL; return fail(ctx, MRCZ_ENOMEM, "staging buffer", e); }
    }
    if (!ctx->cmp_part) {
        hipError_t e = hipMalloc((void **)&ctx->cmp_part, (size_t)ctx->max_chunks * CMP_WGS * sizeof(CmpPart));
        if (e != hipSuccess) { ctx->cmp_part = NULL; return fail(ctx, MRCZ_ENOMEM, "compare partials", e); }
    }
    /* a bound that is negative or NaN switches its check off: no error exceeds +Inf */
    if (!(eps_abs >= 0.0)) eps_abs = INFINITY;
    if (!(eps_rel >= 0.0)) eps_rel = INFINITY;
    int rc = uncompress_compare_enqueue(ctx, (const uint8_t *)d_records, len, nfloats_file, chk, first_chunk, nchunks, (const uint32_t *)d_orig, eps_abs,
                                        eps_rel, int_mode, d_acc);
    if (rc == MRCZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MRCZ_EHIP, "stream sync (uncompress compare)", hipSuccess);
    if (rc != MRCZ_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    latch_fallbacks(ctx);
    if (ctx->h_result[1]) return fail(ctx, MRCZ_EFORMAT, "malformed chunk records or deflate stream", hipSuccess);
    return MRCZ_OK;
}

/* t <- t and c folded, c being a later chunk */
static void compare_add(mrcz_compare_t *t, const mrcz_compare_t *c)
{
    t->n += c->n; t->n_header_diff += c->n_header_diff; t->n_diff += c->n_diff; t->n_finite += c->n_finite;
    t->n_special_diff += c->n_special_diff; t->n_over_abs += c->n_over_abs; t->n_over_rel += c->n_over_rel;
    if (c->first_over < t->first_over) t->first_over = c->first_over;
    if (c->max_err_index != UINT64_MAX && (t->max_err_index == UINT64_MAX || c->max_err > t->max_err ||
                                           (c->max_err == t->max_err && c->max_err_index < t->max_err_index))) {
        t->max_err = c->max_err; t->max_err_index = c->max_err_index;
    }
    if (c->max_rel_index != UINT64_MAX && (t->max_rel_index == UINT64_MAX || c->max_rel > t->max_rel ||
                                           (c->max_rel == t->max_rel && c->max_rel_index < t->max_rel_index))) {
        t->max_rel = c->max_rel; t->max_rel_index = c->max_rel_index;
    }
    t->sum_err += c->sum_err; t->sum_abs_err += c->sum_abs_err; t->sum_err2 += c->sum_err2;
    if (c->orig_min < t->orig_min) t->orig_min = c->orig_min;
    if (c->orig_max > t->orig_max) t->orig_max = c->orig_max;
    t->orig_sum += c->orig_sum; t->orig_sum2 += c->orig_sum2;
}

extern "C" int mrcz_compare_finish(mrcz_ctx_t *ctx, const mrcz_compare_t *d_acc, uint64_t first_chunk, uint64_t nchunks, mrcz_compare_t *h_total)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (!d_acc || !h_total) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    memset(h_total, 0, sizeof(*h_total));
    h_total->first_over = h_total->max_err_index = h_total->max_rel_index = UINT64_MAX;
    h_total->orig_min = INFINITY;
    h_total->orig_max = -INFINITY;
    if (nchunks == 0) return MRCZ_OK;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    mrcz_compare_t *h = (mrcz_compare_t *)malloc((size_t)nchunks * sizeof(*h));
    if (!h) return fail(ctx, MRCZ_ENOMEM, "chunk summaries", hipSuccess);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d_acc + first_chunk, (size_t)nchunks * sizeof(*h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(h); return fail(ctx, MRCZ_EHIP, "copy chunk summaries", e); }
    *h_total = h[0]; /* the sums start from the first chunk's values */
    for (uint64_t c = 1; c < nchunks; c++) compare_add(h_total, &h[c]);
    free(h);
    return MRCZ_OK;
}
