/*
 * mrcz_probe.hip -- probe (include/mrcz_hip.h, mrcz_probe_chunks): what a compress setting costs and what it buys, before a byte of
 * a container exists.  For the words of a run of chunks and one setting (-b bits, -e eps or -s int) it gives the exact record bytes
 * mrcz_compress_chunks / _abs / _int8 would write, and per chunk the mrcz_compare_t that mrcz_uncompress_compare would assign for
 * that container against the same words.
 *
 * Included from mrcz_api.hip after the compare decode (it uses compress_lane, and CmpPart, cmp_point, the folds and k_compare_chunk
 * of mrcz_compare.hip as they are).  Per batch of up to max_chunks chunks, all on the context's compute stream:
 *   size   compress_lane(phase 0) over the whole batch as one lane: summary ... pair offsets, after which StreamInfo::paylen holds
 *          every stream's payload length; k_probe_sizes adds them into the result words as k_container would.  Phases 1 and 2
 *          (k_container, k_clear_boundaries, k_emit, k_emit_headers) are never launched and there is no records buffer.
 *   error  k_probe_fold<Xform> reads the original's words once more, computes the word each decodes to (probe_word: the inline
 *          functions of the summary pass, stage_tile in mrcz_tile.h) and folds the pair by cmp_point; k_compare_chunk finishes the
 *          chunk.  Nothing is decoded and no second copy of the words exists.
 * k_probe_fold's work distribution and fold order are k_compare_fold's (see mrcz_compare.hip: group g to thread g mod 256 of
 * workgroup (g / 256) mod CMP_WGS, xor butterfly, waves in order, one partial per workgroup with plain stores), so the bits of
 * d_acc[c] depend on chunk c's words and the setting only.
 *
 * Streams.  compress_enqueue's rule is that a workspace row is only ever touched by one stream within a call.  The probe runs on
 * the compute stream alone (it is not the throughput path), so the rule holds trivially inside it; between calls everything is
 * ordered through the compute stream, which every compress call's lanes wait for at their start (ev_start) and which waits for
 * them at its end (ev_done).
 */

namespace mrcz {

/* the word a container written with transform X decodes to, for a word past the file header */
template <Xform X> __device__ __forceinline__ uint32_t probe_word(uint32_t w, typename XformArg<X>::type arg)
{
    if constexpr (X == Xform::Quant) return dequant_int8(quant_int8(w));
    else if constexpr (X == Xform::AbsErr) return abs_round(w, arg.q, arg.E);
    else return w & arg;
}

/* grid (CMP_WGS, nb): workgroup (w, k) folds its groups of chunk k of the batch (orig holds the batch's words from file word bbase
 * on, bfl of them, in chunks of CHK) against what they decode to into part[k * CMP_WGS + w] */
template <Xform X>
__global__ __launch_bounds__(256) void k_probe_fold(const uint32_t *__restrict__ orig, uint64_t bbase, uint64_t bfl, typename XformArg<X>::type arg,
                                                    double eps_abs, double eps_rel, CmpPart *__restrict__ part)
{
    __shared__ CmpPart sh[4];
    const uint32_t k = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
    const uint64_t cb = (uint64_t)k * CHK;                                    /* the chunk's first word in the batch (16-byte aligned) */
    const uint32_t cl = (uint32_t)(bfl - cb < CHK ? bfl - cb : CHK);          /* its words */
    const uint64_t fw = bbase + cb;                                           /* its first file word */
    const uint32_t nhdr = fw >= 256u ? 0u : (uint32_t)(256u - fw);            /* chunk words < nhdr are header words: they keep their bits */
    const uint32_t *__restrict__ op = orig + cb;
    const uint32_t ngroups = (cl + 3u) >> 2;
    CmpPart p;
    cmp_init(p);
    for (uint32_t g = w * 256u + t; g < ngroups; g += CMP_WGS * 256u) {
        const uint32_t i = g << 2;
        uint4 a;
        if (i + 4u <= cl) {
            a = *reinterpret_cast<const uint4 *>(op + i);
        } else { /* the tail group of a ragged last chunk */
            a.x = op[i];
            a.y = i + 1u < cl ? op[i + 1u] : 0u;
            a.z = i + 2u < cl ? op[i + 2u] : 0u;
            a.w = i + 3u < cl ? op[i + 3u] : 0u;
        }
        cmp_point(p, a.x, i < nhdr ? a.x : probe_word<X>(a.x, arg), i, true, i < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.y, i + 1u < nhdr ? a.y : probe_word<X>(a.y, arg), i + 1u, i + 1u < cl, i + 1u < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.z, i + 2u < nhdr ? a.z : probe_word<X>(a.z, arg), i + 2u, i + 2u < cl, i + 2u < nhdr, eps_abs, eps_rel);
        cmp_point(p, a.w, i + 3u < nhdr ? a.w : probe_word<X>(a.w, arg), i + 3u, i + 3u < cl, i + 3u < nhdr, eps_abs, eps_rel);
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

/* one workgroup, after phase 0 of a batch of nchunks <= 128 chunks: what k_container adds to the result words, and nothing else:
 * result[0] += 16 + the four payload lengths per chunk, result[1 + j] += payload length + 4 per chunk of plane j */
__global__ __launch_bounds__(256) void k_probe_sizes(const StreamInfo *__restrict__ sinfo, uint32_t nchunks, uint64_t *__restrict__ result)
{
    __shared__ unsigned long long sh[4][5];
    const uint32_t c = threadIdx.x;
    unsigned long long v[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    if (c < nchunks) {
        v[0] = 16ull;
        for (int j = 0; j < 4; j++) {
            const unsigned long long len = sinfo[4u * c + (uint32_t)j].paylen;
            v[0] += len;
            v[1 + j] = len + 4ull;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        for (int j = 0; j < 5; j++) v[j] += __shfl_xor(v[j], m);
    if ((c & 63u) == 0u)
        for (int j = 0; j < 5; j++) sh[c >> 6][j] = v[j];
    __syncthreads();
    if (c < 5u) result[c] += sh[0][c] + sh[1][c] + sh[2][c] + sh[3][c];
}

} /* namespace mrcz */

/* ---- host side ---- */

/* enqueue a probe on the compute stream; its five result words (record bytes, per-plane sums) are copied to the pinned host words
 * h_res[0..4] in stream order.  No host synchronisation.  nfloats == 0 enqueues nothing. */
static int probe_enqueue(mrcz_ctx *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int xform, int bits, float eps, double eps_abs,
                         double eps_rel, mrcz_compare_t *d_acc, uint64_t *h_res)
{
    if (!ctx || !h_res) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (xform != MRCZ_PROBE_MASK && xform != MRCZ_PROBE_ABS && xform != MRCZ_PROBE_INT8) return fail(ctx, MRCZ_EINVAL, "unknown probe transform", hipSuccess);
    uint32_t mask = 0xFFFFFFFFu;
    AbsErr ae = {};
    if (xform == MRCZ_PROBE_MASK) {
        if (bits < 0 || bits > 32) return fail(ctx, MRCZ_EINVAL, "bits outside 0..32 (reference table has 33 entries, workers.c:29-37)", hipSuccess);
        mask = mask_of(bits);
    }
    if (xform == MRCZ_PROBE_ABS)
        if (int rc = abs_err_param(ctx, eps, &ae)) return rc;
    if (nfloats == 0) return MRCZ_OK;
    if (!d_in) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_acc & 7u)) return fail(ctx, MRCZ_EINVAL, "d_in must be 16-byte and d_acc 8-byte aligned", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (int rc = ensure_planes(ctx)) return rc;
    if (d_acc && !ctx->cmp_part) {
        hipError_t e = hipMalloc((void **)&ctx->cmp_part, (size_t)ctx->max_chunks * CMP_WGS * sizeof(CmpPart));
        if (e != hipSuccess) { ctx->cmp_part = NULL; return fail(ctx, MRCZ_ENOMEM, "compare partials", e); }
    }
    /* a bound that is negative or NaN switches its check off: no error exceeds +Inf */
    if (!(eps_abs >= 0.0)) eps_abs = INFINITY;
    if (!(eps_rel >= 0.0)) eps_rel = INFINITY;
    const Xform xf = xform == MRCZ_PROBE_INT8 ? Xform::Quant : xform == MRCZ_PROBE_ABS ? Xform::AbsErr : Xform::Mask;
    const uint32_t cleared = cleared_planes(xf, mask);
    const uint32_t *in = (const uint32_t *)d_in;
    const uint64_t nchunks = (nfloats + CHK - 1) / CHK;
    hipStream_t lstream = ctx->stream;
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    for (uint64_t c0 = 0; c0 < nchunks; c0 += ctx->max_chunks) {
        const uint32_t nb = (uint32_t)((nchunks - c0) < ctx->max_chunks ? (nchunks - c0) : ctx->max_chunks);
        const uint64_t bfl = (nfloats - c0 * CHK) < (uint64_t)nb * CHK ? (nfloats - c0 * CHK) : (uint64_t)nb * CHK;
        const uint32_t fstart = (first_chunk + c0 == 0) ? 1u : 0u;
        const uint32_t *bin = in + c0 * CHK;
        /* the whole batch as one lane on the compute stream: workspace rows 0 .. 4 nb - 1, sizes only (no output pointer is used) */
        if (int rc = compress_lane(ctx, lstream, 0, 0, 0u, bin, bfl, nb, mask, fstart, (uint8_t *)NULL, xf, ae, cleared)) return rc;
        LAUNCH("k_probe_sizes", k_probe_sizes, dim3(1), dim3(256), ctx->sinfo, nb, ctx->result);
        if (!d_acc) continue;
        const uint64_t bbase = (first_chunk + c0) * (uint64_t)CHK;
        if (xf == Xform::Quant) LAUNCH("k_probe_fold", k_probe_fold<Xform::Quant>, dim3(CMP_WGS, nb), dim3(256), bin, bbase, bfl, mask, eps_abs, eps_rel, ctx->cmp_part);
        else if (xf == Xform::AbsErr) LAUNCH("k_probe_fold", k_probe_fold<Xform::AbsErr>, dim3(CMP_WGS, nb), dim3(256), bin, bbase, bfl, ae, eps_abs, eps_rel, ctx->cmp_part);
        else LAUNCH("k_probe_fold", k_probe_fold<Xform::Mask>, dim3(CMP_WGS, nb), dim3(256), bin, bbase, bfl, mask, eps_abs, eps_rel, ctx->cmp_part);
        LAUNCH("k_compare_chunk", k_compare_chunk, dim3(nb), dim3(64), ctx->cmp_part, bbase, bfl, (uint32_t)CHK, first_chunk + c0, d_acc);
    }
    HIPCHK(hipMemcpyAsync(h_res, ctx->result, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_probe_chunks(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int xform, int bits, float eps,
                                 double eps_abs, double eps_rel, mrcz_compare_t *d_acc, uint64_t *out_len, uint64_t plane_bytes[4])
{
    if (!ctx || !out_len) return MRCZ_EINVAL;
    *out_len = 0;
    if (int rc = probe_enqueue(ctx, d_in, nfloats, first_chunk, xform, bits, eps, eps_abs, eps_rel, d_acc, ctx->h_result)) return rc;
    if (nfloats == 0) return MRCZ_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream), "stream sync (probe)");
    *out_len = ctx->h_result[0];
    if (plane_bytes)
        for (int j = 0; j < 4; j++) plane_bytes[j] = ctx->h_result[1 + j];
    return MRCZ_OK;
}

extern "C" int mrcz_probe_chunks_async(mrcz_ctx_t *ctx, const void *d_in, uint64_t nfloats, uint64_t first_chunk, int xform, int bits, float eps,
                                       double eps_abs, double eps_rel, mrcz_compare_t *d_acc, uint64_t *h_result5)
{
    return probe_enqueue(ctx, d_in, nfloats, first_chunk, xform, bits, eps, eps_abs, eps_rel, d_acc, h_result5);
}
