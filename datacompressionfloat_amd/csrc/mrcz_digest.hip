/*
 * mrcz_digest.hip -- digest decode (include/mrcz_hip.h, mrcz_uncompress_digest / mrcz_digest_words): the standard CRC-32 (zlib,
 * gzip, PNG: reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF) of the bytes every chunk of a container
 * decodes to, streaming the chunks through a context of fixed size.
 *
 * Included from mrcz_api.hip after the compare decode (it uses the context, decode_batch and the staging buffer as that does).
 * Per run of up to max_chunks consecutive chunks: decode_batch, k_merge_segments<false> into the staging buffer, k_crc_fold
 * (CRC_WGS workgroups per chunk, each writes the remainder of its slice to its own slot of ctx->crc_part with plain stores),
 * k_crc_chunk (one wave per chunk combines the chunk's slice remainders and assigns the chunk's mrcz_digest_t to d_acc[chunk]).
 *
 * Arithmetic.  A 32-bit value is a polynomial over GF(2) of degree < 32 in the reflected order of zlib: bit 31 is x^0, bit 0 is
 * x^31, so a little-endian word of the file read as uint32_t IS the polynomial of its four bytes.  raw(M) = M(x) x^32 mod P is
 * the CRC register after M from a zero initial value; raw(A || B) = raw(A) x^(8 |B|) xor raw(B), and
 * crc32(M) = raw(M) xor 0xFFFFFFFF x^(8 |M|) xor 0xFFFFFFFF.  Everything is exact: any cut into slices, lanes, batches or calls
 * gives the same bits.
 *
 * How a slice is reduced (there is no carry-less multiply on gfx950).  A slice is n whole 16-byte groups.  Thread t of the
 * 1024 takes groups t, t + 1024, t + 2048, ... of the slice (so a wave-instruction loads 1 KiB contiguous), zero groups being put
 * in FRONT of the slice so that every thread takes the same number J (zeros in front change no remainder that starts from zero).
 * A thread keeps one accumulator per word of the group and steps it by Horner's rule with the stride as the constant:
 * a_k = a_k x^(128 * 1024) xor w_k.  Multiplying a 32-bit polynomial by a constant mod P is four table lookups (one 256-entry
 * table per byte of the operand) and three xors: one 4-byte LDS gather per input byte, the cost of slice-by-4, but the four chains
 * of a thread are independent of one another, and nothing crosses lanes inside the loop.  The gathers are uniformly random
 * indices, which on one shared table are expected to replay on bank conflicts (balls into bins: about 3.5 lanes of a 32-lane group on
 * the fullest bank; not measured);
 * so the 4 KiB of tables are stored 32 times, entry (k, b) of lane l at dword ((k * 256 + b) * 32 + (l mod 32)): every lane of a
 * ds_read_b32 group then reads its own bank and no gather ever conflicts.  That is 128 KiB of LDS, one 1024-thread workgroup per
 * CU (4 waves per SIMD), filled once per workgroup from a table in constant memory (per workgroup 32 K dword stores against the 786 K
 * gathers of a full chunk's slice).  After the loop a thread folds its four accumulators into one (three multiplications by x^32
 * through an unreplicated table), multiplies by x^(128 (1023 - t) + 32), its distance from the end of the slice (a table of
 * 1024 constants; the product is a 32-step shift-and-xor in VALU, once per thread), and the workgroup xors the results.
 */

namespace mrcz {

constexpr uint32_t CRC_WGS = 32;   /* workgroups (slices) per chunk: a constant of the source */
constexpr uint32_t CRC_T = 1024;   /* threads of a k_crc_fold workgroup; the Horner stride is CRC_T groups */
constexpr uint32_t CRC_ROW = CRC_WGS + 4u; /* workspace words per chunk: CRC_WGS slice remainders, then the 0..3 words behind the last whole group */
constexpr uint32_t CRC_POLY = 0xEDB88320u;

/* a x mod P */
__host__ __device__ constexpr uint32_t crc_mulx(uint32_t a) { return (a >> 1) ^ ((a & 1u) ? CRC_POLY : 0u); }
/* a b mod P */
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= ((a >> i) & 1u) ? b : 0u;
        b = crc_mulx(b);
    }
    return p;
}

/* sq[i] = x^(2^i) mod P */
struct CrcSquares { uint32_t sq[64]; };
constexpr CrcSquares crc_make_squares()
{
    CrcSquares r{};
    uint32_t s = 0x40000000u; /* x */
    for (int i = 0; i < 64; i++) { r.sq[i] = s; s = crc_mul(s, s); }
    return r;
}
static __device__ const CrcSquares crc_squares = crc_make_squares();
/* x^n mod P (n in bits) */
__device__ __forceinline__ uint32_t crc_xpow(uint64_t n)
{
    uint32_t r = 0x80000000u; /* 1 */
    for (int i = 0; n; i++, n >>= 1)
        if (n & 1u) r = crc_mul(r, crc_squares.sq[i]);
    return r;
}
constexpr uint32_t crc_xpow_const(uint64_t n)
{
    uint32_t r = 0x80000000u, s = 0x40000000u;
    for (; n; n >>= 1) { if (n & 1u) r = crc_mul(r, s); s = crc_mul(s, s); }
    return r;
}

/* t[k * 256 + b] = (b << 8 k) C mod P: v C mod P = t[v & 255] ^ t[256 + (v >> 8 & 255)] ^ t[512 + (v >> 16 & 255)] ^ t[768 + (v >> 24)] */
struct CrcTab { uint32_t t[1024]; };
static_assert(CRC_T == 1024u, "k_crc_fold copies one entry of a CrcTab per thread");
constexpr CrcTab crc_make_tab(uint32_t C)
{
    CrcTab r{};
    for (uint32_t k = 0; k < 4; k++)
        for (uint32_t b = 0; b < 256; b++) r.t[k * 256 + b] = crc_mul(b << (8 * k), C);
    return r;
}
static __device__ const CrcTab crc_tab32 = crc_make_tab(crc_xpow_const(32));                      /* by x^32: one word further */
static __device__ const CrcTab crc_tab_stride = crc_make_tab(crc_xpow_const(128ull * CRC_T));     /* by x^(128 CRC_T): one stride further */
/* p[t] = x^(128 (CRC_T - 1 - t) + 32): what a thread's last group has behind it in the slice, and the x^32 of raw() */
struct CrcLanePow { uint32_t p[CRC_T]; };
constexpr CrcLanePow crc_make_lane_pow()
{
    CrcLanePow r{};
    const uint32_t g = crc_xpow_const(128);
    uint32_t v = crc_xpow_const(32);
    for (uint32_t t = CRC_T; t-- > 0;) { r.p[t] = v; v = crc_mul(v, g); }
    return r;
}
static __device__ const CrcLanePow crc_lane_pow = crc_make_lane_pow();

/* What a word becomes before it enters the CRC: nothing (decoded words, plain files), or what a container written from it with
 * -b bits / -e eps / -s int decodes to.  File words < 256 are exempt (data = false). */
enum class CrcXform { None, Mask, AbsErr, Int8 };
struct CrcArg {
    uint32_t mask;
    AbsErr ae;
};
template <CrcXform X> __device__ __forceinline__ uint32_t crc_xform(uint32_t w, bool data, const CrcArg &a)
{
    if constexpr (X == CrcXform::Mask) return data ? (w & a.mask) : w;
    else if constexpr (X == CrcXform::AbsErr) return data ? abs_round(w, a.ae.q, a.ae.E) : w;
    else if constexpr (X == CrcXform::Int8) return data ? dequant_int8(quant_int8(w)) : w;
    else return w;
}

/* the slice of workgroup w of a chunk of cl words: whole groups [g0, g1) */
__device__ __forceinline__ void crc_slice(uint32_t cl, uint32_t w, uint32_t &g0, uint32_t &g1)
{
    const uint32_t gf = cl >> 2, per = (gf + CRC_WGS - 1u) / CRC_WGS;
    g0 = w * per < gf ? w * per : gf;
    g1 = g0 + per < gf ? g0 + per : gf;
}

/* grid (CRC_WGS, nb): workgroup (w, k) reduces its slice of chunk k of the run (words holds the run's words from file word bbase
 * on, bfl of them) to part[k * CRC_ROW + w]; workgroup (0, k) also copies the chunk's 0..3 words behind its last whole group,
 * transformed, to part[k * CRC_ROW + CRC_WGS ..] */
template <CrcXform X>
__global__ __launch_bounds__(1024) void k_crc_fold(const uint32_t *__restrict__ words, uint64_t bbase, uint64_t bfl, uint32_t chk, CrcArg arg,
                                                   uint32_t *__restrict__ part)
{
    __shared__ uint32_t tab[1024 * 32]; /* crc_tab_stride, one copy per bank */
    __shared__ uint32_t tab32[1024];
    __shared__ uint32_t shw[CRC_T / 64];
    const uint32_t k = blockIdx.y, w = blockIdx.x, t = threadIdx.x;
    const uint64_t cb = (uint64_t)k * chk;                                    /* the chunk's first word in the run */
    const uint32_t cl = (uint32_t)(bfl - cb < chk ? bfl - cb : chk);          /* its words */
    const uint64_t fw = bbase + cb;                                           /* its first file word */
    const uint32_t nhdr = fw >= 256u ? 0u : (uint32_t)(256u - fw);            /* chunk words < nhdr are header words */
    const bool vec = (chk & 3u) == 0u;                                        /* then every chunk base is 16-byte aligned */
    const uint32_t *__restrict__ wp = words + cb;
    uint32_t g0, g1;
    crc_slice(cl, w, g0, g1);
    if (w == 0u && t < 3u) {
        const uint32_t i = (cl & ~3u) + t;
        part[(uint64_t)k * CRC_ROW + CRC_WGS + t] = i < cl ? crc_xform<X>(wp[i], i >= nhdr, arg) : 0u;
    }
    for (uint32_t i = t; i < 1024u * 32u; i += CRC_T) tab[i] = crc_tab_stride.t[i >> 5];
    tab32[t] = crc_tab32.t[t];
    __syncthreads();
    const uint32_t n = g1 - g0;
    const uint32_t J = ((n + 4u * CRC_T - 1u) / (4u * CRC_T)) * 4u;           /* groups per thread, a multiple of the unroll */
    const uint32_t pad = J * CRC_T - n;                                       /* zero groups in front of the slice */
    const uint32_t *tb = tab + (t & 31u);
    uint32_t a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u;
#define CRC_STRIDE(a) (tb[((a) & 0xffu) << 5] ^ tb[(256u + (((a) >> 8) & 0xffu)) << 5] ^ tb[(512u + (((a) >> 16) & 0xffu)) << 5] ^ tb[(768u + ((a) >> 24)) << 5])
    for (uint32_t j = 0; j < J; j += 4u) {
        uint4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) { /* the four loads first: they do not depend on the accumulators */
            const uint32_t q = t + CRC_T * (j + u);
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (q >= pad) {
                const uint32_t i = (g0 + (q - pad)) << 2;
                if (vec) v[u] = *reinterpret_cast<const uint4 *>(wp + i);
                else v[u] = make_uint4(wp[i], wp[i + 1u], wp[i + 2u], wp[i + 3u]); /* a chunk size that is no multiple of four */
                if constexpr (X != CrcXform::None) {
                    v[u].x = crc_xform<X>(v[u].x, i >= nhdr, arg);
                    v[u].y = crc_xform<X>(v[u].y, i + 1u >= nhdr, arg);
                    v[u].z = crc_xform<X>(v[u].z, i + 2u >= nhdr, arg);
                    v[u].w = crc_xform<X>(v[u].w, i + 3u >= nhdr, arg);
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            a0 = CRC_STRIDE(a0) ^ v[u].x;
            a1 = CRC_STRIDE(a1) ^ v[u].y;
            a2 = CRC_STRIDE(a2) ^ v[u].z;
            a3 = CRC_STRIDE(a3) ^ v[u].w;
        }
    }
#undef CRC_STRIDE
#define CRC_X32(a) (tab32[(a) & 0xffu] ^ tab32[256u + (((a) >> 8) & 0xffu)] ^ tab32[512u + (((a) >> 16) & 0xffu)] ^ tab32[768u + ((a) >> 24)])
    uint32_t r = a0;                       /* a0 x^96 + a1 x^64 + a2 x^32 + a3 */
    r = CRC_X32(r) ^ a1;
    r = CRC_X32(r) ^ a2;
    r = CRC_X32(r) ^ a3;
#undef CRC_X32
    r = crc_mul(r, crc_lane_pow.p[t]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) r ^= __shfl_xor(r, m);
    if ((t & 63u) == 0u) shw[t >> 6] = r;
    __syncthreads();
    if (t == 0u) {
        for (uint32_t i = 1; i < CRC_T / 64u; i++) r ^= shw[i];
        part[(uint64_t)k * CRC_ROW + w] = r;
    }
}

/* grid (nb), one wave: chunk k's slice remainders, in slice order, and its last 0..3 words -> acc[c_first + k] */
__global__ __launch_bounds__(64) void k_crc_chunk(const uint32_t *__restrict__ part, uint64_t bfl, uint32_t chk, uint64_t c_first,
                                                  mrcz_digest_t *__restrict__ acc)
{
    static_assert(CRC_WGS + 4u <= 64u, "one lane per slice, three for the last words, one for the initial value");
    const uint32_t k = blockIdx.x, l = threadIdx.x;
    const uint64_t cb = (uint64_t)k * chk;
    const uint32_t cl = (uint32_t)(bfl - cb < chk ? bfl - cb : chk);
    const uint32_t nt = cl & 3u;
    uint32_t v = 0u;
    if (l < CRC_WGS) { /* slice l has 4 cl - 16 g1 bytes behind it */
        uint32_t g0, g1;
        crc_slice(cl, l, g0, g1);
        v = crc_mul(part[(uint64_t)k * CRC_ROW + l], crc_xpow(8ull * (4ull * cl - 16ull * g1)));
    } else if (l < CRC_WGS + nt) { /* raw(word) = word x^32, and the words behind it */
        const uint32_t i = l - CRC_WGS;
        v = crc_mul(part[(uint64_t)k * CRC_ROW + l], crc_xpow(32ull + 32ull * (nt - 1u - i)));
    } else if (l == CRC_WGS + 3u) { /* the initial value 0xFFFFFFFF carried over the chunk's 32 cl bits, and the final xor */
        v = crc_mul(0xFFFFFFFFu, crc_xpow(32ull * cl)) ^ 0xFFFFFFFFu;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m);
    if (l != 0u) return;
    mrcz_digest_t r;
    r.crc32 = v;
    r.reserved = 0u;
    r.nbytes = 4ull * cl;
    acc[c_first + k] = r;
}

} /* namespace mrcz */

/* ---- host side ---- */

static int ensure_crc_part(mrcz_ctx *ctx)
{
    if (ctx->crc_part) return MRCZ_OK;
    hipError_t e = hipMalloc((void **)&ctx->crc_part, (size_t)ctx->max_chunks * CRC_ROW * sizeof(uint32_t));
    if (e != hipSuccess) { ctx->crc_part = NULL; return fail(ctx, MRCZ_ENOMEM, "digest partials", e); }
    return MRCZ_OK;
}

/* fold nb chunks (bfl words from file word bbase on) of `words` into acc[c_first ..] on the compute stream */
template <CrcXform X>
static int digest_launch(mrcz_ctx *ctx, const uint32_t *words, uint64_t bbase, uint64_t bfl, uint32_t chk, uint32_t nb, uint64_t c_first, CrcArg arg,
                         mrcz_digest_t *acc)
{
    hipStream_t lstream = ctx->stream;
    LAUNCH("k_crc_fold", k_crc_fold<X>, dim3(CRC_WGS, nb), dim3(CRC_T), words, bbase, bfl, chk, arg, ctx->crc_part);
    LAUNCH("k_crc_chunk", k_crc_chunk, dim3(nb), dim3(64), ctx->crc_part, bfl, chk, c_first, acc);
    return MRCZ_OK;
}

static int uncompress_digest_enqueue(mrcz_ctx *ctx, const uint8_t *rec, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                     uint64_t nchunks, int int_mode, mrcz_digest_t *acc)
{
    hipStream_t lstream = ctx->stream;
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    const uint64_t end = first_chunk + nchunks;
    CrcArg none = {};
    for (uint64_t c = first_chunk; c < end;) {
        const uint32_t nb = (uint32_t)((end - c) < ctx->max_chunks ? (end - c) : ctx->max_chunks);
        const uint64_t bbase = c * chk, bfl = (nfloats_file - bbase) < (uint64_t)nb * chk ? (nfloats_file - bbase) : (uint64_t)nb * chk;
        if (int rc = decode_batch(ctx, rec, len, bfl, nb, chk)) return rc;
        LAUNCH("k_merge_segments", k_merge_segments<false>, dim3(512, nb), dim3(256), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx,
               bfl, chk, ctx->stage, len, (uint64_t)4 * ctx->row_chunks * CHK, int_mode ? 1u : 0u, bbase, (int64_t)0, (uint64_t)0);
        if (int rc = digest_launch<CrcXform::None>(ctx, ctx->stage, bbase, bfl, chk, nb, c, none, acc)) return rc;
        c += nb;
    }
    HIPCHK(hipMemcpyAsync(ctx->h_result, ctx->result, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_digest(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk,
                                      uint64_t first_chunk, uint64_t nchunks, int int_mode, mrcz_digest_t *d_acc)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EFORMAT, "chunk size in header exceeds CHUNK_SIZE (constant.h:25)", hipSuccess);
    const uint64_t nchunks_file = (nfloats_file + chk - 1) / chk;
    if (first_chunk > nchunks_file || nchunks > nchunks_file - first_chunk) return fail(ctx, MRCZ_EINVAL, "chunks past the end of the file", hipSuccess);
    if (!d_acc || (nchunks && !d_records)) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (nchunks == 0) return MRCZ_OK;
    if ((uintptr_t)d_acc & 7u) return fail(ctx, MRCZ_EINVAL, "d_acc must be 8-byte aligned", hipSuccess);
    if (int rc = uncompress_prepare(ctx, d_records, chk, NULL)) return rc;
    if (!ctx->stage) { /* k_merge_segments<false> writes a batch's words here for k_crc_fold */
        hipError_t e = hipMalloc((void **)&ctx->stage, (size_t)ctx->max_chunks * CHK * 4u);
        if (e != hipSuccess) { ctx->stage = NULL; return fail(ctx, MRCZ_ENOMEM, "staging buffer", e); }
    }
    if (int rc = ensure_crc_part(ctx)) return rc;
    int rc = uncompress_digest_enqueue(ctx, (const uint8_t *)d_records, len, nfloats_file, chk, first_chunk, nchunks, int_mode, d_acc);
    if (rc == MRCZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, MRCZ_EHIP, "stream sync (uncompress digest)", hipSuccess);
    if (rc != MRCZ_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    latch_fallbacks(ctx);
    if (ctx->h_result[1]) return fail(ctx, MRCZ_EFORMAT, "malformed chunk records or deflate stream", hipSuccess);
    return MRCZ_OK;
}

extern "C" int mrcz_digest_words_async(mrcz_ctx_t *ctx, const void *d_words, uint64_t nwords, uint64_t first_chunk, uint32_t chk, int xform, int bits,
                                       float eps, mrcz_digest_t *d_acc)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EINVAL, "chunk size of 0 or above CHUNK_SIZE", hipSuccess);
    if (xform != MRCZ_DIGEST_NONE && xform != MRCZ_DIGEST_MASK && xform != MRCZ_DIGEST_INT8 && xform != MRCZ_DIGEST_ABS)
        return fail(ctx, MRCZ_EINVAL, "unknown digest transform", hipSuccess);
    CrcArg arg = {};
    if (xform == MRCZ_DIGEST_MASK) {
        if (bits < 0 || bits > 32) return fail(ctx, MRCZ_EINVAL, "bits outside 0..32", hipSuccess);
        arg.mask = mask_of(bits);
    }
    if (xform == MRCZ_DIGEST_ABS)
        if (int rc = abs_err_param(ctx, eps, &arg.ae)) return rc;
    if (!d_acc || (nwords && !d_words)) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (nwords == 0) return MRCZ_OK;
    if (((uintptr_t)d_words & 15u) || ((uintptr_t)d_acc & 7u)) return fail(ctx, MRCZ_EINVAL, "d_words must be 16-byte and d_acc 8-byte aligned", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (int rc = ensure_crc_part(ctx)) return rc;
    const uint32_t *words = (const uint32_t *)d_words;
    const uint64_t nchunks = (nwords + chk - 1) / chk;
    for (uint64_t c = 0; c < nchunks;) {
        const uint32_t nb = (uint32_t)((nchunks - c) < ctx->max_chunks ? (nchunks - c) : ctx->max_chunks);
        const uint64_t bfl = (nwords - c * chk) < (uint64_t)nb * chk ? (nwords - c * chk) : (uint64_t)nb * chk;
        const uint64_t bbase = (first_chunk + c) * chk;
        int rc;
        if (xform == MRCZ_DIGEST_MASK) rc = digest_launch<CrcXform::Mask>(ctx, words + c * chk, bbase, bfl, chk, nb, first_chunk + c, arg, d_acc);
        else if (xform == MRCZ_DIGEST_ABS) rc = digest_launch<CrcXform::AbsErr>(ctx, words + c * chk, bbase, bfl, chk, nb, first_chunk + c, arg, d_acc);
        else if (xform == MRCZ_DIGEST_INT8) rc = digest_launch<CrcXform::Int8>(ctx, words + c * chk, bbase, bfl, chk, nb, first_chunk + c, arg, d_acc);
        else rc = digest_launch<CrcXform::None>(ctx, words + c * chk, bbase, bfl, chk, nb, first_chunk + c, arg, d_acc);
        if (rc) return rc;
        c += nb;
    }
    return MRCZ_OK;
}

extern "C" int mrcz_digest_words(mrcz_ctx_t *ctx, const void *d_words, uint64_t nwords, uint64_t first_chunk, uint32_t chk, int xform, int bits, float eps,
                                 mrcz_digest_t *d_acc)
{
    if (int rc = mrcz_digest_words_async(ctx, d_words, nwords, first_chunk, chk, xform, bits, eps, d_acc)) return rc;
    if (nwords) HIPCHK(hipStreamSynchronize(ctx->stream), "stream sync (digest words)");
    return MRCZ_OK;
}

/* crc32(A || B) from crc32(A), crc32(B) and |B|: crc(A) x^(8 |B|) xor crc(B) (the initial-value and final-xor terms of the three
 * cancel).  x^(8 n) = (x^8)^n by squaring, so n may be any 64-bit count. */
extern "C" uint32_t mrcz_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t nbytes_b)
{
    uint32_t r = 0x80000000u, s = 0x00800000u; /* 1, x^8 */
    for (uint64_t n = nbytes_b; n; n >>= 1) {
        if (n & 1u) r = crc_mul(r, s);
        s = crc_mul(s, s);
    }
    return crc_mul(crc_a, r) ^ crc_b;
}

extern "C" int mrcz_digest_finish(mrcz_ctx_t *ctx, const mrcz_digest_t *d_acc, uint64_t first_chunk, uint64_t nchunks, mrcz_digest_t *h_total)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (!d_acc || !h_total) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    memset(h_total, 0, sizeof(*h_total)); /* the CRC-32 of no bytes is 0 */
    if (nchunks == 0) return MRCZ_OK;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    mrcz_digest_t *h = (mrcz_digest_t *)malloc((size_t)nchunks * sizeof(*h));
    if (!h) return fail(ctx, MRCZ_ENOMEM, "chunk digests", hipSuccess);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d_acc + first_chunk, (size_t)nchunks * sizeof(*h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(h); return fail(ctx, MRCZ_EHIP, "copy chunk digests", e); }
    for (uint64_t c = 0; c < nchunks; c++) {
        h_total->crc32 = mrcz_crc32_combine(h_total->crc32, h[c].crc32, h[c].nbytes);
        h_total->nbytes += h[c].nbytes;
    }
    free(h);
    return MRCZ_OK;
}
