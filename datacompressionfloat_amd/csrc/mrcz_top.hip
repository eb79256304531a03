/*
 * mrcz_top.hip -- top-planes decode (include/mrcz_hip.h, mrcz_uncompress_top / mrcz_record_top_span): the `keep` (2 or 3) most
 * significant byte planes of every word of a run of chunks, the other planes neither read nor decoded.  Plane 3 of a float32 is
 * its sign and seven exponent bits, plane 2 the last exponent bit and the top seven mantissa bits: planes 3 and 2 of a word ARE
 * its bfloat16 truncation.  A chunk record is its 16-byte header followed by the payloads of planes 0, 1, 2, 3, so the kept
 * payloads are the tail of the record and the header says where that tail begins.
 *
 * Included from mrcz_api.hip after the digest decode (it uses the context and decode_streams as the other decode modes do).  Per run
 * of up to max_chunks consecutive chunks: k_parse_top (the record walk: a compact stream table of `keep` streams per chunk,
 * stream keep * c + p = plane 4 - keep + p of chunk c), decode_streams with ns = keep * nb (candidate scan, validation, block
 * decode, chain, sequential decoders: none of them knows which plane a stream is), k_merge_top<KEEP, OUT16>.
 *
 * k_merge_top: one workgroup of KEEP waves per tile of MTILE positions.  Wave p gathers kept plane p of the tile from its
 * segments into LDS exactly as a wave of k_merge_segments does (a private copy of that loop: the full merge's instructions stay
 * what they are); then every thread transposes: F32, four words (one dword of each kept plane, the dropped planes' bytes zero)
 * to one 16-byte store; U16 (KEEP 2), eight words (one 8-byte LDS read of each plane) to one 16-byte store of eight bfloat16 bit
 * patterns.  LDS: consecutive lanes read consecutive dwords (or 8-byte pairs) of a plane's row, and wrote consecutive 16-byte
 * groups: no bank conflicts either way.  Global: a wave-instruction stores 1 KiB contiguous.  Bytes moved per position at KEEP 2,
 * U16: 2 read + 2 written, against 4 + 4 of the full merge.
 */

namespace mrcz {

/* The record walk of top-planes decode: k_parse_records for `keep` kept planes.  thinned = the records hold their header and the
 * kept payloads only.  The lengths of all four planes are checked against what a record can hold (the header is read whole); the
 * dropped payloads are stepped over (ordinary records) or absent (thinned), never read. */
__global__ void k_parse_top(const uint8_t *__restrict__ rec, uint64_t len, uint64_t nfloats, uint32_t chk,
                            DecStream *__restrict__ ds, uint64_t *__restrict__ result /* [0] consumed, [1] error */,
                            uint32_t lz4_planes, uint32_t keep, uint32_t thinned)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t off = result[0]; /* where the previous batch of this call stopped (0 for the first) */
    uint64_t err = 0;
    const uint64_t nchunks = (nfloats + chk - 1) / chk;
    const uint32_t drop = 4u - keep;
    uint64_t c = 0;
    for (; c < nchunks; c++) {
        const uint64_t left = nfloats - c * chk;
        const uint32_t n = (uint32_t)(left < chk ? left : chk);
        if (off + 16 > len) { err = 1; break; }
        uint64_t p = off + 16;
        DecStream d3[3];
        for (uint32_t j = 0; j < 4u; j++) {
            const uint8_t *h = rec + off + 4 * j;
            const uint32_t raw = (h[3] & 0x80u) >> 7;
            const uint32_t l = (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16) | ((uint32_t)(h[3] & 0x7fu) << 24);
            if ((raw && l < n) || (!raw && l > CHK + (CHK >> 3) + 1024u)) err = 1;
            if (j < drop) { /* a dropped plane: its length moves the walk of ordinary records and nothing else */
                if (!thinned) p += l;
                continue;
            }
            DecStream &d = d3[j - drop];
            d.payoff = p; d.paylen = l; d.raw = raw ? 1u : (((lz4_planes >> j) & 1u) ? 2u : 0u); d.n = n; d.pad = 0;
            if (p + l > len) err = 1;
            p += l;
        }
        if (err) break;
        for (uint32_t j = 0; j < keep; j++) ds[keep * c + j] = d3[j];
        off = p;
    }
    /* as k_parse_records: from the first bad chunk on the kernels queued behind this one get empty streams */
    for (; c < nchunks; c++)
        for (uint32_t j = 0; j < keep; j++) {
            DecStream d;
            d.payoff = 0; d.paylen = 0; d.raw = 0; d.n = 0; d.pad = 0;
            ds[keep * c + j] = d;
        }
    result[0] = off;
    if (err) result[1] = err; /* sticky across the batches of a call */
}

/* grid (tiles, nb), KEEP waves: kept plane p of chunk c is stream KEEP * c + p.  out: OUT16 ? uint16_t : uint32_t per word, the
 * batch's first word at out[0]. */
template <int KEEP, bool OUT16>
__global__ __launch_bounds__(64 * KEEP) void k_merge_top(const uint8_t *__restrict__ rec, const uint8_t *__restrict__ scratch,
                                                         const uint8_t *__restrict__ planes, const Seg *__restrict__ segs,
                                                         const uint32_t *__restrict__ nseg, const uint16_t *__restrict__ segidx,
                                                         uint64_t nfloats, uint32_t chk, void *__restrict__ out, uint64_t reclen,
                                                         uint64_t planes_bytes)
{
    static_assert(KEEP == 2 || KEEP == 3, "two or three top planes");
    static_assert(!OUT16 || KEEP == 2, "16-bit words hold two planes");
    constexpr uint32_t NT = 64u * KEEP;
    __shared__ __attribute__((aligned(16))) uint4 tile[KEEP][MTILE / 16];
    const uint32_t c = blockIdx.y;
    const uint64_t cbase = (uint64_t)c * chk;
    const uint32_t n = (uint32_t)((nfloats - cbase) < chk ? (nfloats - cbase) : chk);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t s = (uint32_t)KEEP * c + (uint32_t)__builtin_amdgcn_readfirstlane(w);
    const Seg *sg = segs + (size_t)s * MAXSEG;
    const uint32_t ns = nseg[s];
    SegBases sb;
    sb.rec = rec; sb.scratch = scratch; sb.planes = planes; sb.reclen = reclen; sb.planes_bytes = planes_bytes;
    /* the segment logic of k_merge_segments: three segments per tile by wave-uniform loads, the next tile's looked up while this
     * tile's data is in flight */
    constexpr int NSEGF = 3;
    Seg ZS;
    ZS.src = 0; ZS.dst = 0; ZS.len = 0; ZS.fill_until = 0; ZS.fillb = 0;
    uint32_t k0n = 0;
    Seg Sn[NSEGF];
#pragma unroll
    for (int i = 0; i < NSEGF; i++) Sn[i] = ZS;
    if ((uint64_t)blockIdx.x * MTILE < n) {
        k0n = ns ? (uint32_t)__builtin_amdgcn_readfirstlane((int)segidx[(size_t)s * MTILES + blockIdx.x]) : 0u;
#pragma unroll
        for (int i = 0; i < NSEGF; i++) if (k0n + (uint32_t)i < ns) Sn[i] = sg[k0n + (uint32_t)i];
    }
    for (uint32_t t = blockIdx.x; (uint64_t)t * MTILE < n; t += gridDim.x) {
        const uint32_t p0 = t * MTILE, pend = (n - p0) < (uint32_t)MTILE ? n : p0 + MTILE;
        const uint32_t k0 = k0n;
        Seg S[NSEGF];
        const uint8_t *base[NSEGF];
        uint32_t send[NSEGF];
#pragma unroll
        for (int i = 0; i < NSEGF; i++) { S[i] = Sn[i]; base[i] = seg_base(sb, S[i].src); send[i] = S[i].dst + S[i].len; }
        const uint32_t tn = t + gridDim.x;
        const bool more = (uint64_t)tn * MTILE < n;
        if (more) k0n = ns ? (uint32_t)__builtin_amdgcn_readfirstlane((int)segidx[(size_t)s * MTILES + tn]) : 0u;
        /* a 16-byte group over the boundary of two consecutive segments is read once relative to each and blended */
        bool adj[NSEGF - 1];
#pragma unroll
        for (int i = 0; i + 1 < NSEGF; i++) adj[i] = S[i + 1].len != 0u && S[i + 1].dst == send[i] && S[i].len != 0u;
        uint4 v[MTILE / 16 / 64], v2[MTILE / 16 / 64];
        uint32_t kind[MTILE / 16 / 64]; /* 0 zero, 1 inside a segment, 3 straddles two, 4 general path, 5 inside a segment's fill; | segment number << 4 */
#pragma unroll
        for (int j = 0; j < MTILE / 16 / 64; j++) {
            const uint32_t g = (uint32_t)lane + 64u * (uint32_t)j, p = p0 + 16u * g;
            const bool whole = ns != 0u && p + 16u <= pend;
            uint32_t kd = (p < pend && ns) ? 4u : 0u;
            v[j] = make_uint4(0, 0, 0, 0);
            v2[j] = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int i = NSEGF - 1; i >= 0; i--) {
                if (whole && p >= S[i].dst && p + 16u <= send[i]) kd = (p + 16u <= S[i].fill_until ? 5u : 1u) | ((uint32_t)i << 4);
            }
#pragma unroll
            for (int i = NSEGF - 2; i >= 0; i--) {
                if (kd == 4u && whole && adj[i] && p >= S[i].dst && p < send[i] && p + 16u <= send[i + 1] && p >= S[i].fill_until && S[i + 1].fill_until <= S[i + 1].dst &&
                    seg_can_overread(sb, S[i].src, (int64_t)(p - S[i].dst)) && seg_can_overread(sb, S[i + 1].src, (int64_t)p - (int64_t)S[i + 1].dst)) kd = 3u | ((uint32_t)i << 4);
            }
            kind[j] = kd;
#pragma unroll
            for (int i = 0; i < NSEGF; i++) {
                if (kd == (1u | ((uint32_t)i << 4)) || kd == (3u | ((uint32_t)i << 4))) __builtin_memcpy(&v[j], base[i] + (p - S[i].dst), 16);
                if (i + 1 < NSEGF && kd == (3u | ((uint32_t)i << 4))) __builtin_memcpy(&v2[j], base[i + 1] + ((int64_t)p - (int64_t)S[i + 1].dst), 16);
            }
        }
#pragma unroll
        for (int i = 0; i < NSEGF; i++) { Sn[i] = ZS; if (more && k0n + (uint32_t)i < ns) Sn[i] = sg[k0n + (uint32_t)i]; }
#pragma unroll
        for (int j = 0; j < MTILE / 16 / 64; j++) {
            const uint32_t g = (uint32_t)lane + 64u * (uint32_t)j, p = p0 + 16u * g;
            const uint32_t kd = kind[j] & 15u, si = kind[j] >> 4;
            uint32_t fu = 0, fb = 0, se = 0;
#pragma unroll
            for (int i = 0; i < NSEGF; i++) if (si == (uint32_t)i) { fu = S[i].fill_until; fb = S[i].fillb & 0xffu; se = send[i]; }
            if (kd == 1u) {
                if (p < fu) {
                    const uint32_t fw = 0x01010101u * fb;
                    v[j] = blend16(make_uint4(fw, fw, fw, fw), v[j], fu - p >= 16u ? 16u : fu - p);
                }
            } else if (kd == 5u) {
                const uint32_t fw = 0x01010101u * fb;
                v[j] = make_uint4(fw, fw, fw, fw);
            } else if (kd == 3u) v[j] = blend16(v[j], v2[j], se - p);
            else if (kd == 4u) v[j] = merge_slow16(sb, sg, ns, p, pend, k0);
            tile[w][g] = v[j];
        }
        __syncthreads();
        if constexpr (OUT16) {
            /* eight words per thread: bytes 0..7 of the group in plane 2 (lo) and plane 3 (hi) -> eight (hi << 8 | lo) */
            uint16_t *o16 = reinterpret_cast<uint16_t *>(out);
            for (uint32_t q = threadIdx.x; q < (uint32_t)MTILE / 8u; q += NT) {
                const uint32_t i = p0 + 8u * q;
                if (i >= n) break;
                const uint2 lo = reinterpret_cast<const uint2 *>(tile[0])[q], hi = reinterpret_cast<const uint2 *>(tile[1])[q];
                uint4 o4;
                o4.x = __byte_perm(lo.x, hi.x, 0x5140);
                o4.y = __byte_perm(lo.x, hi.x, 0x7362);
                o4.z = __byte_perm(lo.y, hi.y, 0x5140);
                o4.w = __byte_perm(lo.y, hi.y, 0x7362);
                uint16_t *o = o16 + cbase + i;
                if (i + 8u <= n && (((uintptr_t)o) & 15u) == 0) *reinterpret_cast<uint4 *>(o) = o4;
                else { /* the tail of a short last chunk, or a chunk size that is no multiple of eight */
                    const uint32_t ov[4] = {o4.x, o4.y, o4.z, o4.w};
                    for (uint32_t k = 0; k < 8u && i + k < n; k++) o[k] = (uint16_t)(ov[k >> 1] >> (16u * (k & 1u)));
                }
            }
        } else {
            /* four words per thread: one dword of each kept plane; the dropped planes' bytes are zero */
            uint32_t *o32 = reinterpret_cast<uint32_t *>(out);
            for (uint32_t q = threadIdx.x; q < (uint32_t)MTILE / 4u; q += NT) {
                const uint32_t i = p0 + 4u * q;
                if (i >= n) break;
                const uint32_t b = KEEP == 3 ? reinterpret_cast<const uint32_t *>(tile[0])[q] : 0u;
                const uint32_t cc = reinterpret_cast<const uint32_t *>(tile[KEEP - 2])[q], dd = reinterpret_cast<const uint32_t *>(tile[KEEP - 1])[q];
                const uint32_t ab_lo = __byte_perm(0u, b, 0x5140), ab_hi = __byte_perm(0u, b, 0x7362);
                const uint32_t cd_lo = __byte_perm(cc, dd, 0x5140), cd_hi = __byte_perm(cc, dd, 0x7362);
                uint4 o4;
                o4.x = __byte_perm(ab_lo, cd_lo, 0x5410);
                o4.y = __byte_perm(ab_lo, cd_lo, 0x7632);
                o4.z = __byte_perm(ab_hi, cd_hi, 0x5410);
                o4.w = __byte_perm(ab_hi, cd_hi, 0x7632);
                uint32_t *o = o32 + cbase + i;
                if (i + 4u <= n && (((uintptr_t)o) & 15u) == 0) *reinterpret_cast<uint4 *>(o) = o4;
                else {
                    o[0] = o4.x;
                    if (i + 1u < n) o[1] = o4.y;
                    if (i + 2u < n) o[2] = o4.z;
                    if (i + 3u < n) o[3] = o4.w;
                }
            }
        }
        __syncthreads();
    }
}

} /* namespace mrcz */

/* ---- host side ---- */

/* where the kept payloads of a record begin and how long they are, from its 16-byte header; the checks of mrcz_record_size */
extern "C" int mrcz_record_top_span(const void *h_header16, uint32_t n, int keep, uint64_t *skip, uint64_t *bytes)
{
    if (!h_header16 || !skip || !bytes || (keep != 2 && keep != 3)) return MRCZ_EINVAL;
    const uint8_t *h = (const uint8_t *)h_header16;
    uint64_t sk = 16, kept = 0;
    for (int j = 0; j < 4; j++) {
        const uint32_t raw = h[4 * j + 3] >> 7;
        const uint32_t l = (uint32_t)h[4 * j] | ((uint32_t)h[4 * j + 1] << 8) | ((uint32_t)h[4 * j + 2] << 16) | ((uint32_t)(h[4 * j + 3] & 0x7fu) << 24);
        if ((raw && l < n) || (!raw && l > CHK + (CHK >> 3) + 1024u)) return MRCZ_EFORMAT;
        if (j < 4 - keep) sk += l; else kept += l;
    }
    *skip = sk;
    *bytes = kept;
    return MRCZ_OK;
}

static int uncompress_top_enqueue(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                  uint64_t nchunks, int keep, int flags, void *d_out, uint64_t *h_res)
{
    if (!ctx) return MRCZ_EINVAL;
    ctx->ntimers = 0;
    if (chk == 0 || chk > CHK) return fail(ctx, MRCZ_EFORMAT, "chunk size in header exceeds CHUNK_SIZE (constant.h:25)", hipSuccess);
    const uint64_t nchunks_file = (nfloats_file + chk - 1) / chk;
    if (first_chunk > nchunks_file || nchunks > nchunks_file - first_chunk) return fail(ctx, MRCZ_EINVAL, "chunks past the end of the file", hipSuccess);
    if (keep != 2 && keep != 3) return fail(ctx, MRCZ_EINVAL, "keep must be 2 or 3 planes", hipSuccess);
    if (flags & ~(MRCZ_TOP_U16 | MRCZ_TOP_THINNED)) return fail(ctx, MRCZ_EINVAL, "unknown flag bits", hipSuccess);
    const bool out16 = (flags & MRCZ_TOP_U16) != 0, thinned = (flags & MRCZ_TOP_THINNED) != 0;
    if (out16 && keep != 2) return fail(ctx, MRCZ_EINVAL, "16-bit words hold two planes: the U16 flag needs keep == 2", hipSuccess);
    if (!d_out || !h_res || (nchunks && !d_records)) return fail(ctx, MRCZ_EINVAL, "NULL pointer", hipSuccess);
    if (((uintptr_t)d_out & 15u) || ((uintptr_t)d_records & 3u)) return fail(ctx, MRCZ_EINVAL, "d_out must be 16-byte and d_records 4-byte aligned", hipSuccess);
    if (nchunks == 0) return MRCZ_OK;
    if (int rc = uncompress_prepare(ctx, d_records, chk, d_out)) return rc;
    hipStream_t lstream = ctx->stream;
    const uint8_t *rec = (const uint8_t *)d_records;
    HIPCHK(hipMemsetAsync(ctx->result, 0, 8 * sizeof(uint64_t), ctx->stream), "memset result");
    const uint64_t end = first_chunk + nchunks, planes_bytes = (uint64_t)4 * ctx->row_chunks * CHK;
    for (uint64_t c = first_chunk; c < end;) {
        const uint32_t nb = (uint32_t)((end - c) < ctx->max_chunks ? (end - c) : ctx->max_chunks);
        const uint64_t bbase = c * chk, bfl = (nfloats_file - bbase) < (uint64_t)nb * chk ? (nfloats_file - bbase) : (uint64_t)nb * chk;
        const uint64_t o0 = (c - first_chunk) * chk; /* the batch's first word in d_out */
        LAUNCH("k_parse_top", k_parse_top, dim3(1), dim3(64), rec, len, bfl, chk, ctx->dstreams, ctx->result, ctx->lz4_planes, (uint32_t)keep, thinned ? 1u : 0u);
        if (int rc = decode_streams(ctx, rec, len, (uint32_t)keep * nb)) return rc;
        if (out16)
            LAUNCH("k_merge_top", (k_merge_top<2, true>), dim3(512, nb), dim3(128), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx, bfl, chk,
                   (void *)((uint16_t *)d_out + o0), len, planes_bytes);
        else if (keep == 2)
            LAUNCH("k_merge_top", (k_merge_top<2, false>), dim3(512, nb), dim3(128), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx, bfl, chk,
                   (void *)((uint32_t *)d_out + o0), len, planes_bytes);
        else
            LAUNCH("k_merge_top", (k_merge_top<3, false>), dim3(512, nb), dim3(192), rec, ctx->scratch + 16, ctx->planes, ctx->segs, ctx->nseg, ctx->segidx, bfl, chk,
                   (void *)((uint32_t *)d_out + o0), len, planes_bytes);
        c += nb;
    }
    HIPCHK(hipMemcpyAsync(h_res, ctx->result, result_words(ctx, h_res) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream), "copy result");
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_top(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                   uint64_t nchunks, int keep, int flags, void *d_out, uint64_t *consumed)
{
    if (!ctx) return MRCZ_EINVAL;
    if (consumed) *consumed = 0;
    int rc = uncompress_top_enqueue(ctx, d_records, len, nfloats_file, chk, first_chunk, nchunks, keep, flags, d_out, ctx->h_result);
    if (rc != MRCZ_OK || nchunks == 0) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream), "stream sync (uncompress top)");
    if (consumed) *consumed = ctx->h_result[0];
    latch_fallbacks(ctx);
    if (ctx->h_result[1]) return fail(ctx, MRCZ_EFORMAT, "malformed chunk records or deflate stream", hipSuccess);
    return MRCZ_OK;
}

extern "C" int mrcz_uncompress_top_async(mrcz_ctx_t *ctx, const void *d_records, uint64_t len, uint64_t nfloats_file, uint32_t chk, uint64_t first_chunk,
                                         uint64_t nchunks, int keep, int flags, void *d_out, uint64_t *h_result3)
{
    return uncompress_top_enqueue(ctx, d_records, len, nfloats_file, chk, first_chunk, nchunks, keep, flags, d_out, h_result3);
}
