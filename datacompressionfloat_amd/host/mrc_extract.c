/*
 * mrc_extract.c -- range, box and binned decode from the command line: part of a container without reading or decoding the rest,
 * or a binned overview of it without a buffer of the volume's size.
 *
 *   mrc_extract -i vol.mrc.zip -o out.raw (-w first:count | -z z0:z1 | -B centers.txt -S bx[,by,bz] [-F fill] | -N f[,fy,fz]
 *               | -P keep [-H]) [-s float|int] [-g device]
 *
 *   -w first:count   words [first, first + count) of the decoded file (4 bytes each)
 *   -z z0:z1         sections [z0, z1) of a float32 (mode 2) MRC volume: nx, ny, nz, mode (bytes 0-15) and nsymbt (bytes 92-95)
 *                    come from the decoded first 256 words, the data start at byte 1024 + nsymbt
 *   -B centers.txt   boxes of a float32 MRC volume around particle centres, one "x y z" per line (blank lines and lines that
 *                    start with '#' are skipped); box i starts at round(c) - size / 2 per axis (mrcz_box_origins).  The output
 *                    is raw float32 in [N][bz][by][bx] order
 *   -S bx[,by,bz]    box size (one number: a cube)
 *   -F fill          value of the voxels outside the volume, default 0
 *   -N f | fx,fy,fz  a float32 MRC volume average-pooled by the bin factors (1 <= f <= the dimension; voxels of a trailing
 *                    remainder of an axis are ignored).  The output is raw float32 in [mz][my][mx] order, (mx, my, mz) =
 *                    (nx / fx, ny / fy, nz / fz): each voxel is the mean of its bin, summed in double in file order
 *   -P keep          the whole file at reduced precision: every word & (0xFFFFFFFF << 8 (4 - keep)), keep = 2 or 3 top byte planes
 *                    (2: the bfloat16 truncation of every float32).  The output is raw float32, all floor(fsz / 4) words of the
 *                    file, the 256 header words truncated like the rest.  Not with -s int (that data lives in plane 0)
 *   -H               with -P 2: raw 16-bit words instead, word >> 16 (bfloat16 bit patterns), 2 bytes each
 *   -s               decode mode, as mrc_tar -s (the container does not record it)
 *
 * The 17-byte file header and the 16-byte header of every chunk before the window are read with pread; then only the records of
 * the chunks that cover the window, which mrcz_uncompress_range decodes (in one call: the covering records and the window must
 * fit in device memory; the workspace is batched as in every decode).  -B reads the chunk headers up to the last chunk a box
 * touches (mrcz_boxes_chunks), then the records of every run of touched chunks, one mrcz_uncompress_boxes call per run.  -N reads
 * the chunk headers up to the last chunk the bins use (mrcz_bin_chunks), then the records of the used chunks in pieces of at
 * most the context's batch (16 chunks), one mrcz_uncompress_binned call per piece, and one mrcz_binned_finish.  -P reads every
 * chunk header, then per chunk the kept payloads alone (one pread of the record's tail, mrcz_record_top_span) into thinned
 * records, in pieces of the context's batch: not one byte of a dropped payload is read.  Not one of the
 * reference's front ends: mrc_tar and mrc_tarx keep the reference's command lines.
 */
#include "../../include/mrcz_hip.h"

#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#define MRC_HEADER_BYTES 1024u

static void usage(const char *prog)
{
    printf("\nUsage:\n\n\t%s -i <container> -o <output file> (-w <first>:<count> | -z <z0>:<z1> | -B <centres> -S <bx>[,<by>,<bz>] [-F <fill>]\n"
           "\t\t| -N <f>[,<fy>,<fz>] | -P <keep> [-H]) [-s float|int] [-g device]\nwhere:\n", prog);
    printf("\t-i\tcontainer written by mrc_tar -t zip\n\n");
    printf("\t-o\traw output: the decoded words of the window, 4 bytes each\n\n");
    printf("\t-w\twords [first, first + count) of the decoded file\n\n");
    printf("\t-z\tsections [z0, z1) of a float32 (mode 2) MRC volume\n\n");
    printf("\t-B\tboxes of a float32 (mode 2) MRC volume around the centres in this text file, one \"x y z\" per line;\n"
           "\t\toutput: raw float32, [N][bz][by][bx]\n\n");
    printf("\t-S\tbox size with -B: bx, or bx,by,bz\n\n");
    printf("\t-F\tvalue of box voxels outside the volume, default 0\n\n");
    printf("\t-N\ta float32 (mode 2) MRC volume binned (average-pooled) by f, or by fx,fy,fz; remainders are ignored;\n"
           "\t\toutput: raw float32, [nz / fz][ny / fy][nx / fx]\n\n");
    printf("\t-P\tthe whole file with only its <keep> = 2 or 3 top byte planes (2: bfloat16 precision, truncated); the low planes\n"
           "\t\tare not read; output: raw float32 with the dropped bytes zero\n\n");
    printf("\t-H\twith -P 2: raw 16-bit words (bfloat16 bit patterns) instead of float32\n\n");
    printf("\t-s\tdata type the container was written with, [float | int], default float\n\n");
    printf("\t-g\tHIP device, default 0\n\n");
}

/* errors leave with the reference's exit(-1) status (255), never through a signal; stdio is flushed by hand and no exit handlers
 * run (the HIP runtime's destructors are not needed to release anything a dying process holds) */
static void die(const char *what, mrcz_ctx_t *c)
{
    fprintf(stderr, "[%s:%d] ERROR: %s%s%s\n", __FILE__, __LINE__, what, c ? ": " : "", c ? mrcz_last_error(c) : "");
    fflush(stdout);
    fflush(stderr);
    _exit(255);
}

static int parse_pair(const char *s, uint64_t *a, uint64_t *b)
{
    char *e = NULL;
    errno = 0;
    if (*s < '0' || *s > '9') return -1;
    *a = strtoull(s, &e, 10);
    if (errno || *e != ':' || e[1] < '0' || e[1] > '9') return -1;
    *b = strtoull(e + 1, &e, 10);
    return (errno || *e) ? -1 : 0;
}

static void pread_all(int fd, void *buf, uint64_t n, uint64_t off, const char *what)
{
    uint8_t *p = (uint8_t *)buf;
    while (n) {
        const ssize_t r = pread(fd, p, n > (1u << 30) ? (1u << 30) : (size_t)n, (off_t)off);
        if (r <= 0) die(what, NULL);
        p += r; n -= (uint64_t)r; off += (uint64_t)r;
    }
}

struct container {
    int fd;
    uint64_t nfl; /* words of the decoded file */
    uint32_t chk;
    signed char ztypes[4];
};

/* words [w0, w1) of the file, decoded on the device, into a malloc'ed host buffer */
static uint32_t *decode_window(mrcz_ctx_t **pc, int device, const struct container *ct, uint64_t w0, uint64_t w1, int int_mode)
{
    const uint64_t chk = ct->chk, c_lo = w0 / chk, c_hi = (w1 + chk - 1) / chk;
    uint64_t off = MRCZ_FILE_HEADER_BYTES, start = 0;
    for (uint64_t c = 0; c < c_hi; c++) { /* 16 bytes per chunk up to the window's last one */
        uint8_t h[16];
        uint64_t bytes = 0;
        const uint64_t left = ct->nfl - c * chk;
        if (c == c_lo) start = off;
        pread_all(ct->fd, h, 16, off, "truncated container (chunk header)");
        if (mrcz_record_size(h, (uint32_t)(left < chk ? left : chk), &bytes) != MRCZ_OK) die("damaged chunk header", NULL);
        off += bytes;
    }
    const uint64_t len = off - start, n = w1 - w0;
    if (!*pc) {
        const uint64_t nch = c_hi - c_lo;
        if (mrcz_create(pc, device, (uint32_t)(nch < 16 ? nch : 16)) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
    }
    mrcz_ctx_t *c = *pc;
    if (mrcz_set_ztypes(c, ct->ztypes) != MRCZ_OK) die("byte stream compressor types", c);
    void *h_rec = NULL, *d_rec = NULL, *d_out = NULL;
    uint32_t *out = (uint32_t *)malloc(4 * n);
    if (!out || mrcz_host_malloc(c, &h_rec, len) || mrcz_dev_malloc(c, &d_rec, len) || mrcz_dev_malloc(c, &d_out, 4 * n)) die("out of memory", c);
    pread_all(ct->fd, h_rec, len, start, "truncated container (payload)");
    uint64_t consumed = 0;
    if (mrcz_copy_h2d(c, d_rec, h_rec, len) != MRCZ_OK) die("copy to the device", c);
    if (mrcz_uncompress_range(c, d_rec, len, ct->nfl, ct->chk, c_lo, w0, w1, d_out, int_mode, &consumed) != MRCZ_OK) die("range decode", c);
    if (mrcz_copy_d2h(c, out, d_out, 4 * n) != MRCZ_OK) die("copy from the device", c);
    mrcz_dev_free(c, d_out);
    mrcz_dev_free(c, d_rec);
    mrcz_host_free(c, h_rec);
    return out;
}

/* the float32 (mode 2) MRC volume of the container: data_word0, nx, ny, nz into g, from the decoded first 256 words (whether
 * the file holds all of it is the caller's check) */
static void mrc_volume(mrcz_ctx_t **pc, int device, const struct container *ct, mrcz_box_geom_t *g)
{
    if (ct->nfl < MRC_HEADER_BYTES / 4) die("file shorter than an MRC header", NULL);
    uint32_t *hdr = decode_window(pc, device, ct, 0, MRC_HEADER_BYTES / 4, 0);
    int32_t nx = (int32_t)hdr[0], ny = (int32_t)hdr[1], nz = (int32_t)hdr[2], mode = (int32_t)hdr[3], nsymbt = (int32_t)hdr[23];
    free(hdr);
    if (mode != 2) die("only float32 (mode 2) MRC volumes can be cut into sections or boxes", NULL);
    if (nx <= 0 || ny <= 0 || nz <= 0 || nsymbt < 0 || (nsymbt & 3)) die("implausible MRC header (nx, ny, nz, nsymbt)", NULL);
    g->data_word0 = (MRC_HEADER_BYTES + (uint64_t)nsymbt) / 4;
    g->nx = (uint32_t)nx; g->ny = (uint32_t)ny; g->nz = (uint32_t)nz;
}

/* -S bx or bx,by,bz (each 1 .. max); -N likewise */
static int parse_size(const char *s, uint32_t sz[3], unsigned long long max)
{
    for (int k = 0; k < 3; k++) {
        char *e = NULL;
        if (*s < '0' || *s > '9') return -1;
        errno = 0;
        const unsigned long long v = strtoull(s, &e, 10);
        if (errno || v == 0 || v > max) return -1;
        sz[k] = (uint32_t)v;
        if (k == 0 && *e == 0) { sz[1] = sz[2] = sz[0]; return 0; }
        if (k < 2 ? *e != ',' : *e != 0) return -1;
        s = e + 1;
    }
    return 0;
}

/* centres file: one "x y z" per line; blank lines and lines starting with '#' skipped */
static double *read_centres(const char *path, uint32_t *count)
{
    FILE *f = fopen(path, "r");
    if (!f) die("cannot open the centres file (-B)", NULL);
    size_t cap = 1024, n = 0, lineno = 0;
    double *c = (double *)malloc(cap * 3 * sizeof(double));
    char line[4096];
    if (!c) die("out of memory", NULL);
    while (fgets(line, sizeof line, f)) {
        lineno++;
        const size_t ll = strlen(line);
        if (ll == sizeof line - 1 && line[ll - 1] != '\n') die("a line of the centres file is too long", NULL);
        char *p = line;
        while (isspace((unsigned char)*p)) p++;
        if (*p == 0 || *p == '#') continue;
        if (n == cap) {
            cap *= 2;
            c = (double *)realloc(c, cap * 3 * sizeof(double));
            if (!c) die("out of memory", NULL);
        }
        for (int k = 0; k < 3; k++) {
            char *e = NULL;
            errno = 0;
            c[3 * n + k] = strtod(p, &e);
            if (e == p || errno || (*e && !isspace((unsigned char)*e))) {
                fprintf(stderr, "centres file line %zu: ", lineno);
                die("want three numbers \"x y z\" per line", NULL);
            }
            p = e;
        }
        while (isspace((unsigned char)*p)) p++;
        if (*p) {
            fprintf(stderr, "centres file line %zu: ", lineno);
            die("want three numbers \"x y z\" per line", NULL);
        }
        if (++n > 0x7fffffffu) die("too many centres", NULL);
    }
    if (ferror(f)) die("read error in the centres file", NULL);
    fclose(f);
    *count = (uint32_t)n;
    return c;
}

/* boxes of g around the n centres, decoded on the device, into a malloc'ed host buffer of n * bz * by * bx words */
static uint32_t *decode_boxes(mrcz_ctx_t *c, const struct container *ct, mrcz_box_geom_t *g, const double *centres, uint32_t n, int int_mode)
{
    const uint64_t chk = ct->chk, nch = (ct->nfl + chk - 1) / chk, words = (uint64_t)n * g->bz * g->by * g->bx;
    int32_t *org = (int32_t *)malloc(12u * (size_t)n + 12u);
    uint8_t *covered = (uint8_t *)malloc((size_t)nch);
    uint64_t *offs = (uint64_t *)malloc(8u * (size_t)(nch + 1));
    uint32_t *out = (uint32_t *)malloc(4u * (size_t)words + 4u);
    if (!org || !covered || !offs || !out) die("out of memory", NULL);
    if (mrcz_box_origins(g, centres, n, org) != MRCZ_OK) die("a centre is not a finite number or its box lies outside int32", NULL);
    if (mrcz_boxes_chunks(g, org, n, ct->nfl, ct->chk, covered) != MRCZ_OK) die("box geometry", NULL);
    uint64_t last = 0; /* chunks [0, last) hold every covered one */
    for (uint64_t k = 0; k < nch; k++)
        if (covered[k]) last = k + 1;
    uint64_t off = MRCZ_FILE_HEADER_BYTES, biggest = 0;
    for (uint64_t k = 0; k < last; k++) { /* 16 bytes per chunk up to the last covered one, nothing behind it */
        uint8_t h[16];
        uint64_t bytes = 0;
        const uint64_t left = ct->nfl - k * chk;
        offs[k] = off;
        pread_all(ct->fd, h, 16, off, "truncated container (chunk header)");
        if (mrcz_record_size(h, (uint32_t)(left < chk ? left : chk), &bytes) != MRCZ_OK) die("damaged chunk header", NULL);
        off += bytes;
    }
    offs[last] = off;
    for (uint64_t k = 0; k < last;) { /* the largest run of covered chunks sizes the record buffers */
        uint64_t e = k;
        while (e < last && covered[e]) e++;
        if (e > k && offs[e] - offs[k] > biggest) biggest = offs[e] - offs[k];
        k = e > k ? e : k + 1;
    }
    void *h_rec = NULL, *d_rec = NULL, *d_out = NULL;
    if (mrcz_dev_malloc(c, &d_out, words ? 4 * words : 16)) die("out of device memory", c);
    if (biggest && (mrcz_host_malloc(c, &h_rec, biggest) || mrcz_dev_malloc(c, &d_rec, biggest))) die("out of memory", c);
    uint64_t runs = 0;
    for (uint64_t k = 0; k < last;) { /* one read and one decode call per run of covered chunks */
        if (!covered[k]) { k++; continue; }
        uint64_t e = k, dec = 0;
        while (e < last && covered[e]) e++;
        const uint64_t len = offs[e] - offs[k];
        pread_all(ct->fd, h_rec, len, offs[k], "truncated container (payload)");
        if (mrcz_copy_h2d(c, d_rec, h_rec, len) != MRCZ_OK) die("copy to the device", c);
        if (mrcz_uncompress_boxes(c, d_rec, len, ct->nfl, ct->chk, k, e - k, g, org, n, d_out, int_mode, &dec) != MRCZ_OK) die("box decode", c);
        runs++;
        k = e;
    }
    if (!runs && mrcz_uncompress_boxes(c, NULL, 0, ct->nfl, ct->chk, 0, 0, g, org, n, d_out, int_mode, NULL) != MRCZ_OK) die("box decode", c);
    if (words && mrcz_copy_d2h(c, out, d_out, 4 * words) != MRCZ_OK) die("copy from the device", c);
    mrcz_dev_free(c, d_out);
    if (biggest) { mrcz_dev_free(c, d_rec); mrcz_host_free(c, h_rec); }
    free(org); free(covered); free(offs);
    return out;
}

/* the volume of g binned, decoded on the device, into a malloc'ed host buffer of mz * my * mx floats */
static float *decode_binned(mrcz_ctx_t *c, const struct container *ct, const mrcz_bin_geom_t *g, uint32_t batch, int int_mode)
{
    const uint64_t chk = ct->chk, nbins = (uint64_t)(g->nx / g->fx) * (g->ny / g->fy) * (g->nz / g->fz);
    uint64_t c0 = 0, c1 = 0;
    if (mrcz_bin_chunks(g, ct->nfl, ct->chk, &c0, &c1) != MRCZ_OK) die("bin geometry", NULL);
    uint64_t *offs = (uint64_t *)malloc(8u * (size_t)(c1 + 1));
    float *out = (float *)malloc(4u * (size_t)nbins);
    if (!offs || !out) die("out of memory", NULL);
    uint64_t off = MRCZ_FILE_HEADER_BYTES, biggest = 0;
    for (uint64_t k = 0; k < c1; k++) { /* 16 bytes per chunk up to the last used one, nothing behind it */
        uint8_t h[16];
        uint64_t bytes = 0;
        const uint64_t left = ct->nfl - k * chk;
        offs[k] = off;
        pread_all(ct->fd, h, 16, off, "truncated container (chunk header)");
        if (mrcz_record_size(h, (uint32_t)(left < chk ? left : chk), &bytes) != MRCZ_OK) die("damaged chunk header", NULL);
        off += bytes;
    }
    offs[c1] = off;
    for (uint64_t k = c0; k < c1; k += batch) { /* the largest piece sizes the record buffers */
        const uint64_t e = k + batch < c1 ? k + batch : c1;
        if (offs[e] - offs[k] > biggest) biggest = offs[e] - offs[k];
    }
    void *h_rec = NULL, *d_rec = NULL, *d_acc = NULL, *d_out = NULL;
    if (mrcz_dev_malloc(c, &d_acc, 8 * nbins) || mrcz_dev_malloc(c, &d_out, 4 * nbins)) die("out of device memory", c);
    if (mrcz_host_malloc(c, &h_rec, biggest) || mrcz_dev_malloc(c, &d_rec, biggest)) die("out of memory", c);
    for (uint64_t k = c0; k < c1; k += batch) { /* one read and one decode call per piece of at most `batch` chunks */
        const uint64_t e = k + batch < c1 ? k + batch : c1, len = offs[e] - offs[k];
        pread_all(ct->fd, h_rec, len, offs[k], "truncated container (payload)");
        if (mrcz_copy_h2d(c, d_rec, h_rec, len) != MRCZ_OK) die("copy to the device", c);
        if (mrcz_uncompress_binned(c, d_rec, len, ct->nfl, ct->chk, k, e - k, g, (double *)d_acc, int_mode, NULL) != MRCZ_OK) die("binned decode", c);
    }
    if (mrcz_binned_finish(c, g, (const double *)d_acc, (float *)d_out) != MRCZ_OK) die("binned finish", c);
    if (mrcz_copy_d2h(c, out, d_out, 4 * nbins) != MRCZ_OK) die("copy from the device", c);
    mrcz_dev_free(c, d_out);
    mrcz_dev_free(c, d_acc);
    mrcz_dev_free(c, d_rec);
    mrcz_host_free(c, h_rec);
    free(offs);
    return out;
}

/* the whole file with its `keep` top planes, written to fo piece by piece: 16 bytes per chunk header, then per chunk one pread of
 * the kept payloads behind a copy of the header (thinned records) in a pinned buffer of the largest piece */
static void extract_top(mrcz_ctx_t *c, const struct container *ct, int keep, int half, uint32_t batch, FILE *fo)
{
    const uint64_t chk = ct->chk, nch = (ct->nfl + chk - 1) / chk, esz = half ? 2 : 4;
    uint64_t *at = (uint64_t *)malloc(8u * (size_t)nch), *kept = (uint64_t *)malloc(8u * (size_t)nch);
    uint8_t *hdrs = (uint8_t *)malloc(16u * (size_t)nch);
    if (!at || !kept || !hdrs) die("out of memory", NULL);
    uint64_t off = MRCZ_FILE_HEADER_BYTES, biggest = 0, piece = 0;
    for (uint64_t k = 0; k < nch; k++) { /* where every record's kept tail is: at[k], kept[k] bytes */
        uint64_t skip = 0;
        const uint64_t left = ct->nfl - k * chk;
        pread_all(ct->fd, hdrs + 16 * k, 16, off, "truncated container (chunk header)");
        if (mrcz_record_top_span(hdrs + 16 * k, (uint32_t)(left < chk ? left : chk), keep, &skip, &kept[k]) != MRCZ_OK) die("damaged chunk header", NULL);
        at[k] = off + skip;
        off = at[k] + kept[k];
        piece += 16 + kept[k];
        if ((k + 1) % batch == 0 || k + 1 == nch) { if (piece > biggest) biggest = piece; piece = 0; }
    }
    const uint64_t pw = (uint64_t)batch * chk; /* words of a full piece */
    void *h_rec = NULL, *d_rec = NULL, *d_out = NULL, *h_out = NULL;
    if (mrcz_host_malloc(c, &h_rec, biggest) || mrcz_host_malloc(c, &h_out, esz * pw) || mrcz_dev_malloc(c, &d_rec, biggest) || mrcz_dev_malloc(c, &d_out, esz * pw))
        die("out of memory", c);
    for (uint64_t k = 0; k < nch; k += batch) {
        const uint64_t e = k + batch < nch ? k + batch : nch;
        const uint64_t words = (e * chk < ct->nfl ? e * chk : ct->nfl) - k * chk;
        uint64_t len = 0, consumed = 0;
        for (uint64_t j = k; j < e; j++) {
            memcpy((uint8_t *)h_rec + len, hdrs + 16 * j, 16);
            pread_all(ct->fd, (uint8_t *)h_rec + len + 16, kept[j], at[j], "truncated container (payload)");
            len += 16 + kept[j];
        }
        if (mrcz_copy_h2d(c, d_rec, h_rec, len) != MRCZ_OK) die("copy to the device", c);
        if (mrcz_uncompress_top(c, d_rec, len, ct->nfl, ct->chk, k, e - k, keep, (half ? MRCZ_TOP_U16 : MRCZ_TOP_F32) | MRCZ_TOP_THINNED, d_out, &consumed) != MRCZ_OK)
            die("top-planes decode", c);
        if (consumed != len) die("top-planes decode: the records were not walked to their end", NULL);
        if (mrcz_copy_d2h(c, h_out, d_out, esz * words) != MRCZ_OK) die("copy from the device", c);
        if (fwrite(h_out, (size_t)esz, (size_t)words, fo) != (size_t)words) die("write", NULL);
    }
    mrcz_dev_free(c, d_out);
    mrcz_dev_free(c, d_rec);
    mrcz_host_free(c, h_out);
    mrcz_host_free(c, h_rec);
    free(at); free(kept); free(hdrs);
}

int main(int argc, char *argv[])
{
    const char *in = NULL, *outp = NULL, *wspec = NULL, *zspec = NULL, *bspec = NULL, *sspec = NULL, *fspec = NULL, *nspec = NULL, *pspec = NULL, *dtype = "float";
    int opt, device = 0, half = 0, dtype_given = 0;
    if (argc < 2) { usage(argv[0]); return 255; }
    while ((opt = getopt(argc, argv, "hi:o:w:z:B:S:F:N:P:Hs:g:")) != -1) {
        switch (opt) {
        case 'i': in = optarg; break;
        case 'o': outp = optarg; break;
        case 'w': wspec = optarg; break;
        case 'z': zspec = optarg; break;
        case 'B': bspec = optarg; break;
        case 'S': sspec = optarg; break;
        case 'F': fspec = optarg; break;
        case 'N': nspec = optarg; break;
        case 'P': pspec = optarg; break;
        case 'H': half = 1; break;
        case 's': dtype = optarg; dtype_given = 1; break;
        case 'g': device = atoi(optarg); break;
        case 'h': usage(argv[0]); return 0;
        default: usage(argv[0]); return 255;
        }
    }
    if (!in || !outp || !!wspec + !!zspec + !!bspec + !!nspec + !!pspec != 1) { usage(argv[0]); die("need -i, -o and one of -w, -z, -B, -N, -P", NULL); }
    if (!bspec && (sspec || fspec)) die("-S and -F go with -B", NULL);
    if (half && !pspec) die("-H goes with -P 2", NULL);
    int keep = 0;
    if (pspec) {
        if ((pspec[0] != '2' && pspec[0] != '3') || pspec[1]) die("-P wants 2 or 3 (top byte planes kept)", NULL);
        keep = pspec[0] - '0';
        if (half && keep != 2) die("-H (16-bit words) goes with -P 2", NULL);
        if (dtype_given && strcmp(dtype, "float") != 0) die("-P reads float containers only (-s int keeps its data in plane 0)", NULL);
    }
    const int int_mode = strcmp(dtype, "int") == 0;
    if (!int_mode && strcmp(dtype, "float") != 0) die("-s must be float or int", NULL);
    uint64_t a = 0, b = 0;
    uint32_t bsize[3] = {0, 0, 0}, bin[3] = {0, 0, 0};
    float fill = 0.f;
    if (nspec) {
        if (parse_size(nspec, bin, 0xffffffffull)) die("-N wants f or fx,fy,fz (each at least 1)", NULL);
    } else if (bspec) {
        if (!sspec) die("-B needs a box size (-S bx or -S bx,by,bz)", NULL);
        if (parse_size(sspec, bsize, 65536u)) die("-S wants bx or bx,by,bz (each 1 .. 65536)", NULL);
        if (fspec) {
            char *e = NULL;
            fill = strtof(fspec, &e);
            if (e == fspec || *e) die("-F wants a number", NULL);
        }
    } else if (!pspec && parse_pair(wspec ? wspec : zspec, &a, &b)) die(wspec ? "-w wants first:count" : "-z wants z0:z1", NULL);

    struct container ct;
    ct.fd = open(in, O_RDONLY);
    if (ct.fd < 0) die("cannot open the container", NULL);
    uint8_t fh[MRCZ_FILE_HEADER_BYTES]; /* write_mrczip_header: u64 fsz, u32 chk, i8 type, i8 ztypes[4] */
    pread_all(ct.fd, fh, sizeof fh, 0, "container shorter than its 17-byte header");
    uint64_t fsz = 0;
    memcpy(&fsz, fh, 8);
    memcpy(&ct.chk, fh + 8, 4);
    memcpy(ct.ztypes, fh + 13, 4);
    ct.nfl = fsz / 4;
    if (ct.chk == 0 || ct.chk > MRCZ_CHUNK_FLOATS) die("chunk size in the file header out of range", NULL);
    for (int j = 0; j < 4; j++)
        if (ct.ztypes[j] != 0 && ct.ztypes[j] != 2 && ct.ztypes[j] != 4) die("unknown byte stream compressor type in the file header", NULL);

    mrcz_ctx_t *c = NULL;
    if (pspec) {
        if (ct.nfl == 0) die("empty container", NULL);
        const uint64_t nch = (ct.nfl + ct.chk - 1) / ct.chk;
        const uint32_t batch = (uint32_t)(nch < 16 ? nch : 16);
        if (mrcz_create(&c, device, batch) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
        if (mrcz_set_ztypes(c, ct.ztypes) != MRCZ_OK) die("byte stream compressor types", c);
        FILE *fo = fopen(outp, "wb");
        if (!fo) die("cannot open the output file", NULL);
        extract_top(c, &ct, keep, half, batch, fo);
        if (fclose(fo) != 0) die("write", NULL);
        printf("%" PRIu64 " words with their %d top byte planes (%s) written to %s\n", ct.nfl, keep, half ? "16-bit words" : "float32", outp);
        close(ct.fd);
        fflush(stdout);
        _exit(0);
    }
    if (nspec) {
        if (ct.nfl == 0) die("empty container", NULL);
        mrcz_box_geom_t v;
        mrc_volume(&c, device, &ct, &v); /* (a context of one chunk's batch for the header; the binned pieces get their own) */
        if (v.data_word0 + (uint64_t)v.nx * v.ny * v.nz > ct.nfl) die("the MRC header describes more data than the file holds", NULL);
        mrcz_bin_geom_t g;
        g.data_word0 = v.data_word0;
        g.nx = v.nx; g.ny = v.ny; g.nz = v.nz;
        g.fx = bin[0]; g.fy = bin[1]; g.fz = bin[2];
        if (g.fx > g.nx || g.fy > g.ny || g.fz > g.nz) die("-N: a bin factor is larger than the volume's dimension", NULL);
        if ((uint64_t)g.fx * g.fy * g.fz > 0x80000000ull) die("-N: a bin of more than 2^31 voxels", NULL);
        uint64_t c0 = 0, c1 = 0;
        if (mrcz_bin_chunks(&g, ct.nfl, ct.chk, &c0, &c1) != MRCZ_OK) die("bin geometry", NULL);
        const uint32_t batch = (uint32_t)(c1 - c0 < 16 ? c1 - c0 : 16);
        mrcz_destroy(c);
        if (mrcz_create(&c, device, batch) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
        if (mrcz_set_ztypes(c, ct.ztypes) != MRCZ_OK) die("byte stream compressor types", c);
        float *out = decode_binned(c, &ct, &g, batch, int_mode);
        const size_t words = (size_t)(g.nx / g.fx) * (g.ny / g.fy) * (g.nz / g.fz);
        FILE *fo = fopen(outp, "wb");
        if (!fo) die("cannot open the output file", NULL);
        if (fwrite(out, 4, words, fo) != words || fclose(fo) != 0) die("write", NULL);
        printf("%u x %u x %u volume binned by %u x %u x %u: %u x %u x %u written to %s\n", g.nx, g.ny, g.nz, g.fx, g.fy, g.fz, g.nx / g.fx,
               g.ny / g.fy, g.nz / g.fz, outp);
        free(out);
        close(ct.fd);
        fflush(stdout);
        _exit(0);
    }
    if (bspec) {
        uint32_t n = 0;
        double *centres = read_centres(bspec, &n);
        const uint64_t nch = (ct.nfl + ct.chk - 1) / ct.chk;
        if (ct.nfl == 0) die("empty container", NULL);
        if (mrcz_create(&c, device, (uint32_t)(nch < 16 ? nch : 16)) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
        mrcz_box_geom_t g;
        mrc_volume(&c, device, &ct, &g);
        if (g.data_word0 + (uint64_t)g.nx * g.ny * g.nz > ct.nfl) die("the MRC header describes more data than the file holds", NULL);
        g.bx = bsize[0]; g.by = bsize[1]; g.bz = bsize[2];
        memcpy(&g.fill_bits, &fill, 4);
        uint32_t *out = decode_boxes(c, &ct, &g, centres, n, int_mode);
        const size_t words = (size_t)n * g.bz * g.by * g.bx;
        FILE *fo = fopen(outp, "wb");
        if (!fo) die("cannot open the output file", NULL);
        if (fwrite(out, 4, words, fo) != words || fclose(fo) != 0) die("write", NULL);
        printf("%u boxes of %u x %u x %u written to %s\n", n, g.bx, g.by, g.bz, outp);
        free(out);
        free(centres);
        close(ct.fd);
        fflush(stdout);
        _exit(0);
    }
    uint64_t w0, w1;
    if (wspec) {
        w0 = a;
        w1 = a + b;
        if (b == 0 || w1 < w0 || w1 > ct.nfl) die("-w window empty or past the end of the file", NULL);
    } else {
        mrcz_box_geom_t g;
        mrc_volume(&c, device, &ct, &g);
        if (a >= b || b > (uint64_t)g.nz) die("-z sections outside the volume", NULL);
        const uint64_t sec = (uint64_t)g.nx * (uint64_t)g.ny;
        w0 = g.data_word0 + a * sec;
        w1 = w0 + (b - a) * sec;
        if (w1 > ct.nfl) die("the MRC header describes more data than the file holds", NULL);
    }
    uint32_t *out = decode_window(&c, device, &ct, w0, w1, int_mode);
    FILE *fo = fopen(outp, "wb");
    if (!fo) die("cannot open the output file", NULL);
    if (fwrite(out, 4, (size_t)(w1 - w0), fo) != (size_t)(w1 - w0) || fclose(fo) != 0) die("write", NULL);
    printf("words [%" PRIu64 ", %" PRIu64 ") of %" PRIu64 " written to %s\n", w0, w1, ct.nfl, outp);
    free(out);
    close(ct.fd);
    fflush(stdout);
    _exit(0); /* (as mrc_tar: the process's death releases the device memory; skipping the runtime's teardown saves 0.1 s) */
}
