/*
 * mrc_verify.c -- compare decode from the command line: is the original reproduced by its container, and how well?
 *
 *   mrc_verify -a vol.mrc -z vol.mrc.zip [-e eps] [-r rel] [-s float|int] [-c] [-g device]
 *
 *   -a   the original file
 *   -z   the container written from it by mrc_tar -t zip
 *   -e   absolute bound: the verdict fails if a finite point has |decoded - original| > eps (mrc_tar -e promises <= eps)
 *   -r   relative bound: the verdict fails if a finite point with |original| > 1e-3 has |decoded - original| / |original| > rel
 *   -s   decode mode, as mrc_tar -s (the container does not record it)
 *   -c   one line per chunk as well: "chunk c max_err rmse n_diff", the error profile along the file
 *
 * Digest decode, the fixity check that needs no original (the CRC-32, zlib's, of what the container decodes to):
 *
 *   mrc_verify -z vol.mrc.zip -k [-s float|int]           prints the container's digest sidecar (sidecar.h) to stdout
 *   mrc_verify -a vol.mrc -k                              the same for a plain file: its "file" line is what crc32 vol.mrc prints
 *                                                         when the size is a multiple of four
 *   mrc_verify -z vol.mrc.zip -K vol.mrc.zip.crc          checks the container against a sidecar: "chunk <c> expected <hex> got <hex>"
 *                                                         for every chunk that differs, then "file expected <hex> got <hex>"; exit
 *                                                         status 0 when all match, 1 when any differs.  The mode is the sidecar's
 *                                                         unless -s is given.  A sidecar of other words, chunk size or chunks than
 *                                                         the container's header names is refused (255).
 *   -k / -K exclude -e and -r; nothing is written.
 *
 * Probe, the question before the first container exists (which -b or -e for this volume?):
 *
 *   mrc_verify -a vol.mrc -p SPEC                         SPEC = a comma list of bN, bLO:HI (inclusive; b alone = b0:32), eEPS and
 *                                                         int.  The file streams through the device once, in the runs -a is read
 *                                                         in; every setting is probed on each resident run (mrcz_probe_chunks:
 *                                                         nothing is written or decoded).  One line per setting, in the order given:
 *                                                         "probe <b N | e EPS | int> bytes <container bytes> ratio <file bytes /
 *                                                         container bytes> max_err <..> rmse <..> psnr_db <..> special_diff <n>".
 *                                                         Exit status 0; 255 for a bad SPEC or an unreadable file.
 *   -p excludes -z and everything that goes with a container.
 *
 * The container is decoded on the device in runs of the context's batch (16 chunks); the original passes through a pinned buffer
 * in the same runs, one mrcz_uncompress_compare per run, one mrcz_compare_finish.  The decoded words are never written anywhere.
 * Prints one "key value" line per field of mrcz_compare_t (include/mrcz_hip.h) and the derived mean_err = sum_err / n_finite,
 * rmse = sqrt(sum_err2 / n_finite), psnr_db = 20 log10((orig_max - orig_min) / rmse).
 * Exit status: 0 when no header word differs and, if a bound was given, no point exceeds it and no NaN / Inf word differs; 1 when
 * that verdict fails; 255 for bad arguments, unreadable files and malformed containers.
 */
#include "../../include/mrcz_hip.h"
#include "sidecar.h"

#include <errno.h>
#include <fcntl.h>
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#define BATCH 16u

static void usage(const char *prog)
{
    printf("\nUsage:\n\n\t%s -a <original> -z <container> [-e <eps>] [-r <rel>] [-s float|int] [-c] [-g device]\nwhere:\n", prog);
    printf("\t-a\tthe original file\n\n");
    printf("\t-z\tcontainer written from it by mrc_tar -t zip\n\n");
    printf("\t-e\tabsolute error bound of the verdict\n\n");
    printf("\t-r\trelative error bound of the verdict\n\n");
    printf("\t-s\tdata type the container was written with, [float | int], default float\n\n");
    printf("\t-c\tprint the error of every chunk as well\n\n");
    printf("\t-g\tHIP device, default 0\n\n");
    printf("\t-k\tprint the digest sidecar (CRC-32 of the decode) of the container -z, or of the plain file -a when no -z is given\n\n");
    printf("\t-K\tcheck the container -z against this sidecar: exit status 0 all chunks match, 1 some differ\n\n");
    printf("\t-p\tprobe the plain file -a (no -z): size and error of every setting of the comma list, e.g. b0:12,e0.01,int\n");
    printf("\t\t(bN, bLO:HI, b = b0:32, eEPS, int), one line each: probe <setting> bytes .. ratio .. max_err .. rmse .. psnr_db .. special_diff ..\n\n");
}

/* errors leave with the reference's exit(-1) status (255), never through a signal (as mrc_extract) */
static void die(const char *what, mrcz_ctx_t *c)
{
    fprintf(stderr, "[%s:%d] ERROR: %s%s%s\n", __FILE__, __LINE__, what, c ? ": " : "", c ? mrcz_last_error(c) : "");
    fflush(stdout);
    fflush(stderr);
    _exit(255);
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

static double parse_bound(const char *s, const char *what)
{
    char *e = NULL;
    errno = 0;
    const double v = strtod(s, &e);
    if (e == s || *e || errno || !(v >= 0.0) || isinf(v)) die(what, NULL);
    return v;
}

static void print_index(const char *key, uint64_t v)
{
    if (v == UINT64_MAX) printf("%s none\n", key);
    else printf("%s %" PRIu64 "\n", key, v);
}

static double rmse_of(const mrcz_compare_t *t) { return t->n_finite ? sqrt(t->sum_err2 / (double)t->n_finite) : 0.0; }

/* ---- digest decode: -k / -K ---- */

/* the 17-byte file header of an open container (write_mrczip_header: u64 fsz, u32 chk, i8 type, i8 ztypes[4]) */
static void container_header(int fz, uint64_t *fsz, uint32_t *chk32, signed char ztypes[4])
{
    uint8_t fh[MRCZ_FILE_HEADER_BYTES];
    pread_all(fz, fh, sizeof fh, 0, "container shorter than its 17-byte header");
    memcpy(fsz, fh, 8);
    memcpy(chk32, fh + 8, 4);
    memcpy(ztypes, fh + 13, 4);
    if (*chk32 == 0 || *chk32 > MRCZ_CHUNK_FLOATS) die("chunk size in the file header out of range", NULL);
    for (int j = 0; j < 4; j++)
        if (ztypes[j] != 0 && ztypes[j] != 2 && ztypes[j] != 4) die("unknown byte stream compressor type in the file header", NULL);
}

/* record offsets offs[0 .. nch] from the 16-byte chunk headers */
static uint64_t *record_offsets(int fz, uint64_t nfl, uint64_t chk, uint64_t nch)
{
    uint64_t *offs = (uint64_t *)malloc(8u * (size_t)(nch + 1));
    if (!offs) die("out of memory", NULL);
    uint64_t off = MRCZ_FILE_HEADER_BYTES;
    for (uint64_t k = 0; k < nch; k++) {
        uint8_t h[16];
        uint64_t bytes = 0;
        const uint64_t left = nfl - k * chk;
        offs[k] = off;
        pread_all(fz, h, 16, off, "truncated container (chunk header)");
        if (mrcz_record_size(h, (uint32_t)(left < chk ? left : chk), &bytes) != MRCZ_OK) die("damaged chunk header", NULL);
        off += bytes;
    }
    offs[nch] = off;
    return offs;
}

/* -k: print the sidecar of the container `zip`, or of the plain file `orig` when zip == NULL; -K: check `zip` against `check` */
static int digest_main(const char *orig, const char *zip, const char *check, const char *dtype, int device)
{
    sidecar_t sc;
    memset(&sc, 0, sizeof sc);
    if (check) {
        const char *why = NULL;
        if (sidecar_read(check, &sc, &why) != 0) die(why, NULL);
    }
    int int_mode = check ? sc.int_mode : 0;
    if (dtype) {
        int_mode = strcmp(dtype, "int") == 0;
        if (!int_mode && strcmp(dtype, "float") != 0) die("-s must be float or int", NULL);
    }
    const int fd = open(zip ? zip : orig, O_RDONLY);
    if (fd < 0) die(zip ? "cannot open the container" : "cannot open the file", NULL);
    uint64_t fsz = 0, *offs = NULL, biggest = 0;
    uint32_t chk32 = MRCZ_CHUNK_FLOATS;
    signed char ztypes[4] = {0, 0, 0, 0};
    if (zip) container_header(fd, &fsz, &chk32, ztypes);
    else {
        struct stat st;
        if (fstat(fd, &st) != 0) die("cannot stat the file", NULL);
        fsz = (uint64_t)st.st_size;
    }
    const uint64_t nfl = fsz / 4, chk = chk32, nch = (nfl + chk - 1) / chk;
    if (check && (sc.words != nfl || sc.chunk != chk32 || sc.chunks != nch)) die("the sidecar is of another file: words, chunk or chunks differ from the container's header", NULL);
    const uint32_t batch = (uint32_t)(nch < BATCH ? (nch ? nch : 1u) : BATCH);
    if (zip) {
        offs = record_offsets(fd, nfl, chk, nch);
        for (uint64_t k = 0; k < nch; k += batch) {
            const uint64_t e = k + batch < nch ? k + batch : nch;
            if (offs[e] - offs[k] > biggest) biggest = offs[e] - offs[k];
        }
    } else
        biggest = 4 * chk * batch;

    mrcz_ctx_t *c = NULL;
    if (mrcz_create(&c, device, batch) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
    if (mrcz_set_ztypes(c, ztypes) != MRCZ_OK) die("byte stream compressor types", c);
    mrcz_digest_t total, *chunks = (mrcz_digest_t *)malloc(sizeof(mrcz_digest_t) * (size_t)(nch ? nch : 1));
    uint32_t *crcs = (uint32_t *)malloc(4u * (size_t)(nch ? nch : 1));
    void *h_in = NULL, *d_in = NULL, *d_acc = NULL;
    if (!chunks || !crcs || mrcz_dev_malloc(c, &d_acc, sizeof(mrcz_digest_t) * (nch ? nch : 1))) die("out of memory", c);
    if (nch && (mrcz_host_malloc(c, &h_in, biggest) || mrcz_dev_malloc(c, &d_in, biggest))) die("out of memory", c);
    for (uint64_t k = 0; k < nch; k += batch) { /* one read and one digest call per run of at most `batch` chunks */
        const uint64_t e = k + batch < nch ? k + batch : nch;
        if (zip) {
            const uint64_t len = offs[e] - offs[k];
            pread_all(fd, h_in, len, offs[k], "truncated container (payload)");
            if (mrcz_copy_h2d(c, d_in, h_in, len) != MRCZ_OK) die("copy to the device", c);
            if (mrcz_uncompress_digest(c, d_in, len, nfl, chk32, k, e - k, int_mode, (mrcz_digest_t *)d_acc) != MRCZ_OK) die("digest decode", c);
        } else {
            const uint64_t w0 = k * chk, w1 = e * chk < nfl ? e * chk : nfl;
            pread_all(fd, h_in, 4 * (w1 - w0), 4 * w0, "read of the file");
            if (mrcz_copy_h2d(c, d_in, h_in, 4 * (w1 - w0)) != MRCZ_OK) die("copy to the device", c);
            if (mrcz_digest_words(c, d_in, w1 - w0, k, chk32, MRCZ_DIGEST_NONE, 0, 0.0f, (mrcz_digest_t *)d_acc) != MRCZ_OK) die("digest", c);
        }
    }
    if (mrcz_digest_finish(c, (const mrcz_digest_t *)d_acc, 0, nch, &total) != MRCZ_OK) die("digest finish", c);
    if (nch && mrcz_copy_d2h(c, chunks, d_acc, sizeof(mrcz_digest_t) * nch) != MRCZ_OK) die("copy from the device", c);
    for (uint64_t k = 0; k < nch; k++) crcs[k] = chunks[k].crc32;
    int ok = 1;
    if (!check) {
        if (sidecar_write(stdout, nfl, chk32, nch, int_mode, total.crc32, crcs) != 0) die("write to stdout", NULL);
    } else {
        for (uint64_t k = 0; k < nch; k++)
            if (crcs[k] != sc.crcs[k]) { ok = 0; printf("chunk %" PRIu64 " expected %08" PRIx32 " got %08" PRIx32 "\n", k, sc.crcs[k], crcs[k]); }
        if (total.crc32 != sc.file) ok = 0;
        printf("file expected %08" PRIx32 " got %08" PRIx32 "\n", sc.file, total.crc32);
    }
    close(fd);
    fflush(stdout);
    _exit(ok ? 0 : 1);
}

/* ---- probe: -p ---- */

typedef struct {
    int xform, bits;
    float eps;
    char label[48]; /* "b N", "e EPS" (as given) or "int" */
} probe_setting_t;

/* the bound as mrc_tar -e takes it: float32 toward zero, finite and > 0 */
static float probe_eps(const char *s, size_t n)
{
    char buf[40], *e = NULL;
    if (n == 0 || n >= sizeof buf) die("-p: eEPS wants a finite number > 0", NULL);
    memcpy(buf, s, n);
    buf[n] = 0;
    errno = 0;
    const double v = strtod(buf, &e);
    if (e == buf || *e || !(v > 0.0) || isinf(v)) die("-p: eEPS wants a finite number > 0", NULL);
    float f = v > 3.4028234663852886e38 ? 3.4028234663852886e38f : (float)v;
    if ((double)f > v) { /* rounded up: one step toward zero, so that the bound holds for the value given */
        uint32_t u;
        memcpy(&u, &f, 4);
        u--;
        memcpy(&f, &u, 4);
    }
    if (!(f > 0.0f)) die("-p: eEPS is below the smallest float32", NULL);
    return f;
}

/* digits [s, s + n) as a mask level 0..32 */
static int probe_bits(const char *s, size_t n)
{
    if (n == 0 || n > 2) die("-p: bN wants a mask level 0..32", NULL);
    int v = 0;
    for (size_t i = 0; i < n; i++) {
        if (s[i] < '0' || s[i] > '9') die("-p: bN wants a mask level 0..32", NULL);
        v = 10 * v + (s[i] - '0');
    }
    if (v > 32) die("-p: bN wants a mask level 0..32", NULL);
    return v;
}

static probe_setting_t *parse_probe_spec(const char *spec, size_t *count)
{
    size_t n = 0, cap = 64;
    probe_setting_t *st = (probe_setting_t *)malloc(cap * sizeof *st);
    if (!st) die("out of memory", NULL);
    for (const char *p = spec;;) {
        const char *q = strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : strlen(p);
        int lo = -1, hi = -1;
        probe_setting_t one;
        memset(&one, 0, sizeof one);
        if (len == 3 && memcmp(p, "int", 3) == 0) {
            one.xform = MRCZ_PROBE_INT8;
            strcpy(one.label, "int");
        } else if (len >= 1 && p[0] == 'e') {
            one.xform = MRCZ_PROBE_ABS;
            one.eps = probe_eps(p + 1, len - 1);
            snprintf(one.label, sizeof one.label, "e %.*s", (int)(len - 1), p + 1);
        } else if (len >= 1 && p[0] == 'b') {
            const char *colon = (const char *)memchr(p, ':', len);
            if (len == 1) { lo = 0; hi = 32; }
            else if (colon) { lo = probe_bits(p + 1, (size_t)(colon - p - 1)); hi = probe_bits(colon + 1, len - (size_t)(colon - p) - 1); }
            else lo = hi = probe_bits(p + 1, len - 1);
            if (lo > hi) die("-p: bLO:HI wants LO <= HI", NULL);
        } else
            die("-p: a setting is bN, bLO:HI, b, eEPS or int", NULL);
        const int reps = lo < 0 ? 1 : hi - lo + 1; /* a range of mask levels is one setting per level */
        for (int r = 0; r < reps; r++) {
            if (n == cap) {
                cap *= 2;
                st = (probe_setting_t *)realloc(st, cap * sizeof *st);
                if (!st) die("out of memory", NULL);
            }
            if (lo >= 0) {
                one.xform = MRCZ_PROBE_MASK;
                one.bits = lo + r;
                snprintf(one.label, sizeof one.label, "b %d", lo + r);
            }
            st[n++] = one;
        }
        if (n > 4096) die("-p: too many settings", NULL);
        if (!q) break;
        p = q + 1;
    }
    *count = n;
    return st;
}

static int probe_main(const char *orig, const char *spec, int device)
{
    size_t nset = 0;
    probe_setting_t *st = parse_probe_spec(spec, &nset);
    const int fd = open(orig, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) die("cannot open the file", NULL);
    const uint64_t fsz = (uint64_t)sb.st_size, nfl = fsz / 4, chk = MRCZ_CHUNK_FLOATS, nch = (nfl + chk - 1) / chk;
    const uint32_t batch = (uint32_t)(nch < BATCH ? (nch ? nch : 1u) : BATCH);
    mrcz_ctx_t *c = NULL;
    if (mrcz_create(&c, device, batch) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
    const uint64_t run_bytes = 4 * chk * batch, acc_bytes = sizeof(mrcz_compare_t) * (nch ? nch : 1);
    uint64_t *size = (uint64_t *)calloc(nset, sizeof *size);
    void *h_in = NULL, *d_in = NULL, *d_acc = NULL; /* d_acc: one run of nch records per setting */
    if (!size || mrcz_dev_malloc(c, &d_acc, acc_bytes * nset)) die("out of memory", c);
    if (nch && (mrcz_host_malloc(c, &h_in, run_bytes) || mrcz_dev_malloc(c, &d_in, run_bytes))) die("out of memory", c);
    for (uint64_t k = 0; k < nch; k += batch) { /* one read and one upload per run of at most `batch` chunks, every setting probed on it */
        const uint64_t e = k + batch < nch ? k + batch : nch;
        const uint64_t w0 = k * chk, w1 = e * chk < nfl ? e * chk : nfl;
        pread_all(fd, h_in, 4 * (w1 - w0), 4 * w0, "read of the file");
        if (mrcz_copy_h2d(c, d_in, h_in, 4 * (w1 - w0)) != MRCZ_OK) die("copy to the device", c);
        for (size_t s = 0; s < nset; s++) {
            uint64_t len = 0;
            if (mrcz_probe_chunks(c, d_in, w1 - w0, k, st[s].xform, st[s].bits, st[s].eps, -1.0, -1.0,
                                  (mrcz_compare_t *)((uint8_t *)d_acc + acc_bytes * s), &len, NULL) != MRCZ_OK)
                die("probe", c);
            size[s] += len;
        }
    }
    for (size_t s = 0; s < nset; s++) {
        mrcz_compare_t t;
        if (mrcz_compare_finish(c, (const mrcz_compare_t *)((uint8_t *)d_acc + acc_bytes * s), 0, nch, &t) != MRCZ_OK) die("compare finish", c);
        const uint64_t bytes = nfl ? MRCZ_FILE_HEADER_BYTES + size[s] : 0; /* mrc_tar writes nothing for a file of fewer than four bytes */
        const double rmse = rmse_of(&t);
        printf("probe %s bytes %" PRIu64 " ratio %.17g max_err %.17g rmse %.17g psnr_db ", st[s].label, bytes, bytes ? (double)fsz / (double)bytes : 0.0,
               t.max_err, rmse);
        if (rmse == 0.0) printf("inf");
        else printf("%.17g", 20.0 * log10((t.orig_max - t.orig_min) / rmse));
        printf(" special_diff %" PRIu64 "\n", t.n_special_diff);
    }
    close(fd);
    fflush(stdout);
    _exit(0);
}

int main(int argc, char *argv[])
{
    const char *orig = NULL, *zip = NULL, *dtype = NULL, *check = NULL, *probe = NULL;
    double eps_abs = -1.0, eps_rel = -1.0;
    int opt, device = 0, per_chunk = 0, print_digest = 0;
    if (argc < 2) { usage(argv[0]); return 255; }
    while ((opt = getopt(argc, argv, "ha:z:e:r:s:cg:kK:p:")) != -1) {
        switch (opt) {
        case 'a': orig = optarg; break;
        case 'z': zip = optarg; break;
        case 'e': eps_abs = parse_bound(optarg, "-e wants a finite number >= 0"); break;
        case 'r': eps_rel = parse_bound(optarg, "-r wants a finite number >= 0"); break;
        case 's': dtype = optarg; break;
        case 'c': per_chunk = 1; break;
        case 'g': device = atoi(optarg); break;
        case 'k': print_digest = 1; break;
        case 'K': check = optarg; break;
        case 'p': probe = optarg; break;
        case 'h': usage(argv[0]); return 0;
        default: usage(argv[0]); return 255;
        }
    }
    if (probe) {
        if (zip || check || print_digest || dtype || per_chunk || eps_abs >= 0.0 || eps_rel >= 0.0) die("-p probes a plain file: give -a and none of -z, -k, -K, -s, -c, -e, -r", NULL);
        if (!orig) die("-p wants the file to probe (-a)", NULL);
        return probe_main(orig, probe, device);
    }
    if (print_digest || check) {
        if (eps_abs >= 0.0 || eps_rel >= 0.0 || per_chunk) die("-k and -K exclude -e, -r and -c", NULL);
        if (print_digest && check) die("-k prints a sidecar, -K checks one: give one of them", NULL);
        if (check && (!zip || orig)) die("-K checks a container: give -z and no -a", NULL);
        if (print_digest && !zip == !orig) die("-k wants a container (-z) or a plain file (-a), not both", NULL);
        return digest_main(orig, zip, check, dtype, device);
    }
    if (!orig || !zip) { usage(argv[0]); die("need -a and -z", NULL); }
    if (!dtype) dtype = "float";
    const int int_mode = strcmp(dtype, "int") == 0;
    if (!int_mode && strcmp(dtype, "float") != 0) die("-s must be float or int", NULL);

    const int fz = open(zip, O_RDONLY);
    if (fz < 0) die("cannot open the container", NULL);
    uint8_t fh[MRCZ_FILE_HEADER_BYTES]; /* write_mrczip_header: u64 fsz, u32 chk, i8 type, i8 ztypes[4] */
    pread_all(fz, fh, sizeof fh, 0, "container shorter than its 17-byte header");
    uint64_t fsz = 0;
    uint32_t chk32 = 0;
    signed char ztypes[4];
    memcpy(&fsz, fh, 8);
    memcpy(&chk32, fh + 8, 4);
    memcpy(ztypes, fh + 13, 4);
    if (chk32 == 0 || chk32 > MRCZ_CHUNK_FLOATS) die("chunk size in the file header out of range", NULL);
    for (int j = 0; j < 4; j++)
        if (ztypes[j] != 0 && ztypes[j] != 2 && ztypes[j] != 4) die("unknown byte stream compressor type in the file header", NULL);
    const int fa = open(orig, O_RDONLY);
    struct stat st;
    if (fa < 0 || fstat(fa, &st) != 0) die("cannot open the original", NULL);
    if ((uint64_t)st.st_size != fsz) die("the original's size is not the size the container records", NULL);
    const uint64_t nfl = fsz / 4, chk = chk32, nch = (nfl + chk - 1) / chk;

    /* record offsets from the 16-byte chunk headers */
    uint64_t *offs = (uint64_t *)malloc(8u * (size_t)(nch + 1));
    if (!offs) die("out of memory", NULL);
    uint64_t off = MRCZ_FILE_HEADER_BYTES, biggest = 0;
    for (uint64_t k = 0; k < nch; k++) {
        uint8_t h[16];
        uint64_t bytes = 0;
        const uint64_t left = nfl - k * chk;
        offs[k] = off;
        pread_all(fz, h, 16, off, "truncated container (chunk header)");
        if (mrcz_record_size(h, (uint32_t)(left < chk ? left : chk), &bytes) != MRCZ_OK) die("damaged chunk header", NULL);
        off += bytes;
    }
    offs[nch] = off;
    const uint32_t batch = (uint32_t)(nch < BATCH ? (nch ? nch : 1u) : BATCH);
    for (uint64_t k = 0; k < nch; k += batch) { /* the largest run sizes the record buffers */
        const uint64_t e = k + batch < nch ? k + batch : nch;
        if (offs[e] - offs[k] > biggest) biggest = offs[e] - offs[k];
    }

    mrcz_ctx_t *c = NULL;
    if (mrcz_create(&c, device, batch) != MRCZ_OK) die("no usable HIP device (the codec has no CPU path)", NULL);
    if (mrcz_set_ztypes(c, ztypes) != MRCZ_OK) die("byte stream compressor types", c);
    mrcz_compare_t total, *chunks = (mrcz_compare_t *)malloc(sizeof(mrcz_compare_t) * (size_t)(nch ? nch : 1));
    void *h_rec = NULL, *d_rec = NULL, *h_org = NULL, *d_org = NULL, *d_acc = NULL;
    const uint64_t run_bytes = 4 * chk * batch;
    if (!chunks || mrcz_dev_malloc(c, &d_acc, sizeof(mrcz_compare_t) * (nch ? nch : 1))) die("out of memory", c);
    if (nch && (mrcz_host_malloc(c, &h_rec, biggest) || mrcz_dev_malloc(c, &d_rec, biggest) || mrcz_host_malloc(c, &h_org, run_bytes) ||
                mrcz_dev_malloc(c, &d_org, run_bytes)))
        die("out of memory", c);
    for (uint64_t k = 0; k < nch; k += batch) { /* one read of each file and one compare call per run of at most `batch` chunks */
        const uint64_t e = k + batch < nch ? k + batch : nch, len = offs[e] - offs[k];
        const uint64_t w0 = k * chk, w1 = e * chk < nfl ? e * chk : nfl;
        pread_all(fz, h_rec, len, offs[k], "truncated container (payload)");
        pread_all(fa, h_org, 4 * (w1 - w0), 4 * w0, "read of the original");
        if (mrcz_copy_h2d(c, d_rec, h_rec, len) != MRCZ_OK || mrcz_copy_h2d(c, d_org, h_org, 4 * (w1 - w0)) != MRCZ_OK) die("copy to the device", c);
        if (mrcz_uncompress_compare(c, d_rec, len, nfl, chk32, k, e - k, d_org, eps_abs, eps_rel, int_mode, (mrcz_compare_t *)d_acc) != MRCZ_OK)
            die("compare decode", c);
    }
    if (mrcz_compare_finish(c, (const mrcz_compare_t *)d_acc, 0, nch, &total) != MRCZ_OK) die("compare finish", c);
    if (per_chunk && nch && mrcz_copy_d2h(c, chunks, d_acc, sizeof(mrcz_compare_t) * nch) != MRCZ_OK) die("copy from the device", c);

    const double rmse = rmse_of(&total);
    printf("n %" PRIu64 "\n", total.n);
    printf("n_header_diff %" PRIu64 "\n", total.n_header_diff);
    printf("n_diff %" PRIu64 "\n", total.n_diff);
    printf("n_finite %" PRIu64 "\n", total.n_finite);
    printf("n_special_diff %" PRIu64 "\n", total.n_special_diff);
    printf("n_over_abs %" PRIu64 "\n", total.n_over_abs);
    printf("n_over_rel %" PRIu64 "\n", total.n_over_rel);
    print_index("first_over", total.first_over);
    print_index("max_err_index", total.max_err_index);
    print_index("max_rel_index", total.max_rel_index);
    printf("max_err %.17g\nmax_rel %.17g\n", total.max_err, total.max_rel);
    printf("sum_err %.17g\nsum_abs_err %.17g\nsum_err2 %.17g\n", total.sum_err, total.sum_abs_err, total.sum_err2);
    printf("orig_min %.17g\norig_max %.17g\norig_sum %.17g\norig_sum2 %.17g\n", total.orig_min, total.orig_max, total.orig_sum, total.orig_sum2);
    printf("mean_err %.17g\n", total.n_finite ? total.sum_err / (double)total.n_finite : 0.0);
    printf("rmse %.17g\n", rmse);
    if (rmse == 0.0) printf("psnr_db inf\n");
    else printf("psnr_db %.17g\n", 20.0 * log10((total.orig_max - total.orig_min) / rmse));
    if (per_chunk)
        for (uint64_t k = 0; k < nch; k++) printf("chunk %" PRIu64 " %.17g %.17g %" PRIu64 "\n", k, chunks[k].max_err, rmse_of(&chunks[k]), chunks[k].n_diff);
    const int bounded = eps_abs >= 0.0 || eps_rel >= 0.0;
    const int ok = total.n_header_diff == 0 && (!bounded || (total.n_over_abs == 0 && total.n_over_rel == 0 && total.n_special_diff == 0));
    if (!ok) {
        if (total.n_header_diff) printf("FAILED: %" PRIu64 " header words differ\n", total.n_header_diff);
        if (bounded && total.first_over != UINT64_MAX) printf("FAILED: first word outside the bound: %" PRIu64 "\n", total.first_over);
    }
    close(fa);
    close(fz);
    fflush(stdout);
    _exit(ok ? 0 : 1); /* (as mrc_extract: the process's death releases the device memory) */
}
