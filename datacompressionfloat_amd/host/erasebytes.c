/*
 * erasebytes.c -- the reference's verification tool (/root/reference/src/tool/erasebytes.c:36-147: copy the
 * 1024-byte header, zero the low `b` bits of every later 32-bit word) with the masking done on the MI355X through
 * mrcz_erase_bits (include/mrcz_hip.h).  Same command line (-i, -o, -b, -h), same output bytes: a decoded file is
 * compared with this tool's output in the reference's round-trip test (run_full_test.sh:84-102).  Trailing
 * bytes that do not fill a 32-bit word are dropped, as the reference's fread(…, sizeof(float), …) does.  One
 * divergence: for a file shorter than 1024 bytes the reference writes 1024 bytes of its (uninitialised) buffer
 * (erasebytes.c:105-107); this tool writes the bytes it read.  Extension: -e <eps> writes what a container of
 * `mrc_tar -e <eps>` decodes to (mrcz_erase_abs) instead of masking.
 */
#include "../../include/mrcz_hip.h"

#include <float.h>
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the bound as mrcz_workers_set_abs_error takes it: float32 toward zero (0 for anything it refuses) */
static float abs_bound(double eps)
{
    if (!(eps > 0.0) || !isfinite(eps)) return 0.0f;
    float f = eps > FLT_MAX ? FLT_MAX : (float)eps;
    if ((double)f > eps) {
        uint32_t u;
        memcpy(&u, &f, 4);
        u--;
        memcpy(&f, &u, 4);
    }
    return f;
}

static void usage(char **argv)
{
    printf("\nUsage:\n\n\t%s -i <input file> -o <output file> [-b <bits to erase>]\nwhere:\n", argv[0]);
    printf("\t-i\tinput file that need to erase lowest byte\n\n");
    printf("\t-o\t output file that save the float number with lowerest byte to be \\0\n\n");
    printf("\t-b\t bits to be erased, default is 8\n\n");
    printf("\t-e\t absolute error bound instead of -b: the words a container of mrc_tar -e <eps> decodes to (extension of the MI355X build)\n\n");
}

int main(int argc, char *argv[])
{
    const char *in = NULL, *out = NULL;
    const char *eps_arg = NULL;
    int bits = 8, bits_given = 0, opt;
    float eps = 0.0f;
    if (argc < 2) { usage(argv); exit(-1); }
    while ((opt = getopt(argc, argv, "hi:o:b:e:")) != -1) {
        switch (opt) {
        case 'i': in = optarg; break;
        case 'o': out = optarg; break;
        case 'b': bits = atoi(optarg); bits_given = 1; break;
        case 'e': eps_arg = optarg; break;
        case 'h': usage(argv); return 0;
        default: printf("Invalid command line parameters!\n"); usage(argv); return -1;
        }
    }
    if (!in || !out) { usage(argv); return -1; }
    if (bits < 0 || bits > 32) { /* the reference indexes a 33-entry table without a check (erasebytes.c:27-33,125) */
        fprintf(stderr, "[%s:%d] bits to erase must be in 0..32\n", __FILE__, __LINE__);
        exit(-1);
    }
    if (eps_arg) {
        char *end;
        const double e = strtod(eps_arg, &end);
        eps = (end == eps_arg || *end) ? 0.0f : abs_bound(e);
        if (!(eps > 0.0f) || bits_given) {
            fprintf(stderr, "[%s:%d] -e needs a finite bound > 0 and excludes -b\n", __FILE__, __LINE__);
            exit(-1);
        }
        printf("Input File = %s, Output File = %s, absErrorBound = %.9g\n", in, out, (double)eps);
    } else {
        printf("Input File = %s, Output File = %s, bitsToErase = %d\n", in, out, bits);
    }
    FILE *fi = fopen(in, "rb"), *fo = fopen(out, "wb");
    if (!fi) { fprintf(stderr, "[%s:%d] open file [%s] failed\n", __FILE__, __LINE__, in); exit(-1); }
    if (!fo) { fprintf(stderr, "[%s:%d] open file [%s] failed\n", __FILE__, __LINE__, out); exit(-1); }
    mrcz_ctx_t *c = NULL;
    if (mrcz_create(&c, 0, 1) != MRCZ_OK) { fprintf(stderr, "[%s:%d] no usable HIP device (this tool has no CPU path)\n", __FILE__, __LINE__); exit(-1); }
    const uint64_t ITEMS = 1024ull * 1024 * 32; /* 128 MiB of words per round trip */
    void *h = NULL, *d = NULL;
    if (mrcz_host_malloc(c, &h, ITEMS * 4) || mrcz_dev_malloc(c, &d, ITEMS * 4)) { fprintf(stderr, "alloc failed: %s\n", mrcz_last_error(c)); exit(-1); }
    /* the header travels as bytes (erasebytes.c:105-107): a file shorter than 1024 bytes is copied whole */
    size_t nh = fread(h, 1, 1024, fi);
    fwrite(h, 1, nh, fo);
    uint64_t word0 = 256; /* index, inside the file, of the first word of the next block */
    size_t num;
    while ((num = fread(h, 4, (size_t)ITEMS, fi)) > 0) {
        if (mrcz_copy_h2d(c, d, h, (uint64_t)num * 4) ||
            (eps_arg ? mrcz_erase_abs(c, d, (uint64_t)num, word0, eps) : mrcz_erase_bits(c, d, (uint64_t)num, word0, bits)) ||
            mrcz_copy_d2h(c, h, d, (uint64_t)num * 4)) {
            fprintf(stderr, "[%s:%d] GPU step failed: %s\n", __FILE__, __LINE__, mrcz_last_error(c));
            exit(-1);
        }
        fwrite(h, 4, num, fo);
        word0 += num;
    }
    mrcz_host_free(c, h);
    mrcz_dev_free(c, d);
    mrcz_destroy(c);
    fclose(fi);
    fclose(fo);
    return EXIT_SUCCESS;
}
