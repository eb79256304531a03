/*
 * mrc_tar.c -- single-file front-end with the reference's command line
 * (/root/reference/src/main/mrc_tar.c:82-165): mrc_tar -i <in> -o <out> [-t zip|unzip] [-b 0..32]
 * [-s float|int] [-h].  The work is done by run_compress / run_uncompress on the GPU.  Extension: -e <eps>, the
 * absolute-error mode of the compressor (mrcz_workers_set_abs_error); unzip needs nothing for it.  Extension: -k (zip) also
 * writes <output>.crc, the digest sidecar (sidecar.h) of what the container will decode to under the mode in force; -K <sidecar>
 * (unzip) digests what is decoded, writes the output as always, and ends with status 1 and the differing chunks named when the
 * digest disagrees with the sidecar (mrcz_workers_set_digest).
 */
#include "../../include/mrcz_hip.h"
#include "../../include/mrcz_workers.h"
#include "sidecar.h"

#include <stdlib.h>
#include <string.h>
#include <unistd.h>

static void usage(char **argv) /* mrc_tar.c:82-100 */
{
    printf("\nUsage:\n\n\t%s -i <input file> -o <output file> [-t <zip | unzip> -b <bits to erase>]\nwhere:\n", argv[0]);
    printf("\t-i\tinput file that need to be compressed or decompressed\n\n");
    printf("\t-o\t output file that being compressed or decompressed \n\n");
    printf("\t-b\t bits to be erased, range[0..32], default is 0\n\n");
    printf("\t-s\t data type to be converted to when compressed/decompressed, value should be [float | int], default is float\n\n");
    printf("\t-t\t operation type, e.g compress or decompressed file, value should be [zip | unzip], default is zip\n\n");
    printf("\t-e\t absolute error bound: every decoded float within eps of the original, eps > 0 (zip only; excludes -b and -s int) (extension of the MI355X build)\n\n");
    printf("\t-k\t zip: also write <output file>.crc, the CRC-32 digest sidecar of what the container decodes to (extension of the MI355X build)\n\n");
    printf("\t-K\t unzip: check what is decoded against this digest sidecar; exit status 1 when it differs (extension of the MI355X build)\n\n");
    printf("\t-g\t first HIP device to use, default 0 (extension of the MI355X build)\n\n");
    printf("\t-G\t number of HIP devices the file's chunks are dealt to, default 1; 0 = all visible devices (extension of the MI355X build)\n\n");
}

static double wall_now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

int main(int argc, char *argv[])
{
    const double t_main = wall_now();
    const char *in = NULL, *out = NULL, *op = "zip", *dtype = "float";
    const char *eps = NULL, *check = NULL;
    int bits = 0, opt, dev0 = 0, ndev = 1, write_digest = 0, status = 0;
    if (argc < 2) { usage(argv); exit(-1); }
    while ((opt = getopt(argc, argv, "hi:o:b:t:s:g:G:e:kK:")) != -1) {
        switch (opt) {
        case 'i': in = optarg; break;
        case 'o': out = optarg; break;
        case 'b': bits = atoi(optarg); break;
        case 't': op = optarg; break;
        case 's': dtype = optarg; break;
        case 'g': dev0 = atoi(optarg); break;
        case 'G': ndev = atoi(optarg); break;
        case 'e': eps = optarg; break;
        case 'k': write_digest = 1; break;
        case 'K': check = optarg; break;
        case 'h': usage(argv); return 0;
        default: printf("Invalid command line parameters!\n"); usage(argv); return -1;
        }
    }
    if (!in || !out) { usage(argv); return -1; }
    if (eps && strcmp(op, "zip") == 0) {
        char *end;
        const double e = strtod(eps, &end);
        if (end == eps || *end || bits != 0 || strcmp(dtype, "int") == 0 || e == 0.0 || mrcz_workers_set_abs_error(e) != 0) {
            printf("Invalid command line parameters: -e needs a finite bound > 0 and excludes -b and -s int\n");
            usage(argv);
            return -1;
        }
    }
    const int zip = strcmp(op, "zip") == 0, int_mode = strcmp(dtype, "int") == 0;
    if ((write_digest && !zip) || (check && strcmp(op, "unzip") != 0)) {
        printf("Invalid command line parameters: -k goes with -t zip, -K with -t unzip\n");
        usage(argv);
        return -1;
    }
    sidecar_t sc;
    memset(&sc, 0, sizeof sc);
    if (check) {
        const char *why = NULL;
        if (sidecar_read(check, &sc, &why) != 0) { fprintf(stderr, "Error: [%s:%d]: %s: %s\n", __FILE__, __LINE__, why, check); exit(-1); }
    }
    if (write_digest || check) mrcz_workers_set_digest(1);
    if (ndev != 1) {
        /* -G n: the file's chunks are dealt over n GPUs of the node, -G 0 over all of them.  Opt-in: every extra
         * device costs an engine (workspace, streams, batch buffers) inside the timed call, which one file has to be large to
         * repay, and the path has been rehearsed on one GPU with aliased engines only (hardware scaling unmeasured). */
        const int have = mrcz_device_count();
        if (ndev <= 0) ndev = have - dev0;
        if (ndev < 1) ndev = 1;
    }
    mrcz_workers_set_devices(dev0, ndev);
    const double t_devices = wall_now();
    printf("CODEC:mrcz-hip gfx950 (DEFLATE Z_RLE stream-compatible with ZLIB:1.2.8)\n"); /* mrc_tar.c:152 prints the zlib version */
    ctx_t ctx;
    init_context(&ctx);
    ctx.fileCount += 1;
    FILE *fin = fopen(in, "rb");
    if (!fin) { fprintf(stderr, "Error: [%s:%d]: Failed to  open input file :%s\n", __FILE__, __LINE__, in); exit(-1); }
    FILE *fout = fopen(out, "wb");
    if (!fout) { fprintf(stderr, "Error: [%s:%d]: Failed to open output file [%s] to write\n", __FILE__, __LINE__, out); exit(-1); }
    const double t_open = wall_now();
    if (strcmp(op, "zip") == 0) { /* mrc_tar.c:24-54 */
        ctx.allFileSize += get_file_size(fin);
        run_compress(fin, &ctx, fout, bits, dtype);
        print_context_info(&ctx, "Contex Info after Compression");
        if (write_digest) { /* <output>.crc: the chunk digests the pipeline collected, in file order */
            const uint32_t *crcs = NULL;
            uint32_t file_crc = 0;
            const uint64_t nch = mrcz_workers_last_digest(&crcs, &file_crc), nfl = get_file_size(fin) / 4u;
            char *name = (char *)malloc(strlen(out) + 5);
            if (!name) exit(-1);
            sprintf(name, "%s.crc", out);
            FILE *fc = fopen(name, "wb");
            if (!fc || sidecar_write(fc, nfl, MRCZ_CHUNK_FLOATS, nch, int_mode, file_crc, crcs) != 0 || fclose(fc) != 0) {
                fprintf(stderr, "Error: [%s:%d]: Failed to write the digest sidecar [%s]\n", __FILE__, __LINE__, name);
                exit(-1);
            }
            free(name);
        }
    } else if (strcmp(op, "unzip") == 0) { /* mrc_tar.c:56-80 */
        mrczip_header_t hd;
        init_mrczip_header(&hd, 0);
        if (read_mrczip_header(fin, &hd) != 0) { fclose(fin); fclose(fout); return -1; }
        print_mrczip_header(&hd, "Header Info in Decompression");
        if (check) { /* a sidecar of another file is refused before anything is decoded */
            const uint64_t nfl = hd.fsz / 4u;
            if (hd.chk == 0 || sc.words != nfl || sc.chunk != hd.chk || sc.chunks != (nfl + hd.chk - 1) / hd.chk) {
                fprintf(stderr, "Error: [%s:%d]: the sidecar is of another file: words, chunk or chunks differ from the container's header\n", __FILE__, __LINE__);
                exit(-1);
            }
        }
        run_uncompress(fin, &ctx, &hd, fout, dtype);
        print_context_info(&ctx, "Contex Info after Decompression");
        if (check) {
            const uint32_t *crcs = NULL;
            uint32_t file_crc = 0;
            const uint64_t nch = mrcz_workers_last_digest(&crcs, &file_crc);
            if (nch != sc.chunks) status = 1;
            for (uint64_t c = 0; c < nch && c < sc.chunks; c++)
                if (crcs[c] != sc.crcs[c]) { status = 1; printf("chunk %" PRIu64 " expected %08" PRIx32 " got %08" PRIx32 "\n", c, sc.crcs[c], crcs[c]); }
            if (file_crc != sc.file) status = 1;
            printf("file expected %08" PRIx32 " got %08" PRIx32 "\n", sc.file, file_crc);
        }
    }
    const double t_run = wall_now();
    fclose(fout);
    fclose(fin);
    if (getenv("MRCZ_TRACE")) /* (what is left of the command's wall time is the loader before main and the HIP runtime's teardown behind it) */
        fprintf(stderr, "[mrcz trace] main: HIP runtime up + device count %.4f s, open %.4f, run %.4f, close %.4f, whole main %.4f s\n", t_devices - t_main,
                t_open - t_devices, t_run - t_open, wall_now() - t_run, wall_now() - t_main);
    /* Everything is on disk.  Leaving through the HIP runtime's static destructors (streams, pinned buffers, device memory,
     * one by one) costs another 0.1 s of the command's wall time; the process's death releases the same things.
     * MRCZ_FULL_TEARDOWN=1 keeps the orderly way (leak checkers). */
    if (!getenv("MRCZ_FULL_TEARDOWN")) { fflush(stdout); fflush(stderr); _exit(status); }
    return status;
}
