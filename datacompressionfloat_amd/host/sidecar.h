/*
 * sidecar.h -- the digest sidecar of a container: a text file that carries the CRC-32 of what the container
 * decodes to, for the file and for every chunk.  One writer and one parser for the host tools (mrc_verify -k / -K, mrc_tar -k / -K).
 *
 *   mrcz-digest crc32 1
 *   words <nfl> chunk <chk> chunks <nch> mode <float|int>
 *   file <8 lowercase hex digits>
 *   <c> <8 hex digits>          one line per chunk, c = 0 .. nch-1
 */
#ifndef MRCZ_SIDECAR_H_
#define MRCZ_SIDECAR_H_

#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint64_t words, chunks;
    uint32_t chunk;
    int int_mode;
    uint32_t file;
    uint32_t *crcs; /* chunks entries (malloc) */
} sidecar_t;

static int sidecar_write(FILE *f, uint64_t words, uint32_t chunk, uint64_t chunks, int int_mode, uint32_t file, const uint32_t *crcs)
{
    fprintf(f, "mrcz-digest crc32 1\nwords %" PRIu64 " chunk %" PRIu32 " chunks %" PRIu64 " mode %s\nfile %08" PRIx32 "\n", words, chunk, chunks,
            int_mode ? "int" : "float", file);
    for (uint64_t c = 0; c < chunks; c++) fprintf(f, "%" PRIu64 " %08" PRIx32 "\n", c, crcs[c]);
    return ferror(f) ? -1 : 0;
}

/* a decimal number of at most 20 digits, no sign, ended by `end`; returns the position behind `end` or NULL */
static const char *sidecar_num(const char *s, char end, uint64_t *v)
{
    uint64_t x = 0;
    int n = 0;
    for (; *s >= '0' && *s <= '9'; s++, n++) {
        if (n >= 20 || x > (UINT64_MAX - (uint64_t)(*s - '0')) / 10u) return NULL;
        x = x * 10u + (uint64_t)(*s - '0');
    }
    if (n == 0 || *s != end) return NULL;
    *v = x;
    return s + 1;
}
/* exactly 8 lowercase hex digits, then '\n' */
static const char *sidecar_hex(const char *s, uint32_t *v)
{
    uint32_t x = 0;
    for (int i = 0; i < 8; i++, s++) {
        if (*s >= '0' && *s <= '9') x = (x << 4) | (uint32_t)(*s - '0');
        else if (*s >= 'a' && *s <= 'f') x = (x << 4) | (uint32_t)(*s - 'a' + 10);
        else return NULL;
    }
    if (*s != '\n') return NULL;
    *v = x;
    return s + 1;
}
static const char *sidecar_word(const char *s, const char *w)
{
    const size_t n = strlen(w);
    return strncmp(s, w, n) == 0 ? s + n : NULL;
}

/* parse the sidecar at `path`; 0, or -1 with *why set (unreadable, or not a sidecar).  sc->crcs is the caller's to free. */
static int sidecar_read(const char *path, sidecar_t *sc, const char **why)
{
    memset(sc, 0, sizeof(*sc));
    FILE *f = fopen(path, "rb");
    *why = "cannot open the sidecar";
    if (!f) return -1;
    *why = "cannot read the sidecar";
    if (fseek(f, 0, SEEK_END) != 0) { fclose(f); return -1; }
    const long size = ftell(f);
    if (size < 0 || size > (1L << 30) || fseek(f, 0, SEEK_SET) != 0) { fclose(f); return -1; }
    char *buf = (char *)malloc((size_t)size + 1);
    if (!buf || fread(buf, 1, (size_t)size, f) != (size_t)size) { free(buf); fclose(f); return -1; }
    fclose(f);
    buf[size] = 0;
    *why = "not a digest sidecar";
    int rc = -1;
    uint64_t chk = 0;
    const char *s = buf;
    if (strlen(buf) != (size_t)size) goto out; /* a NUL byte inside */
    if (!(s = sidecar_word(s, "mrcz-digest crc32 1\nwords ")) || !(s = sidecar_num(s, ' ', &sc->words))) goto out;
    if (!(s = sidecar_word(s, "chunk ")) || !(s = sidecar_num(s, ' ', &chk))) goto out;
    if (!(s = sidecar_word(s, "chunks ")) || !(s = sidecar_num(s, ' ', &sc->chunks))) goto out;
    if (!(s = sidecar_word(s, "mode "))) goto out;
    if (sidecar_word(s, "float\n")) { s += 6; sc->int_mode = 0; }
    else if (sidecar_word(s, "int\n")) { s += 4; sc->int_mode = 1; }
    else goto out;
    if (chk == 0 || chk > UINT32_MAX || sc->chunks != sc->words / chk + (sc->words % chk ? 1u : 0u)) goto out;
    sc->chunk = (uint32_t)chk;
    if (sc->chunks > (uint64_t)size / 11u) goto out; /* a chunk line has at least 11 bytes */
    if (!(s = sidecar_word(s, "file ")) || !(s = sidecar_hex(s, &sc->file))) goto out;
    sc->crcs = (uint32_t *)malloc(4u * (size_t)(sc->chunks ? sc->chunks : 1));
    if (!sc->crcs) goto out;
    for (uint64_t c = 0; c < sc->chunks; c++) {
        uint64_t n = 0;
        if ((*s == '0' && s[1] != ' ') || !(s = sidecar_num(s, ' ', &n)) || n != c || !(s = sidecar_hex(s, &sc->crcs[c]))) goto out;
    }
    if (*s) goto out; /* something behind the last chunk line */
    rc = 0;
out:
    free(buf);
    if (rc != 0) { free(sc->crcs); sc->crcs = NULL; }
    return rc;
}

#endif /* MRCZ_SIDECAR_H_ */
