/* gtfsort.c -- `lr2rmats sort-gtf` and `lr2rmats sort-gtf-check`: GTF files merged and put into the order update-gtf, unique-gtf and
 * STAR read them in -- the step the reference pipeline runs as a shell script after each of its two concatenations of GTF files.
 *
 * The order is l2r_gtf_order's (include/lr2rmats_hip.h): of the concatenated text the lines are kept whose third field contains
 * "transcript" or equals "exon" and whose first byte is not '#'; a transcript line sets the key (chromosome rank, start, end) that it
 * and the kept lines behind it carry; the kept lines are ordered by that key and then by line number.  The engine orders rows (offset,
 * length, line number); the bytes stay here, and h_gtf_write_rows writes every row as its first nine tab-separated columns.
 *
 * `sort-gtf-check` answers "would sort-gtf only drop and trim lines?" on the host, with the engine's exact host routine
 * (l2r_gtf_check): it needs no GPU. */
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "l2r_host.h"

/* the files, concatenated byte for byte in argument order; *n_out = bytes (the buffer holds one more) */
uint8_t *h_gtf_read_files(int n_files, char **fn, int64_t *n_out, const char *who)
{
    size_t cap = 1 << 20, n = 0;
    uint8_t *buf = (uint8_t *)h_malloc(cap);
    for (int k = 0; k < n_files; ++k) {
        FILE *f = fopen(fn[k], "rb");
        if (!f) h_fatal(who, "Can not open \"%s\"\n", fn[k]);
        for (;;) {
            if (cap - n < (1 << 16)) {
                cap *= 2;
                uint8_t *q = (uint8_t *)realloc(buf, cap);
                if (!q) h_fatal(who, "out of memory (%zu bytes)\n", cap);
                buf = q;
            }
            const size_t got = fread(buf + n, 1, cap - n - 1, f);
            if (got == 0) break;
            n += got;
        }
        if (ferror(f)) h_fatal(who, "Error in reading \"%s\"\n", fn[k]);
        fclose(f);
    }
    *n_out = (int64_t)n;
    return buf;
}

int h_gtf_write_rows(const uint8_t *text, int64_t n_bytes, int64_t n_rows, const uint64_t *start, const uint32_t *len, const uint32_t *line, FILE *out)
{
    (void)line;                                          /* a row's line number is not written */
    for (int64_t k = 0; k < n_rows; ++k) {
        if (start[k] > (uint64_t)n_bytes || (uint64_t)len[k] > (uint64_t)n_bytes - start[k]) return -1;
        const uint8_t *p = text + start[k], *end = p + len[k];
        int col = 1;
        const uint8_t *q = p;
        for (; q < end; ++q) if (*q == '\t' && ++col > 9) break;          /* q: the tenth column's tab, or the line's end */
        if (q > p && fwrite(p, 1, (size_t)(q - p), out) != (size_t)(q - p)) return -1;
        for (; col < 9; ++col) if (fputc('\t', out) == EOF) return -1;   /* missing columns are empty */
        if (fputc('\n', out) == EOF) return -1;
    }
    return 0;
}

int h_gtf_write_rows_path(const uint8_t *text, int64_t n_bytes, int64_t n_rows, const uint64_t *start, const uint32_t *len, const uint32_t *line, const char *path)
{
    FILE *out = fopen(path, "wb");
    if (!out) return -1;
    int rc = h_gtf_write_rows(text, n_bytes, n_rows, start, len, line, out);
    if (fclose(out) != 0) rc = -1;
    return rc;
}

/* ------------------------------------------------------------------ sort-gtf */

static int gtf_sort_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s sort-gtf [option] <in.gtf> [more.gtf ...] > out.sort.gtf\n\n", "lr2rmats");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "         -o --output     [STR]      write the sorted GTF to this file. [stdout]\n");
    fprintf(stderr, "\n");
    fprintf(stderr, "Note:    the files are concatenated byte for byte.  Transcript and exon lines are kept; every transcript, with the lines\n");
    fprintf(stderr, "         behind it, is placed by chromosome (chr1..chr22, chrX, chrY, chrM, then other names as they appear), start and\n");
    fprintf(stderr, "         end; lines that compare equal keep their order.  Each line is written as its first nine tab-separated columns.\n");
    fprintf(stderr, "         Plain text only.\n\n");
    return 2;
}

int h_gtf_sort_run(int n_files, char **fn, FILE *out, int64_t *counts)
{
    int64_t n = 0;
    h_stage_time("start");
    uint8_t *text = h_gtf_read_files(n_files, fn, &n, "sort_gtf");
    h_stage_time("read files");
    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("sort_gtf", "%s", l2r_last_error());
    h_stage_time("engine: create");
    const l2r_gtf_text t = { n, text };
    int64_t n_rows = 0;
    if (l2r_gtf_order(ctx, &t, &n_rows)) {
        fprintf(stderr, "[sort_gtf] %s\n", l2r_last_error());
        l2r_destroy(ctx); free(text);
        return 1;
    }
    l2r_gtf_rows rows = { n_rows, 0, (uint64_t *)h_malloc((size_t)(n_rows + 1) * 8), (uint32_t *)h_malloc((size_t)(n_rows + 1) * 4), (uint32_t *)h_malloc((size_t)(n_rows + 1) * 4) };
    if (l2r_gtf_rows_out(ctx, &rows)) h_fatal("sort_gtf", "%s", l2r_last_error());
    double st[17];
    if (l2r_gtf_stats(ctx, st, 17)) h_fatal("sort_gtf", "%s", l2r_last_error());
    h_stage_time("engine: order (upload, kernels, download)");
    l2r_destroy(ctx);
    if (h_gtf_write_rows(text, n, rows.n, rows.start, rows.len, rows.line, out)) h_fatal("sort_gtf", "Error in writing GTF line\n");
    h_stage_time("write GTF");
    if (counts) { counts[0] = (int64_t)st[1]; counts[1] = rows.n; counts[2] = (int64_t)st[3]; counts[3] = (int64_t)st[16]; }
    free(rows.start); free(rows.len); free(rows.line); free(text);
    return 0;
}

int h_cmd_sort_gtf(int argc, char **argv)
{
    static const struct option long_opt[] = { { "output", 1, NULL, 'o' }, { 0, 0, 0, 0 } };
    const char *out_fn = NULL;
    int c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:", long_opt, NULL)) >= 0) {
        switch (c) {
        case 'o': out_fn = optarg; break;
        default: return gtf_sort_usage();
        }
    }
    if (argc - optind < 1) return gtf_sort_usage();
    FILE *out = stdout;
    if (out_fn && !(out = fopen(out_fn, "wb"))) h_fatal("sort_gtf", "Can not open \"%s\" for writing\n", out_fn);
    int64_t cnt[4] = { 0, 0, 0, 0 };
    int rc = h_gtf_sort_run(argc - optind, argv + optind, out, cnt);
    if (out != stdout && fclose(out) != 0) rc = 1;
    if (rc == 0 && out == stdout && fflush(stdout) != 0) rc = 1;
    if (rc == 0) fprintf(stderr, "Sorted GTF: %lld of %lld lines in %lld transcripts, %lld chromosomes\n", (long long)cnt[1], (long long)cnt[0], (long long)cnt[2], (long long)cnt[3]);
    return rc;
}

/* ------------------------------------------------------------------ sort-gtf-check (no GPU) */

static int gtf_check_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s sort-gtf-check <in.gtf>\n\n", "lr2rmats");
    fprintf(stderr, "Note:    exit status 0 where the kept lines of the file are in the order of `%s sort-gtf` already (it would only drop\n", "lr2rmats");
    fprintf(stderr, "         and trim lines), else 1 and the first kept line (1-based) whose key is below its predecessor's on stdout.\n\n");
    return 2;
}

int h_cmd_sort_gtf_check(int argc, char **argv)
{
    if (argc != 2 || argv[1][0] == '-') return gtf_check_usage();
    int64_t n = 0;
    uint8_t *text = h_gtf_read_files(1, argv + 1, &n, "sort_gtf_check");
    const l2r_gtf_text t = { n, text };
    int64_t line = 0, cnt[4] = { 0, 0, 0, 0 };
    const int rc = l2r_gtf_check(&t, &line, cnt);
    if (rc < 0) { fprintf(stderr, "[sort_gtf_check] %s\n", l2r_last_error()); free(text); return 1; }
    if (rc == 0) printf("GTF sorted: %lld of %lld lines in %lld transcripts, %lld chromosomes\n", (long long)cnt[1], (long long)cnt[0], (long long)cnt[2], (long long)cnt[3]);
    else printf("GTF not sorted: line %lld is below its predecessor\n", (long long)line);
    fflush(stdout);
    free(text);
    return rc;
}
