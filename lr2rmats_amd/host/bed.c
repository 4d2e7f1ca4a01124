/* bed.c -- `lr2rmats bam2bed`: every mapped alignment record as one BED12 line with the blocks between its introns -- the step the
 * reference pipeline runs as `bedtools bamtobed -bed12` behind minimap2 (Snakefile, rule minimap_map).  The rule of a line is
 * l2r_bed_lines' (include/lr2rmats_hip.h); no byte equality with the output of any bedtools release is claimed.
 *
 *   records      SAM text, gzip/BGZF SAM or BAM -> BAM-encoded records in memory (h_read_records, filter.c); MAPQ and the names are
 *                taken from the raw records
 *   batches      l2r_bed_cut: at most L2R_BED_BATCH records (default 1 Mi) and L2R_BED_TEXT_MAX bytes of summed line bounds (default
 *                1 GiB) -- device and text memory are bounded by the batch, the records are not
 *   text         the engine composes a batch's text on the GPU (l2r_bed_lines); it is fetched and written as it arrives
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include "l2r_host.h"

/* three decimal numbers 0..255 with commas between them and nothing else */
int h_bed_color_ok(const char *s)
{
    for (int k = 0; k < 3; ++k) {
        int n = 0, v = 0;
        while (*s >= '0' && *s <= '9' && n < 4) { v = v * 10 + (*s - '0'); ++s; ++n; }
        if (n < 1 || n > 3 || v > 255) return 0;
        if (k < 2) { if (*s != ',') return 0; ++s; }
    }
    return *s == 0;
}

static int64_t env_count(const char *name, int64_t dflt)
{
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long long v = atoll(e);
    return v >= 1 ? (int64_t)v : dflt;
}

int h_bed_run(const char *in_fn, const char *color, FILE *out, int64_t *counts)
{
    if (!color) color = "255,0,0";
    if (!h_bed_color_ok(color)) { fprintf(stderr, "[bam2bed] \"%s\" is not a colour (r,g,b with 0..255 each)\n", color); return 2; }
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_records r;
    h_stage_time("start");
    h_read_records(in_fn, &chr, &r, "bam2bed");
    h_stage_time("read + encode records");
    /* MAPQ and the names, from the raw records (as h_name_order makes them) */
    uint8_t *mapq = (uint8_t *)h_malloc((size_t)r.n + 1);
    int64_t *name_off = (int64_t *)h_malloc((size_t)(r.n + 1) * 8);
    name_off[0] = 0;
    for (int64_t i = 0; i < r.n; ++i) {
        const uint8_t *rec = r.buf + r.rec_off[i] + 4;
        mapq[i] = rec[9];
        name_off[i + 1] = name_off[i] + (int64_t)strlen((const char *)rec + 32);
    }
    uint8_t *names = (uint8_t *)h_malloc((size_t)name_off[r.n] + 1);
    for (int64_t i = 0; i < r.n; ++i) memcpy(names + name_off[i], r.buf + r.rec_off[i] + 4 + 32, (size_t)(name_off[i + 1] - name_off[i]));
    /* the reference names of the header */
    const int n_ref = chr.n_hdr;
    int64_t *ref_off = (int64_t *)h_malloc((size_t)(n_ref + 1) * 8);
    ref_off[0] = 0;
    for (int t = 0; t < n_ref; ++t) ref_off[t + 1] = ref_off[t] + (int64_t)strlen(chr.name[t]);
    uint8_t *ref_names = (uint8_t *)h_malloc((size_t)ref_off[n_ref] + 1);
    for (int t = 0; t < n_ref; ++t) memcpy(ref_names + ref_off[t], chr.name[t], (size_t)(ref_off[t + 1] - ref_off[t]));
    l2r_bed_params prm;
    memset(&prm, 0, sizeof prm);
    prm.n_ref = n_ref; prm.ref_off = ref_off; prm.ref_names = ref_names;
    prm.color_len = (int32_t)strlen(color);
    memcpy(prm.color, color, (size_t)prm.color_len);

    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("bam2bed", "%s", l2r_last_error());
    h_stage_time("engine: create");
    if (l2r_bed_begin(ctx, &prm)) h_fatal("bam2bed", "%s", l2r_last_error());
    const int64_t max_records = env_count("L2R_BED_BATCH", (int64_t)1 << 20), max_bytes = env_count("L2R_BED_TEXT_MAX", (int64_t)1 << 30);
    const l2r_bed_records all = { r.n, r.n_cig, r.flag, r.tid, r.pos, mapq, r.cig_off, r.cig, name_off, names };
    uint8_t *text = NULL; int64_t text_cap = 0;
    int64_t n_lines = 0, n_bytes = 0, n_batches = 0;
    int rc = 0;
    for (int64_t first = 0; first < r.n && !rc;) {
        int64_t take = 0, lines = 0, bytes = 0;
        if (l2r_bed_cut(&all, &prm, first, max_records, max_bytes, &take) || take < 1) { fprintf(stderr, "[bam2bed] %s\n", l2r_last_error()); rc = 1; break; }
        /* the batch: a window of the columns */
        const l2r_bed_records b = { take, r.n_cig, r.flag + first, r.tid + first, r.pos + first, mapq + first, r.cig_off + first, r.cig, name_off + first, names };
        if (l2r_bed_lines(ctx, &b, &lines, &bytes)) {
            const char *msg = l2r_last_error(), *at = strstr(msg, "record ");
            long long k = -1;
            if (at && sscanf(at, "record %lld", &k) == 1 && k >= 0) fprintf(stderr, "[bam2bed] %s (record %lld of the file)\n", msg, (long long)first + k);
            else fprintf(stderr, "[bam2bed] %s\n", msg);
            rc = 1;
            break;
        }
        if (bytes > text_cap) { free(text); text_cap = bytes + bytes / 4 + 64; text = (uint8_t *)h_malloc((size_t)text_cap); }
        if (bytes) {
            if (l2r_bed_text_out(ctx, text, text_cap)) h_fatal("bam2bed", "%s", l2r_last_error());
            if (fwrite(text, 1, (size_t)bytes, out) != (size_t)bytes) h_fatal("bam2bed", "Error in writing BED line\n");
        }
        n_lines += lines; n_bytes += bytes; ++n_batches;
        first += take;
    }
    h_stage_time("engine: lines (upload, kernels, download) + write BED");
    l2r_destroy(ctx);
    if (counts) { counts[0] = r.n; counts[1] = n_lines; counts[2] = n_bytes; counts[3] = n_batches; }
    free(text); free(mapq); free(name_off); free(names); free(ref_off); free(ref_names);
    h_records_free(&r); h_chroms_free(&chr);
    return rc;
}

int h_bed_run_path(const char *in_fn, const char *color, const char *out_path, int64_t *counts)
{
    FILE *out = fopen(out_path, "wb");
    if (!out) return -1;
    int rc = h_bed_run(in_fn, color, out, counts);
    if (fclose(out) != 0 && rc == 0) rc = -1;
    return rc;
}

static int bed_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s bam2bed [option] <in.bam/sam> > out.bed\n\n", "lr2rmats");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "         -o --output     [STR]      write the BED12 lines to this file. [stdout]\n");
    fprintf(stderr, "         -c --color      [STR]      the colour column: r,g,b with 0..255 each. [255,0,0]\n");
    fprintf(stderr, "\n");
    fprintf(stderr, "Note:    one line per mapped record, in input order: reference, start, end, name (/1 or /2 for mates), MAPQ, strand,\n");
    fprintf(stderr, "         start, end, colour, block count, block sizes and block starts.  An N operation of the CIGAR ends a block.\n\n");
    return 2;
}

int h_cmd_bam2bed(int argc, char **argv)
{
    static const struct option long_opt[] = { { "output", 1, NULL, 'o' }, { "color", 1, NULL, 'c' }, { 0, 0, 0, 0 } };
    const char *out_fn = NULL, *color = "255,0,0";
    int c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:c:", long_opt, NULL)) >= 0) {
        switch (c) {
        case 'o': out_fn = optarg; break;
        case 'c': color = optarg; break;
        default: return bed_usage();
        }
    }
    if (argc - optind != 1 || !h_bed_color_ok(color)) return bed_usage();
    FILE *out = stdout;
    if (out_fn && !(out = fopen(out_fn, "wb"))) h_fatal("bam2bed", "Can not open \"%s\" for writing\n", out_fn);
    int64_t cnt[4] = { 0, 0, 0, 0 };
    int rc = h_bed_run(argv[optind], color, out, cnt);
    if (out != stdout && fclose(out) != 0 && rc == 0) rc = 1;
    if (rc == 0 && out == stdout && fflush(stdout) != 0) rc = 1;
    if (rc == 0) fprintf(stderr, "Converted alignments: %lld lines of %lld records\n", (long long)cnt[1], (long long)cnt[0]);
    return rc;
}
