/* sort.c -- `lr2rmats sort`, `lr2rmats sort-check` and what `filter -S` shares with them: coordinate-sorted BAM, the step the
 * reference pipeline leaves to an external tool between `filter` and `update-gtf` (Snakefile, rule sam_novel_gtf).  `sort -n`,
 * `sort-check -n` and what `filter -N` / `fusion -N` share with them: the name order -- records with one name consecutive, groups by
 * first appearance, input order inside a group (l2r_name_order; h_header_grouped: @HD says SO:unsorted GO:query) -- the step in front
 * of `filter` and `fusion`, which take a run of consecutive records with one name for a read.  No equality with the output of any
 * samtools release is claimed for either order.
 *
 *   records      SAM text, gzip/BGZF SAM or BAM -> BAM-encoded records in memory (h_read_records, filter.c)
 *   order        the engine: l2r_sort_order() over FLAG, tid and pos -- one 64-bit key per record (h_sort_key below), stable
 *   header       the @HD line says SO:coordinate (h_header_coordinate)
 *   output       BGZF-compressed BAM, the records gathered on the host in that order (h_write_bam)
 *
 * `sort-check` answers "is this file fit for update-gtf?" on the host: it walks the same keys and names the first record that is
 * below its predecessor.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include "l2r_host.h"

static inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

uint64_t h_sort_key(int32_t tid, int32_t pos, uint32_t flag)
{
    const uint64_t t = tid < 0 ? 0x7fffffffull : (uint64_t)(uint32_t)tid;
    return (t << 33) | ((uint64_t)((uint32_t)pos + 1u) << 1) | (uint64_t)((flag >> 4) & 1u);
}

#define SO_FIELD "SO:coordinate"
#define HD_LINE  "@HD\tVN:1.6\t" SO_FIELD "\n"

int64_t h_header_coordinate(const uint8_t *hdr, size_t hdr_len, uint8_t *out, size_t out_cap)
{
    if (hdr_len < 12 || memcmp(hdr, "BAM\1", 4) != 0) return -1;
    const size_t l_text = le32(hdr + 4);
    if (8 + l_text + 4 > hdr_len) return -1;
    const char *text = (const char *)hdr + 8;
    /* [0, cut) of the text stays, `ins` goes in, [skip, l_text) follows */
    size_t cut = 0, skip = 0;
    const char *ins = HD_LINE;
    if (l_text >= 3 && memcmp(text, "@HD", 3) == 0 && (l_text == 3 || text[3] == '\t' || text[3] == '\n' || text[3] == '\r' || text[3] == 0)) {
        size_t le = 3;                                        /* end of the line: in front of "\r\n", "\n", a NUL or the end of the text */
        while (le < l_text && text[le] != '\n' && text[le] != 0) ++le;
        if (le > 3 && text[le - 1] == '\r') --le;
        size_t f = 3;
        cut = skip = le; ins = "\t" SO_FIELD;                 /* no SO field: appended to the line */
        while (f < le) {                                      /* text[f] == '\t': a field starts behind it */
            size_t fe = f + 1;
            while (fe < le && text[fe] != '\t') ++fe;
            if (fe - f > 3 && memcmp(text + f + 1, "SO:", 3) == 0) { cut = f + 1; skip = fe; ins = SO_FIELD; break; }
            f = fe;
        }
    }
    const size_t l_ins = strlen(ins), new_text = cut + l_ins + (l_text - skip), total = hdr_len - l_text + new_text;
    if (new_text > 0xffffffffu) return -1;
    if (out && total <= out_cap) {
        memcpy(out, hdr, 4);
        put32(out + 4, (uint32_t)new_text);
        memcpy(out + 8, text, cut);
        memcpy(out + 8 + cut, ins, l_ins);
        memcpy(out + 8 + cut + l_ins, text + skip, l_text - skip);
        memcpy(out + 8 + new_text, hdr + 8 + l_text, hdr_len - 8 - l_text);
    }
    return (int64_t)total;
}

void h_records_set_coordinate(h_records *r, const char *who)
{
    const size_t cap = r->hdr_len + H_HEADER_SO_ROOM;
    uint8_t *hdr = (uint8_t *)h_malloc(cap);
    const int64_t len = h_header_coordinate(r->hdr, r->hdr_len, hdr, cap);
    if (len < 0 || (size_t)len > cap) h_fatal(who, "corrupt BAM header");
    free(r->hdr);
    r->hdr = hdr; r->hdr_len = (size_t)len;
}

/* ------------------------------------------------------------------ the name order */

static int hd_line_end(const char *text, size_t l_text, size_t *le)
{
    if (!(l_text >= 3 && memcmp(text, "@HD", 3) == 0 && (l_text == 3 || text[3] == '\t' || text[3] == '\n' || text[3] == '\r' || text[3] == 0))) return 0;
    size_t e = 3;                                             /* end of the line: in front of "\r\n", "\n", a NUL or the end of the text */
    while (e < l_text && text[e] != '\n' && text[e] != 0) ++e;
    if (e > 3 && text[e - 1] == '\r') --e;
    *le = e;
    return 1;
}

int64_t h_header_grouped(const uint8_t *hdr, size_t hdr_len, uint8_t *out, size_t out_cap)
{
    static const char *const want[2] = { "SO:unsorted", "GO:query" };
    if (hdr_len < 12 || memcmp(hdr, "BAM\1", 4) != 0) return -1;
    const size_t l_text = le32(hdr + 4);
    if (8 + l_text + 4 > hdr_len) return -1;
    const char *text = (const char *)hdr + 8;
    size_t le = 0;
    const int has_hd = hd_line_end(text, l_text, &le);
    /* the new line (without its end) replaces text[0, le) */
    char *line = (char *)h_malloc(le + H_HEADER_GO_ROOM);
    size_t ll = 0;
    int seen[2] = { 0, 0 };
    if (has_hd) {
        memcpy(line, "@HD", 3); ll = 3;
        size_t f = 3;
        while (f < le) {                                      /* text[f] == '\t': a field starts behind it */
            size_t fe = f + 1;
            while (fe < le && text[fe] != '\t') ++fe;
            int k = -1;
            if (fe - f > 3 && memcmp(text + f + 1, "SO:", 3) == 0) k = 0;
            else if (fe - f > 3 && memcmp(text + f + 1, "GO:", 3) == 0) k = 1;
            if (k >= 0 && !seen[k]) { line[ll++] = '\t'; memcpy(line + ll, want[k], strlen(want[k])); ll += strlen(want[k]); seen[k] = 1; }
            else if (k < 0) { memcpy(line + ll, text + f, fe - f); ll += fe - f; }      /* (a second SO / GO field goes) */
            f = fe;
        }
    } else { memcpy(line, "@HD\tVN:1.6", 10); ll = 10; }
    for (int k = 0; k < 2; ++k) if (!seen[k]) { line[ll++] = '\t'; memcpy(line + ll, want[k], strlen(want[k])); ll += strlen(want[k]); }
    if (!has_hd) line[ll++] = '\n';
    const size_t new_text = ll + (l_text - le), total = hdr_len - l_text + new_text;
    if (new_text > 0xffffffffu) { free(line); return -1; }
    if (out && total <= out_cap) {
        memcpy(out, hdr, 4);
        put32(out + 4, (uint32_t)new_text);
        memcpy(out + 8, line, ll);
        memcpy(out + 8 + ll, text + le, l_text - le);
        memcpy(out + 8 + new_text, hdr + 8 + l_text, hdr_len - 8 - l_text);
    }
    free(line);
    return (int64_t)total;
}

void h_records_set_grouped(h_records *r, const char *who)
{
    const size_t cap = r->hdr_len + H_HEADER_GO_ROOM;
    uint8_t *hdr = (uint8_t *)h_malloc(cap);
    const int64_t len = h_header_grouped(r->hdr, r->hdr_len, hdr, cap);
    if (len < 0 || (size_t)len > cap) h_fatal(who, "corrupt BAM header");
    free(r->hdr);
    r->hdr = hdr; r->hdr_len = (size_t)len;
}

static inline const char *rec_name(const h_records *r, int64_t i) { return (const char *)(r->buf + r->rec_off[i] + 4 + 32); }

int64_t h_name_order(l2r_ctx *ctx, const h_records *r, int64_t *order, const char *who)
{
    if (r->n == 0) return 0;
    int64_t *off = (int64_t *)h_malloc((size_t)(r->n + 1) * 8);
    off[0] = 0;
    for (int64_t i = 0; i < r->n; ++i) off[i + 1] = off[i] + (int64_t)strlen(rec_name(r, i));
    uint8_t *blob = (uint8_t *)h_malloc((size_t)off[r->n] + 1);
    for (int64_t i = 0; i < r->n; ++i) memcpy(blob + off[i], rec_name(r, i), (size_t)(off[i + 1] - off[i]));
    uint32_t *ord = (uint32_t *)h_malloc((size_t)r->n * 4);
    const l2r_name_records nr = { r->n, off, blob };
    int64_t n_groups = 0;
    if (l2r_name_order(ctx, &nr, ord, &n_groups)) h_fatal(who, "%s", l2r_last_error());
    for (int64_t k = 0; k < r->n; ++k) order[k] = (int64_t)ord[k];
    free(off); free(blob); free(ord);
    return n_groups;
}

void h_sort_order(l2r_ctx *ctx, const h_records *r, const int64_t *rows, int64_t n, int64_t *sorted, const char *who)
{
    if (n == 0) return;
    uint16_t *flag = (uint16_t *)h_malloc((size_t)n * 2);
    int32_t *tid = (int32_t *)h_malloc((size_t)n * 4), *pos = (int32_t *)h_malloc((size_t)n * 4);
    uint32_t *order = (uint32_t *)h_malloc((size_t)n * 4);
    for (int64_t k = 0; k < n; ++k) { const int64_t i = rows ? rows[k] : k; flag[k] = r->flag[i]; tid[k] = r->tid[i]; pos[k] = r->pos[i]; }
    const l2r_sort_records sr = { n, flag, tid, pos };
    if (l2r_sort_order(ctx, &sr, order)) h_fatal(who, "%s", l2r_last_error());
    for (int64_t k = 0; k < n; ++k) sorted[k] = rows ? rows[order[k]] : (int64_t)order[k];
    free(flag); free(tid); free(pos); free(order);
}

/* ------------------------------------------------------------------ sort */

static int sort_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s sort [option] <in.bam/sam> > out.sort.bam\n\n", "lr2rmats");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "         -o --output     [STR]      write the sorted BAM to this file. [stdout]\n");
    fprintf(stderr, "         -n --name                  group the records by read name instead: what `filter` and `fusion` want. [false]\n");
    fprintf(stderr, "\n");
    fprintf(stderr, "Note:    records are ordered by reference, position and strand, records without a reference last; records that\n");
    fprintf(stderr, "         compare equal keep their input order.  The header's @HD line is given SO:coordinate.\n");
    fprintf(stderr, "         -n: the records of one read name are consecutive, the reads follow each other by their first record in the\n");
    fprintf(stderr, "         input, and the records of a read keep their input order.  @HD is given SO:unsorted and GO:query.\n\n");
    return 1;
}

int h_sort_run(const char *in_fn, FILE *out, int64_t *n_written) { return h_sort_run_named(in_fn, 0, out, n_written, NULL); }

int h_sort_run_named(const char *in_fn, int by_name, FILE *out, int64_t *n_written, int64_t *n_groups)
{
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_records r;
    h_stage_time("start");
    h_read_records(in_fn, &chr, &r, "bam_sort");
    h_stage_time("read + encode records");
    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("bam_sort", "%s", l2r_last_error());
    h_stage_time("engine: create");
    int64_t *order = (int64_t *)h_malloc((size_t)(r.n + 1) * 8);
    if (by_name) { const int64_t g = h_name_order(ctx, &r, order, "bam_sort"); if (n_groups) *n_groups = g; }
    else h_sort_order(ctx, &r, NULL, r.n, order, "bam_sort");
    h_stage_time("engine: order (upload, kernels, download)");
    l2r_destroy(ctx);
    if (by_name) h_records_set_grouped(&r, "bam_sort"); else h_records_set_coordinate(&r, "bam_sort");
    if (h_write_bam(out, &r, order, r.n)) h_fatal("bam_sort", "Error in writing SAM record\n");
    h_stage_time("write BAM (BGZF)");
    if (n_written) *n_written = r.n;
    free(order); h_records_free(&r); h_chroms_free(&chr);
    return 0;
}

int h_cmd_sort(int argc, char **argv)
{
    static const struct option long_opt[] = { { "output", 1, NULL, 'o' }, { "name", 0, NULL, 'n' }, { 0, 0, 0, 0 } };
    const char *out_fn = NULL;
    int c, by_name = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:n", long_opt, NULL)) >= 0) {
        switch (c) {
        case 'o': out_fn = optarg; break;
        case 'n': by_name = 1; break;
        default: return sort_usage();
        }
    }
    if (argc - optind != 1) return sort_usage();
    FILE *out = stdout;
    if (out_fn && !(out = fopen(out_fn, "wb"))) h_fatal("bam_sort", "Can not open \"%s\" for writing\n", out_fn);
    int64_t cnt = 0, groups = 0;
    int rc = h_sort_run_named(argv[optind], by_name, out, &cnt, &groups);
    if (out != stdout && fclose(out) != 0) rc = 1;
    if (by_name) fprintf(stderr, "[%s] Grouped alignments: %lld in %lld reads\n", "bam_sort", (long long)cnt, (long long)groups);
    else fprintf(stderr, "[%s] Sorted alignments: %lld\n", "bam_sort", (long long)cnt);
    return rc;
}

/* ------------------------------------------------------------------ sort-check (no GPU) */

static int sort_check_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s sort-check [-n] <in.bam/sam>\n\n", "lr2rmats");
    fprintf(stderr, "Note:    exit status 0 where no record is below its predecessor in the order of `%s sort`, else 1 and the\n", "lr2rmats");
    fprintf(stderr, "         first such record (0-based index and read name) on stdout.\n");
    fprintf(stderr, "         -n: exit status 0 where the records of every read name are consecutive, else 1 and the first record whose\n");
    fprintf(stderr, "         name was seen in an earlier group.\n\n");
    return 2;
}

static const h_records *g_check_rec;
static int cmp_heads(const void *a, const void *b)
{
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    const int c = strcmp(rec_name(g_check_rec, x), rec_name(g_check_rec, y));
    return c ? c : (x < y ? -1 : x > y);
}

int64_t h_name_grouped(const h_records *r, int64_t *n_groups)
{
    /* the first record of every run of one name; sorted by (name, index), a name that opens two runs has them side by side */
    int64_t *head = (int64_t *)h_malloc((size_t)(r->n + 1) * 8), n_head = 0, bad = -1;
    for (int64_t i = 0; i < r->n; ++i) if (i == 0 || strcmp(rec_name(r, i), rec_name(r, i - 1)) != 0) head[n_head++] = i;
    if (n_groups) *n_groups = n_head;
    g_check_rec = r;
    qsort(head, (size_t)n_head, sizeof *head, cmp_heads);
    for (int64_t k = 1; k < n_head; ++k)
        if (strcmp(rec_name(r, head[k]), rec_name(r, head[k - 1])) == 0 && (bad < 0 || head[k] < bad)) bad = head[k];
    free(head);
    return bad;
}

static int sort_check_names(const char *fn)
{
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_records r;
    h_read_records(fn, &chr, &r, "sort_check");
    int64_t n_groups = 0;
    const int64_t bad = h_name_grouped(&r, &n_groups);
    if (bad < 0) printf("name grouped: %lld records in %lld reads\n", (long long)r.n, (long long)n_groups);
    else printf("not name grouped: record %lld (\"%s\") has the name of an earlier group\n", (long long)bad, rec_name(&r, bad));
    fflush(stdout);
    h_records_free(&r); h_chroms_free(&chr);
    return bad < 0 ? 0 : 1;
}

int h_cmd_sort_check(int argc, char **argv)
{
    if (argc == 3 && strcmp(argv[1], "-n") == 0 && argv[2][0] != '-') return sort_check_names(argv[2]);
    if (argc != 2 || argv[1][0] == '-') return sort_check_usage();
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_records r;
    h_read_records(argv[1], &chr, &r, "sort_check");
    int64_t bad = -1;
    uint64_t prev = 0;
    for (int64_t i = 0; i < r.n; ++i) {
        const uint64_t k = h_sort_key(r.tid[i], r.pos[i], r.flag[i]);
        if (k < prev) { bad = i; break; }
        prev = k;
    }
    if (bad < 0) printf("coordinate sorted: %lld records\n", (long long)r.n);
    else printf("not coordinate sorted: record %lld (\"%s\") is below its predecessor\n", (long long)bad, (const char *)(r.buf + r.rec_off[bad] + 4 + 32));
    fflush(stdout);
    h_records_free(&r); h_chroms_free(&chr);
    return bad < 0 ? 0 : 1;
}
