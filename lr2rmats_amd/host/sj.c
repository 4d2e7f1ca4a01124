/* sj.c -- `lr2rmats bam2sj` (reference src/parse_bam.c:987-1058): the junction table of an alignment file.
 *
 *   records   SAM text, gzip / BGZF SAM or BAM, read as a stream (zlib inflates all three): FLAG, refID, position, CIGAR words and
 *             the NH verdict of one batch at a time -- memory is bounded by the batch (L2R_SJ_BATCH records), not by the file
 *   genome    -g: plain or gzip FASTA -> one byte array + offsets, sequences in FILE order (a record's refID indexes them)
 *   table     the engine: l2r_sj_begin / _add per batch / _finish / _download (include/lr2rmats_hip.h)
 *   output    the four header lines and one line per junction (print_sj :974-985)
 *
 * `lr2rmats sjtab` (the end of this file) is the same source and engine with the table `update-gtf -j` reads: nine columns, no header,
 * annotated flag from a GTF, maximum overhang, and the filter the usage text of bam2sj only advertises; with -d, -m or -s also the
 * intron-size rule and the distance to the nearest other junction (l2r_sj_filter_rows2).
 *
 * The reference keeps ONE list and, per junction, searches it backwards for its place (sj_sch_group :339-351).  Where the tids of
 * the records never decrease that list is the table sorted by (tid, don, acc) -- what the engine makes.  Where a tid decreases, the
 * search stops early inside the block of a larger tid and the list is no sort at all: such input takes h_sj_literal(), the same
 * insertion on the host, so the bytes are the reference's there too.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include "l2r_host.h"

#define SJ_INTRON_MIN_LEN 3     /* src/gtf.h:118 */
#define SJ_DEFAULT_BATCH ((int64_t)4 << 20)

static inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

/* ------------------------------------------------------------------ FASTA */

void h_fasta_free(h_fasta *f)
{
    for (int32_t i = 0; i < f->n_seq; ++i) free(f->name[i]);
    free(f->name); free(f->seq_off); free(f->bases);
    memset(f, 0, sizeof *f);
}

/* A '>' at the start of a line opens a sequence, its name ends at the first blank; every other line adds its bytes without the
 * line end (and without a '\r' in front of it) to the open sequence.  The bytes are packed where the file was inflated. */
void h_read_fasta(const char *fn, h_fasta *out, const char *who)
{
    memset(out, 0, sizeof *out);
    h_blob b = h_slurp(fn, who);
    int32_t cap = 0;
    size_t w = 0;
    const uint8_t *p = b.p, *end = b.p + b.n;
    while (p < end) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        const uint8_t *e = nl ? nl : end;
        const uint8_t *le = (e > p && e[-1] == '\r') ? e - 1 : e;
        if (le > p && *p == '>') {
            if (out->n_seq == cap) {
                cap = cap ? cap * 2 : 32;
                out->name = (char **)h_realloc(out->name, (size_t)cap * sizeof(char *));
                out->seq_off = (int64_t *)h_realloc(out->seq_off, ((size_t)cap + 1) * 8);
            }
            const uint8_t *q = p + 1;
            while (q < le && *q != ' ' && *q != '\t') ++q;
            out->name[out->n_seq] = strndup((const char *)p + 1, (size_t)(q - p - 1));
            out->seq_off[out->n_seq++] = (int64_t)w;
        } else if (out->n_seq > 0 && le > p) {
            memmove(b.p + w, p, (size_t)(le - p));          /* (w <= p - b.p: the header lines and line ends are dropped) */
            w += (size_t)(le - p);
        }
        p = nl ? nl + 1 : end;
    }
    if (!out->seq_off) out->seq_off = (int64_t *)h_malloc(8);
    out->seq_off[out->n_seq] = (int64_t)w;
    out->bases = b.p;
}

/* ------------------------------------------------------------------ record source */

struct h_sj_source {
    gzFile g;
    uint8_t *buf; size_t lo, hi, cap;
    int eof, is_bam;
    h_chroms *chr;
    const char *who, *fn;
};

/* at least `want` bytes behind lo, if the file has them; returns the bytes there are */
static size_t src_fill(h_sj_source *s, size_t want)
{
    if (s->hi - s->lo >= want) return s->hi - s->lo;
    if (s->lo) { memmove(s->buf, s->buf + s->lo, s->hi - s->lo); s->hi -= s->lo; s->lo = 0; }
    if (want > s->cap) { size_t c = s->cap; while (c < want) c *= 2; s->buf = (uint8_t *)h_realloc(s->buf, c); s->cap = c; }
    while (!s->eof && s->hi < want) {
        const int k = gzread(s->g, s->buf + s->hi, (unsigned)(s->cap - s->hi > (1u << 30) ? (1u << 30) : s->cap - s->hi));
        if (k < 0) h_fatal(s->who, "read error in \"%s\"", s->fn);
        if (k == 0) s->eof = 1;
        s->hi += (size_t)k;
    }
    return s->hi - s->lo;
}

static const uint8_t *src_need(h_sj_source *s, size_t n, const char *what)
{
    if (src_fill(s, n) < n) h_fatal(s->who, "truncated %s in \"%s\"", what, s->fn);
    return s->buf + s->lo;
}

/* one text line: [*p, *e) without its end; 0 at the end of the file.  The line is consumed. */
static int src_line(h_sj_source *s, const char **p, const char **e)
{
    size_t from = 0;
    for (;;) {
        const size_t have = s->hi - s->lo;
        const uint8_t *nl = have > from ? (const uint8_t *)memchr(s->buf + s->lo + from, '\n', have - from) : NULL;
        if (nl || s->eof) {
            if (!nl && have == 0) return 0;
            const uint8_t *b = s->buf + s->lo, *le = nl ? nl : b + have;
            s->lo += (size_t)(le - b) + (nl ? 1 : 0);
            if (le > b && le[-1] == '\r') --le;
            *p = (const char *)b; *e = (const char *)le;
            return 1;
        }
        from = have;
        src_fill(s, have + (1 << 16));
    }
}

static void sam_header_line(const char *p, const char *e, h_chroms *chr, const char *who)
{
    if (e - p < 4 || memcmp(p, "@SQ", 3) != 0) return;
    for (const char *q = p; q < e;) {
        const char *t = (const char *)memchr(q, '\t', (size_t)(e - q));
        const char *fe = t ? t : e;
        if (fe - q > 3 && memcmp(q, "SN:", 3) == 0) {
            char name[H_NAME_MAX];
            if (fe - q - 3 >= H_NAME_MAX) h_fatal(who, "reference name of 100 or more characters");
            memcpy(name, q + 3, (size_t)(fe - q - 3)); name[fe - q - 3] = 0;
            h_chrom_intern(chr, name);
        }
        if (!t) break;
        q = t + 1;
    }
}

h_sj_source *h_sj_source_open(const char *fn, h_chroms *chr, const char *who)
{
    h_sj_source *s = (h_sj_source *)h_malloc(sizeof *s);
    memset(s, 0, sizeof *s);
    s->g = gzopen(fn, "rb");                                   /* plain files pass through, gzip and BGZF members are inflated */
    if (!s->g) h_fatal_core(who, "Cannot open \"%s\"\n", fn);
    gzbuffer(s->g, 1 << 20);
    s->cap = (size_t)1 << 22; s->buf = (uint8_t *)h_malloc(s->cap);
    s->chr = chr; s->who = who; s->fn = fn;
    if (src_fill(s, 4) >= 4 && memcmp(s->buf, "BAM\1", 4) == 0) {
        s->is_bam = 1;
        const uint32_t l_text = le32(src_need(s, 8, "BAM header") + 4);
        const uint32_t n_ref = le32(src_need(s, 12 + (size_t)l_text, "BAM header") + 8 + l_text);
        s->lo += 12 + (size_t)l_text;
        for (uint32_t i = 0; i < n_ref; ++i) {
            const uint32_t l_name = le32(src_need(s, 4, "BAM header"));
            const uint8_t *p = src_need(s, 8 + (size_t)l_name, "BAM header");
            if (l_name == 0 || p[4 + l_name - 1] != 0) h_fatal(who, "corrupt BAM header in \"%s\"", fn);
            h_chrom_intern(chr, (const char *)p + 4);
            s->lo += 8 + (size_t)l_name;
        }
    } else {
        for (;;) {                                             /* the '@' lines; the first record stays where it is */
            if (src_fill(s, 1) < 1 || s->buf[s->lo] != '@') break;
            const char *p, *e;
            if (!src_line(s, &p, &e)) break;
            sam_header_line(p, e, chr, who);
        }
    }
    chr->n_hdr = chr->n;
    return s;
}

void h_sj_source_close(h_sj_source *s)
{
    if (!s) return;
    gzclose(s->g); free(s->buf); free(s);
}

void h_sj_batch_free(h_sj_batch *b)
{
    free(b->flag); free(b->tid); free(b->pos); free(b->uniq); free(b->nh_seen); free(b->cig_off); free(b->cig);
    memset(b, 0, sizeof *b);
}

static void batch_reserve(h_sj_batch *b, int64_t more_cig)
{
    if (b->n + 2 > b->cap) {
        const int64_t c = b->cap ? b->cap * 2 : 1 << 12;
        b->flag = (uint16_t *)h_realloc(b->flag, (size_t)c * 2); b->tid = (int32_t *)h_realloc(b->tid, (size_t)c * 4);
        b->pos = (int32_t *)h_realloc(b->pos, (size_t)c * 4); b->uniq = (uint8_t *)h_realloc(b->uniq, (size_t)c);
        b->nh_seen = (uint8_t *)h_realloc(b->nh_seen, (size_t)c); b->cig_off = (int64_t *)h_realloc(b->cig_off, (size_t)(c + 1) * 8);
        b->cap = c;
    }
    if (b->n_cig + more_cig + 1 > b->cap_cig) {
        int64_t c = b->cap_cig ? b->cap_cig * 2 : 1 << 14;
        while (c < b->n_cig + more_cig + 1) c *= 2;
        b->cig = (uint32_t *)h_realloc(b->cig, (size_t)c * 4); b->cap_cig = c;
    }
}

static size_t sj_aux_size(uint8_t type, const uint8_t *p, const uint8_t *end)
{
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    case 'Z': case 'H': { const uint8_t *z = (const uint8_t *)memchr(p, 0, (size_t)(end - p)); return z ? (size_t)(z - p) + 1 : 0; }
    case 'B': {
        if (end - p < 5) return 0;
        size_t w;
        switch (p[0]) { case 'c': case 'C': w = 1; break; case 's': case 'S': w = 2; break; case 'i': case 'I': case 'f': w = 4; break; default: return 0; }
        return 5 + w * (size_t)le32(p + 1);
    }
    default: return 0;
    }
}

/* bam_is_uniq_NH (src/parse_bam.c:240-248): the first NH tag; bam_aux2i() is its value for the integer types and 0 for any other */
static void bam_record(h_sj_source *s, const uint8_t *rec, uint32_t bs, h_sj_batch *b)
{
    const uint8_t *rend = rec + bs;
    const uint32_t l_read_name = rec[8], n_cig = le16(rec + 12), l_seq = le32(rec + 16);
    const uint8_t *cig = rec + 32 + l_read_name;
    const uint8_t *aux = cig + 4 * (size_t)n_cig + ((size_t)l_seq + 1) / 2 + l_seq;
    if (bs < 32 || aux > rend) h_fatal(s->who, "corrupt BAM record in \"%s\"", s->fn);
    const uint8_t *cg = NULL; uint32_t cg_n = 0;
    long long nh = 0; int nh_seen = 0;
    for (const uint8_t *a = aux; a + 3 <= rend;) {
        const uint8_t t = a[2];
        const size_t sz = sj_aux_size(t, a + 3, rend);
        if (sz == 0 || a + 3 + sz > rend) h_fatal(s->who, "corrupt BAM aux field in \"%s\"", s->fn);
        if (!nh_seen && a[0] == 'N' && a[1] == 'H') {
            nh_seen = 1;
            switch (t) {
            case 'c': nh = (int8_t)a[3]; break; case 'C': nh = a[3]; break;
            case 's': nh = (int16_t)le16(a + 3); break; case 'S': nh = le16(a + 3); break;
            case 'i': nh = (int32_t)le32(a + 3); break; case 'I': nh = le32(a + 3); break;
            default: nh = 0;
            }
        }
        if (a[0] == 'C' && a[1] == 'G' && t == 'B' && a[3] == 'I') { cg_n = le32(a + 4); cg = a + 8; }
        a += 3 + sz;
    }
    /* beyond 65535 operations the CIGAR sits in CG:B,I behind a <l_seq>S<ref len>N placeholder (htslib swaps it back in) */
    const uint8_t *cp = cig; uint32_t cn = n_cig;
    if (cg && n_cig == 2 && (le32(cig) & 15u) == 4 && (le32(cig) >> 4) == l_seq && (le32(cig + 4) & 15u) == 3) { cp = cg; cn = cg_n; }
    batch_reserve(b, cn);
    const int64_t i = b->n;
    b->tid[i] = (int32_t)le32(rec); b->pos[i] = (int32_t)le32(rec + 4); b->flag[i] = (uint16_t)le16(rec + 14);
    b->nh_seen[i] = (uint8_t)nh_seen; b->uniq[i] = nh_seen && nh == 1;
    for (uint32_t k = 0; k < cn; ++k) b->cig[b->n_cig++] = le32(cp + 4 * (size_t)k);
    b->cig_off[i + 1] = b->n_cig;
    b->n = i + 1;
}

static void sam_record(h_sj_source *s, const char *p, const char *e, h_sj_batch *b)
{
    const char *f[12], *fe[11]; int nf = 0; const char *q = p;
    while (nf < 11) {
        f[nf] = q;
        const char *t = (const char *)memchr(q, '\t', (size_t)(e - q));
        fe[nf++] = t ? t : e;
        if (!t) { q = e; break; }
        q = t + 1;
    }
    if (nf < 11) h_fatal(s->who, "truncated SAM record in \"%s\"", s->fn);
    f[11] = q;
    uint32_t flag = (uint32_t)strtoul(f[1], NULL, 0);
    int tid = -1;
    if (!(fe[2] - f[2] == 1 && f[2][0] == '*')) {
        char name[H_NAME_MAX];
        const size_t len = (size_t)(fe[2] - f[2]);
        if (len >= H_NAME_MAX) h_fatal(s->who, "reference name too long");
        memcpy(name, f[2], len); name[len] = 0;
        tid = h_chrom_find(s->chr, name, s->chr->n_hdr);
        if (tid < 0) h_fatal(s->who, "record \"%.*s\": reference \"%s\" is not in the header", (int)(fe[0] - f[0]), f[0], name);
    }
    batch_reserve(b, (int64_t)(fe[5] - f[5]));
    const int64_t i = b->n;
    if (fe[5] - f[5] == 1 && f[5][0] == '*') flag |= 4u;       /* htslib: a mapped record must have a CIGAR; treated as unmapped */
    else {
        for (const char *c = f[5]; c < fe[5];) {
            uint32_t len = 0;
            while (c < fe[5] && *c >= '0' && *c <= '9') { len = len * 10u + (uint32_t)(*c - '0'); ++c; }
            if (c >= fe[5]) h_fatal(s->who, "bad CIGAR");
            uint32_t op;
            switch (*c) {
            case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'N': op = 3; break;
            case 'S': op = 4; break; case 'H': op = 5; break; case 'P': op = 6; break; case '=': op = 7; break;
            case 'X': op = 8; break; case 'B': op = 9; break;
            default: h_fatal(s->who, "bad CIGAR operator '%c'", *c); op = 0;
            }
            b->cig[b->n_cig++] = (len << 4) | op;
            ++c;
        }
    }
    int nh_seen = 0; long long nh = 0;
    for (const char *a = f[11]; a < e && !nh_seen;) {
        const char *t = (const char *)memchr(a, '\t', (size_t)(e - a));
        const char *ae = t ? t : e;
        if (ae - a >= 5 && a[0] == 'N' && a[1] == 'H' && a[2] == ':' && a[4] == ':') {
            nh_seen = 1;
            nh = (a[3] == 'i' || a[3] == 'I') ? strtoll(a + 5, NULL, 10) : 0;
        }
        if (!t) break;
        a = t + 1;
    }
    b->tid[i] = tid; b->pos[i] = (int32_t)strtol(f[3], NULL, 10) - 1; b->flag[i] = (uint16_t)flag;
    b->nh_seen[i] = (uint8_t)nh_seen; b->uniq[i] = nh_seen && nh == 1;
    b->cig_off[i + 1] = b->n_cig;
    b->n = i + 1;
}

int64_t h_sj_source_next(h_sj_source *s, h_sj_batch *b, int64_t max_records)
{
    b->n = 0; b->n_cig = 0;
    batch_reserve(b, 0);
    b->cig_off[0] = 0;
    while (b->n < max_records) {
        if (s->is_bam) {
            const size_t have = src_fill(s, 4);
            if (have == 0) break;
            const uint32_t bs = le32(src_need(s, 4, "BAM record"));
            const uint8_t *rec = src_need(s, 4 + (size_t)bs, "BAM record") + 4;
            bam_record(s, rec, bs, b);
            s->lo += 4 + (size_t)bs;
        } else {
            const char *p, *e;
            if (!src_line(s, &p, &e)) break;
            if (e == p || *p == '@') continue;
            sam_record(s, p, e, b);
        }
    }
    return b->n;
}

/* ------------------------------------------------------------------ the reference's list, literally */

/* Rows in record order -> the list sj_update_group() builds (src/parse_bam.c:339-380): per row the list is searched from its END
 * backwards; an entry with the row's coordinates takes the row's counts; the search stops behind the first entry that has a smaller
 * tid, OR a smaller donor (whatever its tid), OR the same donor and a smaller acceptor (whatever its tid), and the row is inserted
 * there; a search that reaches the front inserts at the front.  out columns: room for n rows.  Returns the rows of the list. */
int64_t h_sj_literal(int64_t n, const int32_t *tid, const int32_t *don, const int32_t *acc, const int32_t *uniq_c, const int32_t *multi_c,
                     int32_t *o_tid, int32_t *o_don, int32_t *o_acc, int32_t *o_uniq, int32_t *o_multi)
{
    int64_t m = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t t = tid[r], d = don[r], a = acc[r];
        int64_t at = 0; int hit = 0;
        for (int64_t i = m - 1; i >= 0; --i) {
            if (o_tid[i] == t && o_don[i] == d && o_acc[i] == a) { hit = 1; at = i; break; }
            if (o_tid[i] < t || o_don[i] < d || (o_don[i] == d && o_acc[i] < a)) { at = i + 1; break; }
        }
        if (hit) { o_uniq[at] += uniq_c[r]; o_multi[at] += multi_c[r]; continue; }
        const size_t tail = (size_t)(m - at) * 4;
        memmove(o_tid + at + 1, o_tid + at, tail); memmove(o_don + at + 1, o_don + at, tail); memmove(o_acc + at + 1, o_acc + at, tail);
        memmove(o_uniq + at + 1, o_uniq + at, tail); memmove(o_multi + at + 1, o_multi + at, tail);
        o_tid[at] = t; o_don[at] = d; o_acc[at] = a; o_uniq[at] = uniq_c[r]; o_multi[at] = multi_c[r];
        ++m;
    }
    return m;
}

/* intr_deri_str (src/parse_bam.c:319-337) on the host, for the literal list: motif 1..6 or 0; strand = 1 for the odd motifs, 2 for
 * the even ones.  A base outside its sequence matches nothing. */
static int host_motif(const h_fasta *g, int32_t tid, int32_t don, int32_t acc)
{
    static const char motif[6][5] = {"GTAG", "CTAC", "GCAG", "CTGC", "ATAC", "GTAT"};
    if (tid < 0) return 0;
    const int64_t s0 = g->seq_off[tid], len = g->seq_off[tid + 1] - s0;
    const int64_t at[4] = {(int64_t)don - 1, don, (int64_t)acc - 2, (int64_t)acc - 1};
    char w[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        if (at[k] < 0 || at[k] >= len) return 0;
        char c = (char)g->bases[s0 + at[k]];
        w[k] = (c >= 'a' && c <= 'z') ? (char)(c - 32) : c;
    }
    for (int k = 0; k < 6; ++k) if (memcmp(w, motif[k], 4) == 0) return k + 1;
    return 0;
}

/* ------------------------------------------------------------------ the sub-command */

static int bam2sj_usage(void)
{
    /* src/parse_bam.c:44-69 */
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s bam2sj [option] <in.bam> > out.sj\n\n", "lr2rmats");
    fprintf(stderr, "Note:    in.bam should be sorted in advance\n\n");
    fprintf(stderr, "Input Options:\n\n");
    fprintf(stderr, "         -G --gtf-anno    [STR]    GTF annotation file, indicating known splice-junctions. \n");
    fprintf(stderr, "         -g --genome-file [STR]    genome.fa. Use genome sequence to classify intron-motif. \n");
    fprintf(stderr, "                                   If no genome file is give, intron-motif will be set as 0\n");
    fprintf(stderr, "                                   (non-canonical) [None]\n");
    fprintf(stderr, "\nFilter Options:\n\n");
    fprintf(stderr, "         -p --prop-pair            set -p to force to filter out reads mapped in improper pair. [False]\n");
    fprintf(stderr, "         -a --anchor-len  [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum anchor length for junction read, [annotated, non-canonical,\n");
    fprintf(stderr, "                                    GT/AG, GC/AG, AT/AC]. [%d,%d,%d,%d,%d]\n", 1, 30, 12, 12, 12);
    fprintf(stderr, "         -U --uniq-map    [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum uniq-map read count for junction read, [annotated,\n");
    fprintf(stderr, "                                   non-canonical, GT/AG, GC/AG, AT/AC]. [%d,%d,%d,%d,%d]\n", 0, 3, 1, 1, 1);
    fprintf(stderr, "         -A --all-map     [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum total uniq-map and multi-map read count for junction\n");
    fprintf(stderr, "                                   read, [annotated, non-canonical, GT/AG, GC/AG, AT/AC].\n");
    fprintf(stderr, "                                   [%d,%d,%d,%d,%d]\n", 0, 3, 1, 1, 1);
    fprintf(stderr, "         -i --intron-len  [INT]    minimum intron length for junction read. [%d]\n", SJ_INTRON_MIN_LEN);
    fprintf(stderr, "\n");
    return 1;
}

/* -a / -U / -A: five integers with ONE character of any kind between them (:998-1015); 0 when the text ends early */
static int five_ints(const char *arg)
{
    char *p;
    (void)strtol(arg, &p, 10);
    for (int k = 1; k < 5; ++k) {
        if (*p == 0) return 0;
        (void)strtol(p + 1, &p, 10);
    }
    return 1;
}

static void print_header(FILE *out)
{
    fprintf(out, "###STRAND 0:undefined, 1:+, 2:-\n");
    fprintf(out, "###ANNO 0:novel, 1:annotated\n");
    fprintf(out, "###MOTIF 0:non-canonical, 1:GT/AG, 2:CT/AC, 3:GC/AG, 4:CT/GC, 5:AT/AC, 6:GT/AT\n");
    fprintf(out, "#CHR\tSTART\tEND\tSTRAND\tANNO\tUNIQ_C\tMULTI_C\tMOTIF\n");
}

static void print_row(FILE *out, const h_chroms *chr, int32_t tid, int32_t don, int32_t acc, int strand, int32_t uq, int32_t mc, int motif)
{
    if (tid < 0 || tid >= chr->n_hdr) h_fatal("print_sj", "junction on reference %d, the header has %d", tid, chr->n_hdr);
    fprintf(out, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", chr->name[tid], don, acc, strand, 1, uq, mc, motif);      /* ANNO: add_sj(..., 1, ...) :416 */
}

/* src/parse_bam.c:909-914; the message of bam_is_uniq_NH for the records [from, n) that reach it */
static void report_missing_nh(const h_sj_batch *b, int64_t from)
{
    for (int64_t i = from; i < b->n; ++i) if (!(b->flag[i] & 4u) && !b->nh_seen[i]) fprintf(stderr, "No \"NH\" tag.\n");
}

/* The whole file on the host: rows by a plain walk in record order, the reference's list, motifs.  nh_reported: records whose
 * missing NH tag the first attempt has reported already. */
static int bam2sj_literal(const char *fn, const h_fasta *g, int have_genome, int min_intron, int64_t batch_records, int64_t nh_reported)
{
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_sj_source *src = h_sj_source_open(fn, &chr, "bam2sj");
    h_sj_batch b; memset(&b, 0, sizeof b);
    int32_t *col[5] = {NULL, NULL, NULL, NULL, NULL}; int64_t n = 0, cap = 0, seen = 0;
    while (h_sj_source_next(src, &b, batch_records) > 0) {
        report_missing_nh(&b, nh_reported > seen ? (nh_reported - seen < b.n ? nh_reported - seen : b.n) : 0);
        seen += b.n;
        for (int64_t i = 0; i < b.n; ++i) {
            if ((b.flag[i] & 4u) || !(b.flag[i] & 2u)) continue;
            int32_t end = b.pos[i];
            for (int64_t k = b.cig_off[i]; k < b.cig_off[i + 1]; ++k) {
                const uint32_t op = b.cig[k] & 15u; const int32_t len = (int32_t)(b.cig[k] >> 4);
                if (op == 3u && len >= min_intron) {
                    if (have_genome && b.tid[i] >= g->n_seq) h_fatal("intr_deri_str", "unknown tid: %d", b.tid[i]);
                    if (n == cap) { cap = cap ? cap * 2 : 1 << 12; for (int q = 0; q < 5; ++q) col[q] = (int32_t *)h_realloc(col[q], (size_t)cap * 4); }
                    col[0][n] = b.tid[i]; col[1][n] = end + 1; col[2][n] = end + len; col[3][n] = b.uniq[i]; col[4][n] = 1 - b.uniq[i]; ++n;
                }
                if ((0x18du >> op) & 1u) end += len;
            }
        }
    }
    h_sj_source_close(src); h_sj_batch_free(&b);
    int32_t *o[5];
    for (int q = 0; q < 5; ++q) o[q] = (int32_t *)h_malloc((size_t)(n + 1) * 4);
    const int64_t m = h_sj_literal(n, col[0], col[1], col[2], col[3], col[4], o[0], o[1], o[2], o[3], o[4]);
    print_header(stdout);
    for (int64_t i = 0; i < m; ++i) {
        const int mo = have_genome ? host_motif(g, o[0][i], o[1][i], o[2][i]) : 0;
        print_row(stdout, &chr, o[0][i], o[1][i], o[2][i], mo ? 2 - (mo & 1) : 0, o[3][i], o[4][i], mo);
    }
    fflush(stdout);
    for (int q = 0; q < 5; ++q) { free(col[q]); free(o[q]); }
    h_chroms_free(&chr);
    return 0;
}

int h_cmd_bam2sj(int argc, char **argv)
{
    /* option table src/parse_bam.c:216-226 (--proper-pair takes an argument, -p none), getopt string :993 */
    static const struct option lopt[] = {
        {"proper-pair", 1, NULL, 'p'}, {"gtf-anno", 1, NULL, 'G'}, {"genome-file", 1, NULL, 'g'}, {"anchor-len", 1, NULL, 'a'},
        {"uniq-map", 1, NULL, 'U'}, {"all-map", 1, NULL, 'A'}, {"intron-len", 1, NULL, 'i'}, {0, 0, 0, 0}};
    const char *ref_fn = NULL;
    int min_intron = SJ_INTRON_MIN_LEN, c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "G:g:pa:i:A:U:", lopt, NULL)) >= 0) {
        switch (c) {
        case 'g': ref_fn = optarg; break;
        case 'p': break;                                       /* read_type is PAIR_T already (:76): see below */
        case 'a': case 'U': case 'A': if (!five_ints(optarg)) return bam2sj_usage(); break;      /* parsed, never read */
        case 'i': min_intron = atoi(optarg); break;
        default: fprintf(stderr, "Error: unknown option: %s.\n", optarg); return bam2sj_usage();   /* -G too: its case is commented out */
        }
    }
    if (argc - optind != 1) return bam2sj_usage();
    const char *in_fn = argv[optind];
    h_fasta g; memset(&g, 0, sizeof g);
    int have_genome = ref_fn && ref_fn[0];
    if (have_genome) {
        FILE *t = fopen(ref_fn, "rb");
        if (!t) h_fatal("bam2sj", "Can not open genome file. %s\n", ref_fn);
        fclose(t);
        fprintf(stderr, "[kseq_load_genome] loading genome fasta file ...\n");
        h_read_fasta(ref_fn, &g, "bam2sj");
        fprintf(stderr, "[kseq_load_genome] loading genome fasta file done!\n");
        if (g.n_seq == 0) { h_fasta_free(&g); have_genome = 0; }       /* intr_deri_str: seq_n == 0 is "no genome" (:322) */
    }
    const char *e = getenv("L2R_SJ_BATCH");
    const int64_t batch_records = e && atoll(e) > 0 ? atoll(e) : SJ_DEFAULT_BATCH;

    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_sj_source *src = h_sj_source_open(in_fn, &chr, "bam2sj");
    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("bam2sj", "%s", l2r_last_error());
    /* sj_init_para sets read_type = PAIR_T and -p sets it again: a record without FLAG & 2 is skipped with and without -p */
    const l2r_sj_params prm = {min_intron, 1};
    const l2r_sj_genome gen = {g.n_seq, g.seq_off, g.bases};
    if (l2r_sj_begin(ctx, &prm, have_genome ? &gen : NULL)) h_fatal("bam2sj", "%s", l2r_last_error());
    fprintf(stderr, "[bam2sj_core] generating splice-junction with BAM file ...\n");
    h_sj_batch b; memset(&b, 0, sizeof b);
    int32_t last_tid = INT32_MIN; int descends = 0; int64_t seen = 0;
    while (!descends && h_sj_source_next(src, &b, batch_records) > 0) {
        report_missing_nh(&b, 0);
        seen += b.n;
        for (int64_t i = 0; i < b.n && !descends; ++i) {
            if ((b.flag[i] & 4u) || !(b.flag[i] & 2u)) continue;
            if (b.tid[i] < last_tid) descends = 1;
            last_tid = b.tid[i];
        }
        if (descends) break;
        const l2r_sj_records recs = {b.n, b.n_cig, b.flag, b.tid, b.pos, b.uniq, b.cig_off, b.cig};
        if (l2r_sj_add(ctx, &recs)) h_fatal("bam2sj", "%s", l2r_last_error());
    }
    h_sj_source_close(src); h_sj_batch_free(&b);
    int rc = 0;
    if (descends) {
        /* the list of the reference is no sort here (see the head of this file) */
        l2r_destroy(ctx);
        fprintf(stderr, "[bam2sj_core] the records' reference ids descend: the junction list is built on the host, in the reference's search order\n");
        rc = bam2sj_literal(in_fn, &g, have_genome, min_intron, batch_records, seen);
    } else {
        int64_t n = 0;
        const int frc = l2r_sj_finish(ctx, &n);
        if (frc == L2R_SJ_E_UNKNOWN_TID) { fprintf(stderr, "%s\n", l2r_last_error()); l2r_destroy(ctx); exit(EXIT_FAILURE); }
        if (frc) h_fatal("bam2sj", "%s", l2r_last_error());
        int32_t *col[5]; uint8_t *strand = (uint8_t *)h_malloc((size_t)n + 1), *motif = (uint8_t *)h_malloc((size_t)n + 1);
        for (int q = 0; q < 5; ++q) col[q] = (int32_t *)h_malloc((size_t)(n + 1) * 4);
        l2r_sj_table t = {n, 0, col[0], col[1], col[2], col[3], col[4], strand, motif};
        if (l2r_sj_download(ctx, &t)) h_fatal("bam2sj", "%s", l2r_last_error());
        l2r_destroy(ctx);
        print_header(stdout);
        for (int64_t i = 0; i < t.n; ++i) print_row(stdout, &chr, col[0][i], col[1][i], col[2][i], strand[i], col[3][i], col[4][i], motif[i]);
        fflush(stdout);
        for (int q = 0; q < 5; ++q) free(col[q]);
        free(strand); free(motif);
    }
    fprintf(stderr, "[bam2sj_core] generating splice-junction with BAM file done!\n");
    h_chroms_free(&chr);
    if (have_genome) h_fasta_free(&g);
    return rc;
}

/* ------------------------------------------------------------------ `sjtab`: the table update-gtf -j reads */

static int sjtab_usage(void)
{
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s sjtab [option] <in.bam|sam> > SJ.out.tab\n\n", "lr2rmats");
    fprintf(stderr, "Output:  chr, first and last intron base, strand (0 undefined, 1 +, 2 -), motif (0 non-canonical, 1 GT/AG,\n");
    fprintf(stderr, "         2 CT/AC, 3 GC/AG, 4 CT/GC, 5 AT/AC, 6 GT/AT), annotated, unique count, multi count, maximum overhang;\n");
    fprintf(stderr, "         no header, sorted by chr (header order), first base, last base: what `update-gtf -j` reads\n\n");
    fprintf(stderr, "Input Options:\n\n");
    fprintf(stderr, "         -G --gtf-anno    [STR]    GTF annotation file, indicating known splice-junctions. [None]\n");
    fprintf(stderr, "         -g --genome-file [STR]    genome.fa. Use genome sequence to classify intron-motif. \n");
    fprintf(stderr, "                                   If no genome file is give, intron-motif will be set as 0\n");
    fprintf(stderr, "                                   (non-canonical) [None]\n");
    fprintf(stderr, "\nFilter Options:\n\n");
    fprintf(stderr, "         -p --prop-pair            only use reads mapped in proper pair. [False]\n");
    fprintf(stderr, "         -a --anchor-len  [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum anchor length (maximum overhang) of a junction, [annotated,\n");
    fprintf(stderr, "                                   non-canonical, GT/AG, GC/AG, AT/AC]. [%d,%d,%d,%d,%d]\n", 1, 30, 12, 12, 12);
    fprintf(stderr, "         -U --uniq-map    [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum uniq-map read count of a junction. [%d,%d,%d,%d,%d]\n", 0, 3, 1, 1, 1);
    fprintf(stderr, "         -A --all-map     [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum total uniq-map and multi-map read count of a junction; a junction\n");
    fprintf(stderr, "                                   that meets -U or -A is kept. [%d,%d,%d,%d,%d]\n", 0, 3, 1, 1, 1);
    fprintf(stderr, "         -i --intron-len  [INT]    minimum intron length for junction read. [%d]\n", SJ_INTRON_MIN_LEN);
    fprintf(stderr, "         -d --dist-other  [INT,INT,INT,INT,INT]\n");
    fprintf(stderr, "                                   minimum distance of a junction's donor and of its acceptor to those of\n");
    fprintf(stderr, "                                   every other junction that meets the options above. [%d,%d,%d,%d,%d]\n", 0, 0, 0, 0, 0);
    fprintf(stderr, "         -m --intron-max  [INT[,INT...]]\n");
    fprintf(stderr, "                                   up to 8 lengths: a junction that is not annotated and is seen by n reads\n");
    fprintf(stderr, "                                   (n up to the length of the list) spans the n-th length at most. [None]\n");
    fprintf(stderr, "         -s --star-filter          -d %d,%d,%d,%d,%d -m %d,%d,%d: the defaults of STAR's outSJfilterDistToOtherSJmin\n", 0, 10, 0, 5, 10, 50000, 100000, 200000);
    fprintf(stderr, "                                   and outSJfilterIntronMaxVsReadN. -d -m -s apply from left to right.\n");
    fprintf(stderr, "\nOutput Options:\n\n");
    fprintf(stderr, "         -o --output      [STR]    junction table. [stdout]\n");
    fprintf(stderr, "\n");
    return 1;
}

/* -a / -U / -A of sjtab: exactly five decimal integers with a comma between them and nothing else; 1 and out[] on success, else 0 */
int h_sj_five_ints(const char *arg, int32_t out[5])
{
    if (!arg) return 0;
    const char *p = arg;
    for (int k = 0; k < 5; ++k) {
        if (k && *p++ != ',') return 0;
        const char *d = p;
        if (*d == '-' || *d == '+') ++d;
        if (*d < '0' || *d > '9') return 0;
        char *e;
        const long v = strtol(p, &e, 10);
        if (v < INT32_MIN || v > INT32_MAX) return 0;
        out[k] = (int32_t)v;
        p = e;
    }
    return *p == 0;
}

/* -m of sjtab: 1 to cap decimal integers with a comma between them and nothing else, none negative; the count and out[], else 0 */
int h_sj_int_list(const char *arg, int32_t *out, int cap)
{
    if (!arg) return 0;
    const char *p = arg;
    int k = 0;
    for (;;) {
        if (k == cap || *p < '0' || *p > '9') return 0;
        char *e;
        const long long v = strtoll(p, &e, 10);
        if (v > INT32_MAX) return 0;
        out[k++] = (int32_t)v;
        p = e;
        if (*p == 0) return k;
        if (*p++ != ',') return 0;
    }
}

int h_cmd_sjtab(int argc, char **argv)
{
    static const struct option lopt[] = {
        {"prop-pair", 0, NULL, 'p'}, {"gtf-anno", 1, NULL, 'G'}, {"genome-file", 1, NULL, 'g'}, {"anchor-len", 1, NULL, 'a'},
        {"uniq-map", 1, NULL, 'U'}, {"all-map", 1, NULL, 'A'}, {"intron-len", 1, NULL, 'i'}, {"output", 1, NULL, 'o'}, {"dist-other", 1, NULL, 'd'},
        {"intron-max", 1, NULL, 'm'}, {"star-filter", 0, NULL, 's'}, {0, 0, 0, 0}};
    static const l2r_sj_filter2 star = {{0, 10, 0, 5, 10}, 3, {50000, 100000, 200000, 0, 0, 0, 0, 0}};
    const char *ref_fn = NULL, *gtf_fn = NULL, *out_fn = NULL;
    l2r_sj_filter flt = {{1, 30, 12, 12, 12}, {0, 3, 1, 1, 1}, {0, 3, 1, 1, 1}};
    l2r_sj_filter2 flt2; memset(&flt2, 0, sizeof flt2);
    int min_intron = SJ_INTRON_MIN_LEN, pair_only = 0, second = 0, c;       /* second: -d, -m or -s was given */
    optind = 1;
    while ((c = getopt_long(argc, argv, "G:g:pa:i:A:U:o:d:m:s", lopt, NULL)) >= 0) {
        switch (c) {
        case 'g': ref_fn = optarg; break;
        case 'G': gtf_fn = optarg; break;
        case 'p': pair_only = 1; break;
        case 'a': if (!h_sj_five_ints(optarg, flt.anchor_min)) return sjtab_usage(); break;
        case 'U': if (!h_sj_five_ints(optarg, flt.uniq_min)) return sjtab_usage(); break;
        case 'A': if (!h_sj_five_ints(optarg, flt.all_min)) return sjtab_usage(); break;
        case 'i': min_intron = atoi(optarg); break;
        case 'o': out_fn = optarg; break;
        case 'd': {
            if (!h_sj_five_ints(optarg, flt2.dist_min)) return sjtab_usage();
            for (int k = 0; k < 5; ++k) if (flt2.dist_min[k] < 0) return sjtab_usage();
            second = 1; break;
        }
        case 'm': {
            int32_t v[8];
            const int k = h_sj_int_list(optarg, v, 8);
            if (!k) return sjtab_usage();
            memset(flt2.intron_max, 0, sizeof flt2.intron_max); memcpy(flt2.intron_max, v, (size_t)k * sizeof v[0]);
            flt2.n_intron_max = k; second = 1; break;
        }
        case 's': flt2 = star; second = 1; break;
        default: fprintf(stderr, "Error: unknown option: %s.\n", optarg); return sjtab_usage();
        }
    }
    if (argc - optind != 1) return sjtab_usage();
    const char *in_fn = argv[optind];
    h_fasta g; memset(&g, 0, sizeof g);
    int have_genome = ref_fn && ref_fn[0];
    if (have_genome) {
        FILE *t = fopen(ref_fn, "rb");
        if (!t) h_fatal("sjtab", "Can not open genome file. %s\n", ref_fn);
        fclose(t);
        h_read_fasta(ref_fn, &g, "sjtab");
        if (g.n_seq == 0) { h_fasta_free(&g); have_genome = 0; }
    }
    if (gtf_fn) {
        FILE *t = fopen(gtf_fn, "rb");
        if (!t) h_fatal("sjtab", "Can not open annotation file. %s\n", gtf_fn);
        fclose(t);
    }
    const char *e = getenv("L2R_SJ_BATCH");
    const int64_t batch_records = e && atoll(e) > 0 ? atoll(e) : SJ_DEFAULT_BATCH;

    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_sj_source *src = h_sj_source_open(in_fn, &chr, "sjtab");
    h_gtf anno; memset(&anno, 0, sizeof anno);
    if (gtf_fn) h_read_gtf(gtf_fn, &chr, &anno, 0);           /* tids against the header's names; -1 for any other sequence */
    FILE *out = stdout;
    if (out_fn && !(out = fopen(out_fn, "w"))) h_fatal("sjtab", "Can not open \"%s\" for writing\n", out_fn);
    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("sjtab", "%s", l2r_last_error());
    const l2r_sj_params prm = {min_intron, pair_only};
    const l2r_sj_genome gen = {g.n_seq, g.seq_off, g.bases};
    if (l2r_sj_begin_tab(ctx, &prm, have_genome ? &gen : NULL)) h_fatal("sjtab", "%s", l2r_last_error());
    h_sj_batch b; memset(&b, 0, sizeof b);
    int64_t no_nh = 0;
    while (h_sj_source_next(src, &b, batch_records) > 0) {
        for (int64_t i = 0; i < b.n; ++i) if (!(b.flag[i] & 4u) && (!pair_only || (b.flag[i] & 2u)) && !b.nh_seen[i]) ++no_nh;
        const l2r_sj_records recs = {b.n, b.n_cig, b.flag, b.tid, b.pos, b.uniq, b.cig_off, b.cig};
        if (l2r_sj_add(ctx, &recs)) h_fatal("sjtab", "%s", l2r_last_error());
    }
    h_sj_source_close(src); h_sj_batch_free(&b);
    int64_t n = 0;
    const int frc = l2r_sj_finish(ctx, &n);
    if (frc == L2R_SJ_E_UNKNOWN_TID) { fprintf(stderr, "%s\n", l2r_last_error()); l2r_destroy(ctx); exit(EXIT_FAILURE); }
    if (frc) h_fatal("sjtab", "%s", l2r_last_error());
    if (gtf_fn) {
        l2r_annotation a; memset(&a, 0, sizeof a);
        a.n_tx = anno.n_tx; a.n_exon = anno.n_ex; a.tx_tid = anno.tid; a.tx_start = anno.start; a.tx_end = anno.end; a.tx_rev = anno.rev;
        a.tx_ex_off = anno.ex_off; a.ex_start = anno.ex_start; a.ex_end = anno.ex_end;
        if (l2r_sj_annotate(ctx, &a)) h_fatal("sjtab", "%s", l2r_last_error());
    }
    const int64_t n_all = n;
    double st2[30]; memset(st2, 0, sizeof st2);
    if (!second) { if (l2r_sj_filter_rows(ctx, &flt, &n)) h_fatal("sjtab", "%s", l2r_last_error()); }
    else if (l2r_sj_filter_rows2(ctx, &flt, &flt2, &n) || l2r_sj_stats(ctx, st2, 30)) h_fatal("sjtab", "%s", l2r_last_error());
    int32_t *col[6]; uint8_t *byt[3];
    for (int q = 0; q < 6; ++q) col[q] = (int32_t *)h_malloc((size_t)(n + 1) * 4);
    for (int q = 0; q < 3; ++q) byt[q] = (uint8_t *)h_malloc((size_t)n + 1);
    l2r_sj_tab t = {n, 0, col[0], col[1], col[2], col[3], col[4], byt[0], byt[1], byt[2], col[5]};
    if (l2r_sj_download_tab(ctx, &t)) h_fatal("sjtab", "%s", l2r_last_error());
    l2r_destroy(ctx);
    for (int64_t i = 0; i < t.n; ++i) {
        if (col[0][i] < 0 || col[0][i] >= chr.n_hdr) h_fatal("sjtab", "junction on reference %d, the header has %d", col[0][i], chr.n_hdr);
        fprintf(out, "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", chr.name[col[0][i]], col[1][i], col[2][i], byt[0][i], byt[1][i], byt[2][i], col[3][i], col[4][i], col[5][i]);
    }
    if (out == stdout) fflush(stdout); else fclose(out);
    fprintf(stderr, "[sjtab] %lld junctions, %lld left by the filter; %lld records without an NH tag counted as multi-mapped\n", (long long)n_all, (long long)t.n,
            (long long)no_nh);
    if (second)
        fprintf(stderr, "[sjtab] %lld junctions dropped for their intron size, %lld for the distance to another junction\n", (long long)st2[29], (long long)st2[23]);
    for (int q = 0; q < 6; ++q) free(col[q]);
    for (int q = 0; q < 3; ++q) free(byt[q]);
    if (gtf_fn) h_gtf_free(&anno);
    h_chroms_free(&chr);
    if (have_genome) h_fasta_free(&g);
    return 0;
}
