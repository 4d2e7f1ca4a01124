/* fusion.c -- `lr2rmats fusion` (reference src/bam_fusion.c:144-212): reads whose two best alignment parts lie on different
 * chromosomes or far apart and together cover the read -- candidate gene-fusion transcripts; their two records as BAM on
 * stdout, with -f a table of the fusion sites.
 *
 *   records    SAM text, gzip / BGZF SAM or BAM -> BAM-encoded records in memory + the fields the tests read (filter.c)
 *   segments   the engine: l2r_fusion_segments()   (bam2seg, src/parse_bam.c:543-595)
 *   groups     runs of consecutive MAPPED records with one read name (an unmapped record is skipped in front of the name
 *              comparison, src/bam_fusion.c:176-194)
 *   choice     the engine: l2r_fusion_select()     (check_fusion :114-129)
 *   output     per candidate in file order the records of seg[0] and seg[1] -- the order of the reference's sort, not of the
 *              file; the site table without the line of the file's LAST group (:196-204 have no fusion_write)
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <stdlib.h>
#include <string.h>
#include "l2r_host.h"

#define OVLP_FRAC 0.1           /* src/bam_fusion.h:12-16 */
#define EACH_COV 0.1
#define ALL_COV 0.99
#define FUSION_DIS 100000
#define FUSION_DIS_STR "100k"

static int fusion_usage(void)
{
    /* src/bam_fusion.c:25-40 */
    fprintf(stderr, "\n");
    fprintf(stderr, "Usage:   %s fusion [option] <in.bam/sam> > fusion.sam\n", "lr2rmats");
    fprintf(stderr, "     or: %s fusion [option] <in.bam/sam> | bedtools bamtobed -i stdin -bed12 > fusion.bed\n\n", "lr2rmats");
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "         -o --ovlp-frac   [FLOAT]    maximum overlap fraction of each fusion part. [%.2f]\n", OVLP_FRAC);
    fprintf(stderr, "         -v --each-cov    [FLOAT]    minimum fraction of each fusion part. [%.2f]\n", EACH_COV);
    fprintf(stderr, "         -V --all-cov     [FLOAT]    minimum fraction of all mapped parts. [%.2f]\n", ALL_COV);
    fprintf(stderr, "         -d --dis         [INT]      minimum distance of two fusion parts. [%s]\n", FUSION_DIS_STR);
    fprintf(stderr, "         -f --fusion-site [STR]      output fusion site file. [NULL]\n");
    fprintf(stderr, "         -g --gtf         [STR]      gene annotation in GTF format. [None]\n");
    fprintf(stderr, "         -N --group-names            group the records by read name first (input that is not name-grouped). [false]\n");
    fprintf(stderr, "\n");
    /* (one line of our own: what the text above promises and the reference's option loop does not do) */
    fprintf(stderr, "Note:    -d and -g are listed above but not accepted (src/bam_fusion.c:148,153); gene names from -g are outside the MI355X build as well.\n\n");
    return 1;
}

static inline const char *rec_name(const h_records *r, int64_t i) { return (const char *)(r->buf + r->rec_off[i] + 4 + 32); }

int64_t h_fusion_groups(const h_records *r, const int32_t *qlen, int64_t *rows, int64_t *group_off, int32_t *rlen)
{
    return h_fusion_groups_in(r, qlen, NULL, rows, group_off, rlen);
}

int64_t h_fusion_groups_in(const h_records *r, const int32_t *qlen, const int64_t *order, int64_t *rows, int64_t *group_off, int32_t *rlen)
{
    int64_t m = 0, n_groups = 0;
    const char *last = NULL;
    for (int64_t at = 0; at < r->n; ++at) {
        const int64_t i = order ? order[at] : at;
        if (r->flag[i] & 4) continue;
        const char *name = rec_name(r, i);
        if (!last || strcmp(name, last) != 0) {
            int32_t ql;
            if (qlen) ql = qlen[i];
            else {
                uint32_t s = 0;                                      /* bam_query_len, src/parse_bam.c:261-270 */
                for (int64_t k = r->cig_off[i]; k < r->cig_off[i + 1]; ++k) if ((0x193u >> (r->cig[k] & 0xfu)) & 1u) s += r->cig[k] >> 4;
                ql = (int32_t)s;
            }
            rlen[n_groups] = ql;
            group_off[n_groups++] = m;
        }
        rows[m++] = i;
        last = name;
    }
    group_off[n_groups] = m;
    return n_groups;
}

int h_fusion_run(const char *in_fn, const l2r_fusion_params *prm, FILE *out, FILE *site, int64_t *n_pairs)
{
    return h_fusion_run_named(in_fn, prm, 0, out, site, n_pairs);
}

int h_fusion_run_named(const char *in_fn, const l2r_fusion_params *prm, int by_name, FILE *out, FILE *site, int64_t *n_pairs)
{
    h_chroms chr; memset(&chr, 0, sizeof chr);
    h_records r;
    h_stage_time("start");
    h_read_records(in_fn, &chr, &r, "bam_fusion");
    h_stage_time("read + encode records");
    if (site) fprintf(site, "#fusion_id\t1st_chr\t1st_strand\tst_start_site\t1st_end_site\t2nd_chr\t2nd_strand\t2nd_start_site\t2nd_end_site\n");      /* :173 */
    l2r_ctx *ctx = l2r_create(0);
    if (!ctx) h_fatal("bam_fusion", "%s", l2r_last_error());
    h_stage_time("engine: create");
    const size_t n1 = (size_t)r.n + 1;
    int32_t *col = (int32_t *)h_malloc(n1 * 4 * 5);
    int32_t *rs = col, *re = col + n1, *fs = col + 2 * n1, *fe = col + 3 * n1, *ql = col + 4 * n1;
    l2r_fusion_records fr = { r.n, r.n_cig, r.flag, r.tid, r.pos, r.l_qseq, r.nm, r.cig_off, r.cig };
    if (l2r_fusion_segments(ctx, &fr, rs, re, fs, fe, ql)) h_fatal("bam_fusion", "%s", l2r_last_error());
    h_stage_time("engine: segments (upload, kernel, download)");
    int64_t *rows = (int64_t *)h_malloc(n1 * 8), *goff = (int64_t *)h_malloc((n1 + 1) * 8);
    int32_t *rlen = (int32_t *)h_malloc(n1 * 4);
    int64_t *by = NULL;
    if (by_name) {                                                   /* -N: what `samtools sort -n` does in front of the reference's fusion */
        by = (int64_t *)h_malloc(n1 * 8);
        h_name_order(ctx, &r, by, "bam_fusion");
        h_records_set_grouped(&r, "bam_fusion");
        h_stage_time("engine: name order (upload, kernels, download)");
    }
    const int64_t n_groups = h_fusion_groups_in(&r, ql, by, rows, goff, rlen);
    free(by);
    const int64_t m = goff[n_groups];
    /* the columns of the rows (the mapped records) */
    int32_t *g = (int32_t *)h_malloc(((size_t)m + 1) * 4 * 7);
    int32_t *g_sc = g, *g_ed = g + m, *g_tid = g + 2 * m, *g_rs = g + 3 * m, *g_re = g + 4 * m, *g_fs = g + 5 * m, *g_fe = g + 6 * m;
    for (int64_t k = 0; k < m; ++k) {
        const int64_t i = rows[k];
        g_sc[k] = r.as_score[i]; g_ed[k] = r.nm[i]; g_tid[k] = r.tid[i]; g_rs[k] = rs[i]; g_re[k] = re[i]; g_fs[k] = fs[i]; g_fe[k] = fe[i];
    }
    h_stage_time("groups of one read name");
    int64_t *first = (int64_t *)h_malloc(((size_t)n_groups + 1) * 8), *second = (int64_t *)h_malloc(((size_t)n_groups + 1) * 8);
    if (l2r_fusion_select(ctx, n_groups, goff, g_sc, g_ed, g_tid, g_rs, g_re, g_fs, g_fe, rlen, prm, first, second)) h_fatal("bam_fusion", "%s", l2r_last_error());
    h_stage_time("engine: select (upload, kernel, download)");
    l2r_destroy(ctx);
    int64_t *keep = (int64_t *)h_malloc(((size_t)n_groups + 1) * 16);
    int64_t cnt = 0;
    for (int64_t gi = 0; gi < n_groups; ++gi) {
        if (first[gi] < 0 || second[gi] < 0) continue;
        const int64_t a = rows[first[gi]], b = rows[second[gi]];
        const char *name = rec_name(&r, a);
        if (!name[0]) continue;                                      /* strcmp(lqname, "\0") != 0, :181,:196 */
        keep[2 * cnt] = a; keep[2 * cnt + 1] = b; ++cnt;
        if (site && gi != n_groups - 1) {                            /* fusion_write :132-142; the last group of the file gets none */
            const int64_t l = rs[a] < rs[b] ? a : b, rr = rs[a] < rs[b] ? b : a;
            const char *cl = r.tid[l] >= 0 && r.tid[l] < chr.n ? chr.name[r.tid[l]] : "*", *cr = r.tid[rr] >= 0 && r.tid[rr] < chr.n ? chr.name[r.tid[rr]] : "*";
            fprintf(site, "%s\t%s\t%c\t%d\t%d\t%s\t%c\t%d\t%d\n", name, cl, "+-"[(r.flag[l] >> 4) & 1], fs[l], fe[l], cr, "+-"[(r.flag[rr] >> 4) & 1], fs[rr], fe[rr]);
        }
    }
    if (h_write_bam(out, &r, keep, 2 * cnt)) h_fatal("bam_fusion", "Error in writing SAM record\n");
    h_stage_time("write BAM (BGZF)");
    if (n_pairs) *n_pairs = cnt;
    free(col); free(rows); free(goff); free(rlen); free(g); free(first); free(second); free(keep);
    h_records_free(&r); h_chroms_free(&chr);
    return 0;
}

int h_cmd_fusion(int argc, char **argv)
{
    /* src/bam_fusion.c:42-49,148-159: --fusion-site and --gtf are not in the table, and `-d` / `--dis` reach a switch that tests 's' */
    static const struct option long_opt[] = {
        { "ovlp-frac", 1, NULL, 'o' }, { "each-cov", 1, NULL, 'v' }, { "all-cov", 1, NULL, 'V' }, { "dis", 1, NULL, 'd' }, { "group-names", 0, NULL, 'N' }, { 0, 0, 0, 0 }
    };
    l2r_fusion_params prm = { (float)OVLP_FRAC, (float)EACH_COV, (float)ALL_COV, FUSION_DIS };
    FILE *site = NULL;
    int c, by_name = 0;
    optind = 1;
    while ((c = getopt_long(argc, argv, "o:v:V:d:f:N", long_opt, NULL)) >= 0) {
        switch (c) {
        case 'N': by_name = 1; break;
        case 'o': prm.ovlp_frac = (float)atof(optarg); break;
        case 'v': prm.each_cov = (float)atof(optarg); break;
        case 'V': prm.all_cov = (float)atof(optarg); break;
        case 'f':
            if (site) fclose(site);
            site = fopen(optarg, "w");                               /* opened where the option is parsed (xopen) */
            if (!site) h_fatal("bam_fusion", "fail to open file '%s'", optarg);
            break;
        default: if (site) fclose(site); return fusion_usage();
        }
    }
    if (argc - optind != 1) { if (site) fclose(site); return fusion_usage(); }
    int64_t cnt = 0;
    const int rc = h_fusion_run_named(argv[optind], &prm, by_name, stdout, site, &cnt);
    fprintf(stderr, "[%s] Candidate gene-fusion transcripts: %d\n", "bam_fusion", (int)cnt);
    if (site && fclose(site) != 0) return 1;
    return rc;
}
