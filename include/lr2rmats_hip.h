/* lr2rmats_hip.h -- C-ABI of the MI355X (gfx950) read-vs-annotation engine.
 *
 * This is the drop-in boundary for the one hot path of lr2rmats `update-gtf`
 * (and the CIGAR half of `bam2gtf` / `unique-gtf`): everything between
 * "alignment records and annotation are in memory" and "every read carries its
 * exons, class, flags and reference transcript".  In the reference that seam is
 *
 *     read_bam_trans()   src/bam2gtf.c:89-110   (gen_exon :31-78 per record)
 *     check_trans()      src/update_gtf.c:936-965
 *         check_with_anno_trans()  :792-835   check_full() :629-681
 *         check_splice_site()      :717-779   set_full()   :683-696
 *         check_with_short_sj()    :698-709   check_short_sj{,1}() :589-627
 *
 * called from update_gtf() src/update_gtf.c:1069 and :1083.  The list routing,
 * split_trans(), merge_trans() and the writers stay on the host (they are
 * order dependent); they consume the arrays this library returns.
 *
 * Plain C types only: caller-owned host buffers, sizes, int return codes
 * (0 = ok, negative = error, text from l2r_last_error()).  One context drives
 * one GPU (one process per GPU); all device work of a context is issued on the
 * context's own HIP stream.  There is no CPU fallback: l2r_create() fails when
 * no gfx950 device is usable.
 */
#ifndef LR2RMATS_HIP_H
#define LR2RMATS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2R_ABI_VERSION 3

typedef struct l2r_ctx l2r_ctx;

/* The fields of update_gtf_para (src/update_gtf.h:8-15) that the path reads;
 * defaults in src/update_gtf.c:24-35 and src/gtf.h:118-127. */
typedef struct {
    int32_t min_exon;               /* -e  INTER_EXON_MIN_LEN 3  */
    int32_t min_intron;             /* -i  INTRON_MIN_LEN 3      */
    int32_t max_delet;              /* -t  DELETION_MAX_LEN 50   */
    int32_t ss_dis;                 /* -d  SPLICE_DISTANCE 0     */
    int32_t end_dis;                /* -D  END_DISTANCE 0x7fffffff (host merge only) */
    int32_t full_level;             /* -l  1..5, default 5       */
    int32_t split_trans;            /* -s  */
    int32_t use_multi;              /* -M  */
    int32_t min_sj_cnt;             /* -J  MIN_SJ_CNT 1          */
    int32_t force_strand;           /* -c  (host merge only)     */
    float   single_exon_ovlp_frac;  /* -f  SING_OVLP_FRAC 0.80   */
} l2r_params;

/* Annotation transcripts in GTF FILE ORDER, as read_anno_trans() leaves them
 * (src/gtf.c:468-521): exons of a transcript sorted by (start,end), tx_start =
 * first exon start, tx_end = end of the LAST exon in that order, tid = index in
 * the BAM header or -1.  1-based closed coordinates. */
typedef struct {
    int64_t n_tx, n_exon;
    const int32_t *tx_tid, *tx_start, *tx_end;
    const uint8_t *tx_rev;
    const int64_t *tx_ex_off;       /* n_tx + 1 */
    const int32_t *ex_start, *ex_end;
} l2r_annotation;

/* STAR SJ.out.tab rows as read_sj_group() leaves them (src/gtf.c:431-449):
 * sorted by (tid, don, acc); don/acc = first/last intron base. */
typedef struct {
    int64_t n;
    const int32_t *tid, *don, *acc, *uniq_c, *multi_c;
} l2r_junctions;

/* Alignment records in input order: what gen_exon() reads from a bam1_t
 * (src/bam2gtf.c:34-41): core.tid, core.pos (0-based), the strand resolved as
 * "XS aux present ? (XS:A == '+' ? 0 : 1) : FLAG & 16", and the raw CIGAR words
 * (len << 4 | op).  Unmapped records must be rejected by the caller (the
 * reference aborts on them in update-gtf, skips them in bam2gtf). */
typedef struct {
    int64_t n_reads, n_cigar;
    const int32_t *tid, *pos;
    const uint8_t *rev;
    const int64_t *cig_off;         /* n_reads + 1 */
    const uint32_t *cig;
    int64_t first_read_index;       /* global index of record 0 (read shards of a multi-GPU run) */
    /* Optional (NULL: the engine walks every CIGAR once at upload to make it, k_tile_index): what a reader knows of a record's CIGAR
     * while it converts it (host/aln_reader.c does for every input format; lr2rmats_amd/synth.py for synthetic reads), whatever the
     * thresholds of a run -- three words per record:
     *   [0] reference bases of the CIGAR (ops M D N = X): the record ends at pos + [0] (src/bam2gtf.c:41-74: `end` only grows by these);
     *   [1] N operations | the shortest of them << 16;     [2] the longest D operation | the shortest stretch of reference bases
     *       between two N operations << 16 -- each of the four saturated at 65535 (the shortest ones 65535 where there is none).
     * With it a run knows a tile's exon count without a CIGAR walk wherever no threshold is borderline (exons = records + N operations
     * while -i <= shortest N, -t >= longest D, -e <= shortest stretch), and the upload's index is a scan over 15 bytes per record. */
    const uint32_t *cig_summary;
} l2r_reads;

/* bits of info[] : one word per read; bits 8..31 = exon count */
#define L2R_INFO_KNOWN      0x01u   /* trans_t.known                       */
#define L2R_INFO_KNOWN_SITE 0x02u   /* trans_t.has_known_site              */
#define L2R_INFO_FULL       0x04u   /* trans_t.full                        */
#define L2R_INFO_REV        0x08u   /* is_rev after update_gtf.c:825-831   */
#define L2R_INFO_UNREL      0x10u   /* has_unreliable_junction             */
#define L2R_INFO_SJ_CHECKED 0x20u   /* check_with_short_sj() was reached   */
#define L2R_INFO_SJ_PASS    0x40u   /* ... and returned 1                  */
#define L2R_INFO_ACCEPTED   0x80u   /* goes to novel_T / updated_T (whole or, with -s, as split pieces) */
#define L2R_INFO_NEXON(i)   ((i) >> 8)

/* bits of ex_flag[] : one byte per exon j; junction j (exon j -> j+1) lives with exon j */
#define L2R_EXF_NOVEL_EXON  0x01u   /* novel_exon_flag[j]          */
#define L2R_EXF_NOVEL_DON   0x02u   /* novel_site_flag[2j]         */
#define L2R_EXF_NOVEL_ACC   0x04u   /* novel_site_flag[2j+1]       */
#define L2R_EXF_NOVEL_JUNC  0x08u   /* novel_junction_flag[j]      */
#define L2R_EXF_UNREL_JUNC  0x10u   /* unreliable_junction_flag[j] */

/* Per-read results in read order (what check_trans() leaves in bam_T). */
typedef struct {
    int64_t n_reads;                /* in: capacity of the per-read arrays; out: reads written  */
    int64_t ex_cap;                 /* in: capacity of the per-exon arrays                       */
    int64_t n_exons;                /* out */
    int64_t *ex_off;                /* n_reads + 1 */
    int32_t *ex_start, *ex_end;
    uint8_t *ex_flag;
    uint32_t *info;
    int32_t *ref_tx;                /* ref_anno_i or -1 */
} l2r_result;

/* Accepted-novel records, compacted in read order: the reads check_trans()
 * hands to novel_T/merge_trans (update_gtf.c:946-960).  This is the message of
 * the multi-GPU all-gatherv. */
typedef struct {
    uint32_t read_lo, read_hi;      /* global read index (64 bit, split) */
    uint32_t info;
    int32_t  ref_tx;
} l2r_accepted_read;                /* 16 bytes */

typedef struct {
    int64_t n_reads, ex_cap;        /* in: capacities; out n_reads = records written */
    int64_t n_exons;                /* out */
    l2r_accepted_read *rec;
    int64_t *ex_off;                /* n_reads + 1, into the arrays below */
    int32_t *ex_start, *ex_end;
    uint8_t *ex_flag;
} l2r_accepted;

/* Raw device views (for a caller that keeps data in HBM: bench, RCCL gather). */
typedef struct {
    int64_t n_reads, n_exons, n_accepted, n_accepted_exons;
    const uint32_t *ex_off;         /* device, n_reads (exclusive offsets) */
    const int32_t *ex_start, *ex_end;
    const uint8_t *ex_flag;
    const uint32_t *info;
    const int32_t *ref_tx;
    /* Accepted list in HBM.  acc_rec / acc_ex_off: one entry per accepted read; record i has info >> 8 exons starting
     * at acc_ex_off[i] in the three exon arrays.  All five arrays are dense (n_accepted / n_accepted_exons entries, no
     * gaps) but made of one CHUNK PER TILE of reads: inside a chunk the reads are in read order, the chunks follow each
     * other in the order the kernels handed them out.  A consumer that needs read order sorts by the 64-bit read index
     * of the records (l2r_download_accepted() does, and lays the exons out record by record); always address the exon
     * arrays through acc_ex_off. */
    const l2r_accepted_read *acc_rec;
    const uint32_t *acc_ex_off;     /* device, n_accepted */
    const int32_t *acc_ex_start, *acc_ex_end;
    const uint8_t *acc_ex_flag;
} l2r_device_view;

/* Average device time per kernel of the last l2r_run_timed(), milliseconds.  Stages 0..2 are the three kernels of the
 * pipeline the engine chose for the uploaded records (l2r_stage_kernel() names them):
 *     slab    (coordinate-sorted records; default)  0 k_walk_slab (the tile's reads by CIGAR length, CIGAR -> exons; long CIGARs:
 *             k_walk_slab_long, one wave per read as a scan over the op stream,
 *             read-order places)  1 k_describe_scan (the tiles' descriptors and windows, one wave per tile; the tiles' exon counts -> their
 *             first result slots; the tile lists of the wide / chunked kernels)  2 k_probe_slab
 *             (annotation window, site probes, verdicts, read-order results) + k_probe_slab_wide (tiles whose window holds 33 .. 63
 *             transcripts) + k_probe_slab_chunked (tiles beyond that, or with a dictionary key in several entries: the window 63
 *             members at a time).  Every run launches all of them: nothing is kept from an earlier run of the same records.
 *     tile    (coordinate-sorted records with short CIGARs, -e >= 1, an upload that carries the tile index -- i.e. not a single-run one,
 *             l2r_hint_single_run / l2r_classify; default where it applies)  0 k_describe_scan (the tiles' descriptors
 *             and windows from the spans the upload recorded; first kernel of the run)  1 k_tile (CIGAR -> exons, window, probes, verdicts,
 *             junction check, read-order results: one workgroup per tile, nothing handed over through HBM)  2 k_probe_slab for the few
 *             tiles k_tile left in slab form + k_tile's WIDE instance (windows of 33 .. 63 transcripts) + k_tile_chunk (windows beyond that) -- both launched beside
 *             k_tile on streams of their own, so with per-stage events they count here and in stage 1 one behind the other -- + k_probe_slab_wide + k_probe_slab_chunked
 *             (each not launched once a run has shown its list empty)
 *     classic (unsorted records, long CIGARs with -e < 1, L2R_PIPELINE=classic)  0 k_pass_a  1 k_scan_u32 (tile sums)  2 k_classify_fast */
#define L2R_N_STAGES 8
typedef struct {
    float stage_ms[L2R_N_STAGES];   /* 0..2 see above  3 classify_generic (redo list) 4 validate_junctions (+ recount)
                                       5 scan of accepted counts 6 gather_accepted (records; exons of the tiles
                                       the classification did not compact itself) 7 reserved */
    float total_ms;                 /* first launch -> last completion, per iteration */
    int32_t iters;
} l2r_timing;

int          l2r_abi_version(void);
const char  *l2r_last_error(void);
int          l2r_device_count(void);

l2r_ctx     *l2r_create(int device);
void         l2r_destroy(l2r_ctx *ctx);

int          l2r_set_params(l2r_ctx *ctx, const l2r_params *prm);
/* Which outputs a run produces (default: both).  L2R_WANT_RESULTS = the per-read arrays of l2r_result (what
 * check_trans() leaves in bam_T: detail.txt, -a/-k/-u, summary.txt need them); L2R_WANT_ACCEPTED = the compacted
 * accepted-novel records of l2r_accepted (what check_trans() hands to novel_T / merge_trans, update_gtf.c:946-960:
 * all that `update-gtf ... > new.gtf`, -v and -E need; the message of the multi-GPU all-gatherv). */
#define L2R_WANT_RESULTS  1u
#define L2R_WANT_ACCEPTED 2u
int          l2r_set_outputs(l2r_ctx *ctx, unsigned want);
int          l2r_set_annotation(l2r_ctx *ctx, const l2r_annotation *anno);
/* The tables l2r_set_annotation derives from the annotation (transcript headers, cursor keys, the two site dictionaries and
 * their bucket directories: two sorts of ~1.5 M rows each and the dictionary build for a GENCODE-size GTF) can be kept
 * on disk between runs: `dir` (or the environment variable L2R_ANNO_CACHE when no call is made; NULL / "" = off, the
 * default) holds one file per annotation, named by a hash of the arrays passed in.  A hit replaces the build by one
 * read; a file that does not match in any respect is ignored and rewritten.  l2r_annotation_cache_state(): what the last
 * l2r_set_annotation did -- 0 no cache, 1 built and stored, 2 read from the cache.  (The reference re-reads and re-sorts
 * the GTF on every invocation, src/gtf.c:468-521; the pipeline calls update-gtf twice per sample on one GTF.) */
int          l2r_set_annotation_cache(l2r_ctx *ctx, const char *dir);
int          l2r_annotation_cache_state(l2r_ctx *ctx);
int          l2r_set_junctions(l2r_ctx *ctx, const l2r_junctions *sj);   /* NULL or n == 0: no -j file */

/* host -> HBM; detects whether the records are coordinate sorted and, if not,
 * prepares the history-dependent cursor values on the host. */
int          l2r_upload_reads(l2r_ctx *ctx, const l2r_reads *reads);
/* GPU time of the last upload's tile index (k_tile_index; 0 where the upload made none), by HIP events on the context stream: the part of
 * an upload that is kernel work on the records -- bench.py adds it to a first run for the cost of ONE classification of fresh input. */
float        l2r_upload_index_ms(l2r_ctx *ctx);
/* on != 0: every following upload will be classified ONCE (what the CLI does: one l2r_run per l2r_upload_reads).  Such an upload makes
 * no tile index and its run takes the two-kernel pipeline -- by total GPU time the cheaper way for a single run (l2r_classify does the
 * same by itself); the one-kernel tile path is for uploads that are run again (parameter sweeps, the benchmark's resident steps). */
int          l2r_hint_single_run(l2r_ctx *ctx, int on);

/* The hot path on resident inputs; asynchronous on the context stream. */
int          l2r_run(l2r_ctx *ctx);          /* one pass of the path over the resident upload; results in read order in HBM.  (Launches that a
                                              * completed run of the same upload and parameters has shown to be empty -- list kernels, the generic
                                              * kernel -- are dropped from later runs; the one-kernel tile path reads the index the upload made.) */
int          l2r_sync(l2r_ctx *ctx);
/* `iters` back-to-back runs bracketed by HIP events on the context stream. */
int          l2r_run_timed(l2r_ctx *ctx, int iters, l2r_timing *out);
const char  *l2r_stage_kernel(l2r_ctx *ctx, int stage);                 /* kernel behind stage_ms[stage] ("" = none) */

int          l2r_result_sizes(l2r_ctx *ctx, int64_t *n_reads, int64_t *n_exons,
                              int64_t *n_accepted, int64_t *n_accepted_exons);
int          l2r_download(l2r_ctx *ctx, l2r_result *res);               /* HBM -> host */
int          l2r_download_accepted(l2r_ctx *ctx, l2r_accepted *acc);
int          l2r_device_view_get(l2r_ctx *ctx, l2r_device_view *view);
void        *l2r_stream(l2r_ctx *ctx);                                  /* hipStream_t */

/* ---- several GPUs of one node, one process (rank) per GPU: the gathered route's exchange over RCCL (xGMI).
 * Inputs that cannot be cut into independent shards (-s with a junction table: split pieces are compared across chromosomes,
 * src/update_gtf.c:837-913,946-960) are classified shard by shard and their per-read results gathered on rank 0, which runs the
 * order-dependent tail once over the whole read-order set.  Rank 0 makes the id (l2r_xchg_unique_id: l2r_xchg_id_bytes() bytes) and
 * the caller carries it to the other ranks; every rank then creates its end (collective) and, behind l2r_run + l2r_sync, calls
 * l2r_xchg_gather_results (collective): `res` (rank 0 only; capacities as for l2r_download, for the reads / exons of ALL ranks)
 * receives the results of every rank as one set with global exon offsets; counts_out (may be NULL) gets {reads, exons} per rank.
 * l2r_xchg_gather_accepted (collective; L2R_WANT_ACCEPTED): the accepted-novel records alone -- SURVEY 8(e)'s all-gatherv message -- of
 * every rank to rank 0 in read order (`acc`, rank 0 only, capacities for all ranks; read indices are the global ones the uploads'
 * first_read_index gave): all the order-dependent merge needs when no output wants every read; 16 + 9 n bytes per accepted read. */
typedef struct l2r_xchg l2r_xchg;
int          l2r_xchg_id_bytes(void);
int          l2r_xchg_unique_id(void *id_out);
l2r_xchg    *l2r_xchg_create(l2r_ctx *ctx, int rank, int world, const void *id);
int          l2r_xchg_gather_results(l2r_xchg *x, l2r_result *res, int64_t *counts_out);
int          l2r_xchg_gather_accepted(l2r_xchg *x, l2r_accepted *acc, int64_t *counts_out);
void         l2r_xchg_destroy(l2r_xchg *x);

/* ---- diagnostics (tools/, bench.py and the tests read them; no product path does).
 * l2r_debug_counters: out[0] reads the last run left to the generic kernel (the redo list), [1] dictionary entries whose key has
 *   several entries, [2] annotation transcripts the mask kernels take, [3] tiles, [4..11] tiles by the reason their descriptor
 *   is not on the 32-bit masks (0 = it is), [12] tiles of the 64-bit-mask kernel, [13] runs that l2r_sync did again on the slab pipeline
 *   because a tile of k_tile had waited in vain for the exon counts in front of it, [14] entries of the chunked kernel's list that k_tile_chunk
 *   declined in the last run (its staging caps), [15] tiles handed to the chunked kernel late (a key in several entries); the last run's
 *   tile descriptors (slab / tile pipeline; classic: 24 and 25 only): [16..20] tiles of the chunked kernels by the END entries of their
 *   dictionary slices (<= 256, <= 512, <= 768, <= 1024, more), [21] / [22] ... with more than 128 / 256 START entries, [23] all of
 *   them, [24] / [25] the largest START / END slice of any tile, [26] tiles k_tile_chunk took from their CIGARs (TD_CDIRECT),
 *   [27] tiles k_describe_scan marked for k_tile's EXACT instance, which took them whole (TD_XDIRECT; tile pipeline), [28] entries of
 *   the rest list the last run's k_describe_scan made: the tiles k_tile's general instance ran over beside the EXACT one ([27] + [28]
 *   = [3]; both 0 with L2R_TILE_SPLIT=0, where the general instance takes every tile);
 *   n = words of out (4, 12, 13, 14, 16, 24, 27 or 29).
 * l2r_debug_stamps: with L2R_STAMPS=1 in the environment at l2r_create, per-phase cycle sums of the classification kernel
 *   (and clears them); zeros otherwise.
 * l2r_debug_tile_times: with L2R_STAMPS=1, one-kernel tile path: four words per tile -- the chip's 100 MHz clock at the tile's start
 *   << 3 | its XCD, at the publication of its exon count, at the begin and the end of its wait for the counts in front. */
int          l2r_debug_counters(l2r_ctx *ctx, long long *out, int n);
int          l2r_debug_stamps(l2r_ctx *ctx, unsigned long long *out, int n);
int          l2r_debug_tile_times(l2r_ctx *ctx, uint32_t *out, int64_t n_tiles);

/* upload + run + sync + download in one call (the host CLI uses this). */
int          l2r_classify(l2r_ctx *ctx, const l2r_reads *reads, l2r_result *res);

/* ---- `filter` (src/bam_filter.c): the per-record test + score and the per-read choice of the best alignment.
 * Replaces gtf_filter() :61-86 with remove_overlap() :48-59, and the selection loop of bam_filter() :128-154; reading the
 * records and writing the BAM stay with the caller (host/filter.c). */
typedef struct { float cov_rate, map_qual, sec_rat; int32_t min_intron_n; } l2r_filter_params;   /* -v 0.67  -q 0.75  -s 0.98  -i 0 */
typedef struct {
    int64_t n, n_cigar;
    const uint16_t *flag;           /* FLAG */
    const int32_t *tid, *pos;       /* core.tid, core.pos (0-based) */
    const int32_t *l_qseq;          /* core.l_qseq */
    const int32_t *nm;              /* bam_aux2i() of the NM tag: its value for the integer types, 0 for any other type */
    const int64_t *cig_off;         /* n + 1 */
    const uint32_t *cig;            /* len << 4 | op */
} l2r_filter_records;
/* transcripts of the -r GTF in FILE order, as read_anno_trans() leaves them (tid -1: chromosome not in the header; the reference
 * compares tids as numbers, so a mapped record of tid -1 meets such a transcript where it lies in front of the first tid >= 0) */
typedef struct { int64_t n; const int32_t *tid, *start, *end; } l2r_filter_spans;
/* drop[i] = gtf_filter() != 0; score[i] / intron_n[i] = its two outputs (score 0 for dropped records) */
int          l2r_filter_score(l2r_ctx *ctx, const l2r_filter_records *recs, const l2r_filter_params *prm,
                              const l2r_filter_spans *remove /* NULL: no -r */, uint8_t *drop, int32_t *score, int32_t *intron_n);
/* Groups = runs of consecutive KEPT records with one read name (the dropped ones are invisible to bam_filter()'s loop);
 * group g covers rows [group_off[g], group_off[g+1]) of score / intron_n (the kept records, in input order).
 * winner[g] = row of the alignment that is written, or -1 when the read is not retained. */
int          l2r_filter_select(l2r_ctx *ctx, int64_t n_groups, const int64_t *group_off, const int32_t *score,
                               const int32_t *intron_n, const l2r_filter_params *prm, int64_t *winner);

/* ---- `fusion` (src/bam_fusion.c): per alignment record the part of the read and of the reference it covers, per read the two
 * parts of a candidate gene fusion.  Replaces bam2seg() (src/parse_bam.c:543-595) with bam_query_len() (:261-270), and
 * check_fusion() (src/bam_fusion.c:114-129) with its comparator and tests; reading the records, the AS / NM tags, the grouping
 * by read name and the writers stay with the caller (host/fusion.c). */
typedef struct { float ovlp_frac, each_cov, all_cov; int32_t dis; } l2r_fusion_params;            /* -o 0.1  -v 0.1  -V 0.99  dis 100000 */
typedef l2r_filter_records l2r_fusion_records;                  /* the same columns; flag, pos, cig_off and cig are read */
/* Row i: read_start / read_end (1-based on the read as sequenced, first clip counted, swapped round on the reverse strand),
 * ref_start / ref_end (1-based), qlen (bam_query_len: M I S = X).  The rows of unmapped records (FLAG & 4) are 0.  32-bit sums
 * that wrap.  The kernel has a form of one thread and a form of one wave per record; the engine takes the second where the
 * records have more than 32 operations on average (L2R_FUSION_WAVE=0|1 in the environment forces one). */
int          l2r_fusion_segments(l2r_ctx *ctx, const l2r_fusion_records *recs, int32_t *read_start, int32_t *read_end,
                                 int32_t *ref_start, int32_t *ref_end, int32_t *qlen);
/* Groups = runs of consecutive MAPPED records with one read name; group g covers rows [group_off[g], group_off[g+1]) of the
 * seven columns (score = bam_aux2i(AS), ed = bam_aux2i(NM), 0 without the tag); rlen_of_group[g] = qlen of the group's first
 * record.  first[g] / second[g] = rows of the two segments check_fusion() leaves in seg[0] / seg[1] when it returns 2, else
 * -1 / -1.  Equal (score, ed): the earlier row first; scores compared by value; the coverage counts positions of [1, rlen]
 * only; rlen <= 0 or a group of one row: not a candidate. */
int          l2r_fusion_select(l2r_ctx *ctx, int64_t n_groups, const int64_t *group_off, const int32_t *score, const int32_t *ed,
                               const int32_t *tid, const int32_t *read_start, const int32_t *read_end, const int32_t *ref_start,
                               const int32_t *ref_end, const int32_t *rlen_of_group, const l2r_fusion_params *prm,
                               int64_t *first, int64_t *second);
/* diagnostics (tools/bench_fusion.py, tests): out[0] the form the last l2r_fusion_segments took (0 thread, 1 wave per record);
 * with L2R_FUSION_TIMING=1 in the environment (every one of these launches is then waited for) device milliseconds of the last
 * [1] k_fusion_seg [2] k_fusion_select [3] k_filter_score [4] k_filter_select; n = words of out (up to 5) */
int          l2r_fusion_stats(l2r_ctx *ctx, double *out, int n);

/* ---- `bam2sj` (src/parse_bam.c:896-924 bam2sj_core): the junction table of an alignment file -- one row per distinct
 * (tid, don, acc) in that order, with how many uniquely / multiply mapped records carry it, its intron motif and strand.
 * Replaces gen_sj() :402-442 per record, the list search and insertion of sj_sch_group() / sj_update_group() :339-380 (a device
 * radix sort + a segmented sum: the list of the reference equals that order wherever the records' tids never decrease) and
 * intr_deri_str() :319-337.  Reading the records and the FASTA and printing the table stay with the caller (host/sj.c).
 * A short-read file does not fit one upload, so the records come in batches:
 *     l2r_sj_begin  once: parameters, the genome (NULL: no -g; motif and strand are 0 then) -- copied to HBM as bytes
 *     l2r_sj_add    a batch of records, any number of times: record filter (FLAG & 4 skipped; pair_only: without FLAG & 2 skipped),
 *                   CIGAR walk (an N of at least min_intron bases is a row {tid, don = first, acc = last intron base, uniq, 1 - uniq}),
 *                   rows appended in record order; the rows so far are sorted and reduced whenever they exceed a bound
 *     l2r_sj_add_rows  rows that are counted already (a table made earlier, or another file's): the count COLUMNS are summed,
 *                   so tables merge by the same sort + reduce
 *     l2r_sj_finish sorts and reduces all rows, looks up the motifs; *n_rows = rows of the table.  A row on a sequence the genome
 *                   does not have (tid >= n_seq): L2R_SJ_E_UNKNOWN_TID, l2r_last_error() names the tid (the reference: err_fatal)
 *     l2r_sj_download  the table; its first five columns have the layout of l2r_junctions (l2r_set_junctions takes them as they are)
 * The result does not depend on how the records were cut into batches.  The sort is stable and the rows are made in record
 * order, so every intermediate order is the same run after run. */
#define L2R_SJ_SORT_TILE 4096           /* rows one workgroup of a radix pass ranks (csrc/l2r_radix.hip.h holds both to its one tile) */
#define L2R_SJ_E_UNKNOWN_TID (-3)
typedef struct { int32_t min_intron, pair_only; } l2r_sj_params;         /* -i INTRON_MIN_LEN 3; read_type PAIR_T: 1 */
typedef struct { int32_t n_seq; const int64_t *seq_off /* n_seq + 1 */; const uint8_t *bases; } l2r_sj_genome;   /* sequences in FILE order */
typedef struct {
    int64_t n, n_cigar;
    const uint16_t *flag;
    const int32_t *tid, *pos;           /* core.tid, core.pos (0-based) */
    const uint8_t *uniq;                /* NH tag present and bam_aux2i(NH) == 1 */
    const int64_t *cig_off;             /* n + 1 */
    const uint32_t *cig;                /* len << 4 | op */
} l2r_sj_records;
typedef struct { int64_t cap, n; int32_t *tid, *don, *acc, *uniq_c, *multi_c; uint8_t *strand, *motif; } l2r_sj_table;   /* in: cap; out: n */
int          l2r_sj_begin(l2r_ctx *ctx, const l2r_sj_params *prm, const l2r_sj_genome *genome);
int          l2r_sj_add(l2r_ctx *ctx, const l2r_sj_records *recs);
int          l2r_sj_add_rows(l2r_ctx *ctx, const l2r_junctions *rows);
int          l2r_sj_finish(l2r_ctx *ctx, int64_t *n_rows);
int          l2r_sj_download(l2r_ctx *ctx, l2r_sj_table *table);
/* diagnostics (tools/bench_sj.py, tests): out[0] rows made by l2r_sj_add / _add_rows since l2r_sj_begin, [1] sort + reduce rounds,
 * [2] radix passes the last round ran (of 12), [3] rows that went into it, [4] rows it left; with L2R_SJ_TIMING=1 in the environment
 * at l2r_sj_begin (every launch is then waited for), device milliseconds summed since then: [5] k_sj_count [6] k_scan_u32 of the
 * counts [7] k_sj_fill [8] k_sj_hist12 [9] k_radix_digit_hist<SjRows> [10] k_scan_u32 of the tile histograms [11] k_radix_scatter<SjRows> [12] k_sj_heads +
 * its scan [13] k_sj_reduce [14] k_sj_motif; n = words of out (up to 15 for `bam2sj`; `sjtab` below adds words from 15 on) */
int          l2r_sj_stats(l2r_ctx *ctx, double *out, int n);

/* ---- `sjtab` (host/sj.c): the junction table in the form `update-gtf -j` reads (STAR's SJ.out.tab: ..., annotated, unique count,
 * multi count, maximum overhang), filtered as STAR's outSJfilter* options do.  The table of `bam2sj` with a sixth column:
 *   overhang  the junction operations (N of at least min_intron bases) cut a record's CIGAR into blocks; a block's length is the
 *             sum of its M = X lengths (I D S H P B and a shorter N add nothing and cut nothing); a record's overhang at a junction
 *             is the shorter of the blocks on its two sides (0 where the N is the first or the last operation); a row's max_over is
 *             the maximum over its records.  The reference has no such rule (src/parse_bam.c:415 stops at the comment).
 *     l2r_sj_begin_tab   as l2r_sj_begin, with the overhang tracked: l2r_sj_add and l2r_sj_finish carry the column, l2r_sj_add_rows
 *                   gives its rows overhang 0
 *     l2r_sj_add_rows_over  rows of tables that carry the column: counts summed, max_over (n words, none negative) by maximum
 *     l2r_sj_annotate    behind l2r_sj_finish: anno = 1 for every row that is an intron of the annotation -- the interval between two
 *                   consecutive exons of a transcript (exons ascending inside a transcript, as l2r_set_annotation takes them;
 *                   transcripts with tid -1 skipped; abutting or overlapping exons give none).  Never called: anno is 0 everywhere
 *     l2r_sj_filter_rows behind l2r_sj_finish (and l2r_sj_annotate where that is used): a row of category c -- annotated 0; else
 *                   motif 0: 1, motif 1 2: 2, motif 3 4: 3, motif 5 6: 4 -- stays when
 *                   max_over >= anchor_min[c] && (uniq_c >= uniq_min[c] || uniq_c + multi_c >= all_min[c]); order kept; *n_rows = rows left
 *     l2r_sj_download_tab  the nine columns
 * On a table begun with l2r_sj_begin, or in front of l2r_sj_finish, each of these returns an error (l2r_last_error() says which).
 * l2r_sj_stats from word 15: [15] rows the last l2r_sj_filter_rows dropped, [16] distinct annotation introns; with L2R_SJ_TIMING=1
 * device milliseconds of [17] k_sj_introns [18] k_sj_annotate [19] k_sj_keep [20] k_scan_u32 of the keep flags [21] k_sj_take
 * [22] the sort + reduce of the introns (all its kernels).
 *
 * l2r_sj_filter_rows2: l2r_sj_filter_rows and, after STAR's outSJfilterIntronMaxVsReadN and outSJfilterDistToOtherSJmin, two more rules
 * (the project's own definition: no byte equality with a STAR release is claimed).  Categories as above; a motif above 6 counts as 0.
 *   stage 1, row-local   the test of l2r_sj_filter_rows, and the intron-size rule: with reads = max(1, uniq_c + multi_c), a row of
 *             category 1..4 with reads <= n_intron_max stays only if acc - don + 1 <= intron_max[reads - 1] (64-bit arithmetic);
 *             annotated rows are exempt; n_intron_max = 0 switches the rule off
 *   stage 2, neighbours  over exactly the rows stage 1 left, annotated ones included: dd(r) = the smallest |don(r) - don(q)| over the
 *             OTHER rows q with r's tid, da(r) the same for acc (another row with the same coordinate: 0; no other row on the tid:
 *             0x7fffffff; differences in 64 bits, clamped to 0x7fffffff).  A row of category c stays iff dd >= dist_min[c] and
 *             da >= dist_min[c].  The neighbours are the rows stage 1 left: a row that stage 2 drops still counts as a neighbour of
 *             the others, so nothing is iterated.  All five dist_min zero switch the stage off, and no sort runs.
 * Row order is kept.  g == NULL, or all dist_min zero with n_intron_max == 0: exactly l2r_sj_filter_rows, launch for launch.
 * n_intron_max outside 0..8, a negative dist_min or a negative intron_max entry: an error, l2r_last_error() says which.  The
 * preconditions are those of l2r_sj_filter_rows.  The acceptor side needs the rows in (tid, acc) order: one 64-bit key per row,
 * ordered by the radix passes of `sort` below in the context's sort buffers (a byte that is equal in every key is a pass that is not
 * run, keys that never descend run none, L2R_SORT_FORCE=1 runs all eight); more than 2^32 - 1 - L2R_SORT_TILE rows fail before any
 * pointer is read.
 * l2r_sj_stats from word 23, of the last filter call (all 0 behind l2r_sj_filter_rows): [23] rows stage 2 dropped, [24] radix passes
 * the acceptor order ran; with L2R_SJ_TIMING=1 device milliseconds of [25] k_radix_keys<SjAccKeyOf> [26] the acceptor order's passes (all their
 * kernels) [27] k_sj_near_acc [28] k_sj_keep_near; [29] rows that passed the test of l2r_sj_filter_rows and that the intron-size rule
 * dropped.  [15] is then the rows both stages dropped together. */
typedef struct { int32_t anchor_min[5], uniq_min[5], all_min[5]; } l2r_sj_filter;     /* STAR: 30 12 12 12 / 3 1 1 1 / 3 1 1 1 behind the annotated one */
typedef struct { int32_t dist_min[5]; int32_t n_intron_max; int32_t intron_max[8]; } l2r_sj_filter2;   /* STAR: 10 0 5 10 behind the annotated 0 / 50000 100000 200000 */
typedef struct { int64_t cap, n; int32_t *tid, *don, *acc, *uniq_c, *multi_c; uint8_t *strand, *motif; uint8_t *anno; int32_t *max_over; } l2r_sj_tab;   /* l2r_sj_table + two */
int          l2r_sj_begin_tab(l2r_ctx *ctx, const l2r_sj_params *prm, const l2r_sj_genome *genome);
int          l2r_sj_add_rows_over(l2r_ctx *ctx, const l2r_junctions *rows, const int32_t *max_over);
int          l2r_sj_annotate(l2r_ctx *ctx, const l2r_annotation *anno);
int          l2r_sj_filter_rows(l2r_ctx *ctx, const l2r_sj_filter *filter, int64_t *n_rows);
int          l2r_sj_filter_rows2(l2r_ctx *ctx, const l2r_sj_filter *filter, const l2r_sj_filter2 *filter2, int64_t *n_rows);
int          l2r_sj_download_tab(l2r_ctx *ctx, l2r_sj_tab *table);

/* ---- `sort`, `filter -S` (host/sort.c): the coordinate order of alignment records -- what `update-gtf` wants of its input and the
 * reference pipeline gets from `samtools sort` (Snakefile, rule sam_novel_gtf).  One 64-bit key per record,
 *     key = (tid < 0 ? 0x7fffffff : tid) << 33  |  (uint32)(pos + 1) << 1  |  ((flag >> 4) & 1)
 * (pos: core.pos, 0-based, so -1 gives 0; records without a reference last); records with equal keys keep their input order.  That is
 * the whole definition: no byte equality with the output of any samtools release is claimed.
 * l2r_sort_order: order_out[k] = index of the record at rank k (n words).  A stable LSD radix sort on the device with 8-bit digits
 * and the record index as the payload (csrc/l2r_sort.hip.h); a key byte that is equal in every record is a pass that is not run, and
 * input whose keys never descend is answered with the identity and no pass at all.  n == 0 succeeds; n > 2^32 - 1 - L2R_SORT_TILE
 * fails before any pointer is read.  The device buffers belong to the context, grow on demand and go with l2r_destroy.
 * l2r_sort_stats, of the last l2r_sort_order: out[0] rows, [1] radix passes run (of 8), [2] 1 where the input was in order already;
 * with L2R_SORT_TIMING=1 in the environment at the call (every launch is then waited for) device milliseconds of [3] k_radix_keys<SortKeyOf>
 * [4] k_radix_digit_hist<SortRows> [5] k_scan_u32 of the tile histograms [6] k_radix_scatter<SortRows>, each summed over the passes; n = words of out (up
 * to 7).  L2R_SORT_FORCE=1 (tests): all eight passes run, whether the input is in order and whether bytes are constant. */
#define L2R_SORT_TILE 4096              /* rows one workgroup of a radix pass ranks (csrc/l2r_radix.hip.h holds both to its one tile) */
typedef struct { int64_t n; const uint16_t *flag; const int32_t *tid, *pos; } l2r_sort_records;
int          l2r_sort_order(l2r_ctx *ctx, const l2r_sort_records *recs, uint32_t *order_out);  /* order_out[k] = record at rank k */
int          l2r_sort_stats(l2r_ctx *ctx, double *out, int n);

/* ---- `sort -n`, `filter -N`, `fusion -N` (host/sort.c): the name order of alignment records -- what `filter` and `fusion` want of their
 * input (a read is a run of consecutive records with one name) and the reference leaves to `samtools sort -n` / `samtools collate`.
 * Names are byte strings of 0..254 bytes without a NUL; two names are the same read iff they have the same length and bytes.  The name
 * order is the permutation in which (1) records with one name are consecutive, (2) the groups follow each other by the input index of
 * their first record, (3) the records of a group keep their input order.  Input that is grouped already gives the identity.  That is the
 * whole definition: no equality with the output of any samtools release is claimed.
 * l2r_name_order: name i = names[name_off[i], name_off[i + 1]); order_out[k] = index of the record at rank k (n words), *n_groups =
 * distinct names.  On the device (csrc/l2r_names.hip.h): a seeded 64-bit hash per name, the radix passes of `sort` over the hashes in the
 * context's sort buffers (L2R_SORT_FORCE=1 as there), head flags by hash and byte compare, and the groups placed by two scans.  A pair
 * of neighbours with one hash and two names is a mismatch: with none the result is exact; otherwise the call runs once more with a
 * second seed, and if that mismatches too the order is computed on the host (csrc/l2r_nameorder.hip.h).  All three routes give the same
 * order.  n == 0 succeeds with *n_groups = 0.  n > 2^32 - 1 - L2R_SORT_TILE, a descending name_off, a name of more than 254 bytes or a
 * null column with n > 0 fail before any column is read (the offsets apart) and before anything is launched.
 * L2R_NAME_HASH_BITS=<0..64> (tests): only that many low bits of the hash are kept.
 * l2r_name_stats, of the last l2r_name_order: out[0] rows, [1] groups, [2] radix passes run, [3] 1 where the order is the identity,
 * [4] route (0 first seed, 1 second seed, 2 host), [5] mismatching pairs seen on the first seed; with L2R_SORT_TIMING=1 device
 * milliseconds (summed over the seeds that ran) of [6] k_radix_keys<NameHashOf> [7] the passes [8] k_name_heads [9] the two k_scan_u32
 * [10] k_name_firsts + k_name_sizes + k_name_place; n = words of out (up to 11). */
#define L2R_NAME_MAX 254
typedef struct { int64_t n; const int64_t *name_off /* n + 1 */; const uint8_t *names; } l2r_name_records;
int          l2r_name_order(l2r_ctx *ctx, const l2r_name_records *recs, uint32_t *order_out, int64_t *n_groups);
int          l2r_name_stats(l2r_ctx *ctx, double *out, int n);

/* ---- `sort-gtf`, `sort-gtf-check` (host/gtfsort.c): GTF text merged and put into the order update-gtf, unique-gtf and STAR read it in --
 * the step the reference pipeline runs as a shell script after every concatenation of GTF files.  Inside the domain below the rows,
 * written as h_gtf_write_rows writes them, are that script's output byte for byte (tests/golden/sort_gtf).
 * The text is one byte string (several files: concatenated byte for byte).  Lines end at '\n', a last line without one counts, line
 * numbers start at 1 and count every line.  Fields are runs of bytes other than space and tab (leading blanks are skipped).
 *   kept line        byte 0 is not '#', and the third field contains "transcript" anywhere or equals "exon" (case-sensitive)
 *   transcript line  a kept line whose third field equals "transcript".  It sets the current key (c, s, e): s, e = its fourth and fifth
 *                    fields as decimal numbers; c = the rank of its first field: chr1..chr22 1..22, chrX 23, chrY 24, chrM 25, any
 *                    other name 26, 27, ... by its first appearance on a transcript line
 *   key of a line    every kept line carries the current key of the last transcript line at or before it, (0, 0, 0) before the first;
 *                    a kept line that is no transcript line never has its own columns 1, 4, 5 looked at
 *   order            kept lines by (c, s, e, line number)
 *   domain           on a transcript line fields four and five are non-empty strings of decimal digits of value <= 4294967295 (leading
 *                    zeros allowed), and the text holds no NUL byte; anything else is an error that names the smallest such line
 * l2r_gtf_order: *n_rows = kept lines; the rows are held by the context until the next call and fetched with l2r_gtf_rows_out (cap < n
 * fails and writes nothing).  n_bytes == 0 succeeds with no rows; a negative size or a null text with a positive size fails before
 * anything is read.  On the device (csrc/l2r_gtf.hip.h): the text is uploaded once; newlines are counted and line starts written per
 * tile of L2R_GTF_TILE bytes, one thread per line parses its first five fields, scans compact kept lines and transcripts (which is the
 * carry-forward of the key), the transcripts whose name differs from their predecessor's go to the host to be ranked, and where any row
 * is below its predecessor two stable radix stages (e, then c << 32 | s) run in the context's sort buffers (L2R_SORT_FORCE=1 as there).
 * Texts of 2^32 - 64 bytes and more, more kept rows than one sort takes (2^32 - 1 - L2R_SORT_TILE), and L2R_GTF_ROUTE=host (tests) take
 * the exact host routine (csrc/l2r_gtforder.hip.h): same rows, same errors.
 * l2r_gtf_check needs no context and no GPU: 0 where the kept lines are in the order already (*line = 0), 1 where not (*line = the
 * first kept line whose key is below its predecessor's), negative on a domain error.  counts (null, or 4 words): lines, kept rows,
 * transcript lines, distinct chromosome names.
 * l2r_gtf_stats, of the last l2r_gtf_order: out[0] bytes, [1] lines, [2] kept rows, [3] transcript lines, [4] heads sent to the host,
 * [5] distinct names ranked beyond the table, [6] passes of stage 1, [7] passes of stage 2, [8] 1 where the order is the identity,
 * [9] route (0 device, 1 host); with L2R_SORT_TIMING=1 device milliseconds of [10] k_gtf_count + k_gtf_starts [11] k_gtf_fields
 * [12] the k_scan_u32 [13] k_gtf_rows + heads + k_gtf_triples [14] the two key kernels and all passes [15] k_gtf_compose. */
#define L2R_GTF_TILE 16384              /* bytes of text one workgroup of the line kernels takes */
typedef struct { int64_t n_bytes; const uint8_t *text; } l2r_gtf_text;
typedef struct { int64_t cap, n; uint64_t *start; uint32_t *len; uint32_t *line; } l2r_gtf_rows;   /* kept lines in the order: offset, length without '\n', 1-based line number */
int          l2r_gtf_order(l2r_ctx *ctx, const l2r_gtf_text *text, int64_t *n_rows);
int          l2r_gtf_rows_out(l2r_ctx *ctx, l2r_gtf_rows *rows);          /* of the last l2r_gtf_order; cap < n fails and writes nothing */
int          l2r_gtf_stats(l2r_ctx *ctx, double *out, int n);
int          l2r_gtf_check(const l2r_gtf_text *text, int64_t *line, int64_t *counts);

/* ---- `bam2bed` (host/bed.c): alignment records as BED12 text, one line per mapped record with the blocks between its introns -- what the
 * reference pipeline gets from `bedtools bamtobed -bed12` (Snakefile, rule minimap_map).  The rule below is the whole definition: no byte
 * equality with the output of any bedtools release is claimed.
 * A record with FLAG & 4 writes nothing.  Every other record, in input order, writes twelve tab-separated columns and '\n':
 *    1 the reference name of tid    2 pos (0-based)    3 pos + span    4 QNAME, followed by "/1" where FLAG & 0x40, else "/2" where FLAG & 0x80
 *    5 MAPQ    6 '-' where FLAG & 16, else '+'    7 pos    8 pos + span    9 the colour string    10 the block count
 *    11 the block sizes, commas between them and none behind the last    12 the block starts relative to pos, likewise
 * The blocks come from one walk over the CIGAR: cur = 0, len = 0, starts = [0]; M = X D add their length to cur and len; N appends len to
 * the sizes, adds its length to cur, appends cur to the starts and sets len = 0; I S H P do nothing; at the end len is appended to the
 * sizes and span = cur.  A block may be 0 long (a CIGAR that begins with N, two N in a row, no CIGAR at all).  Sums are 64 bit.
 * Domain errors fail the call and write nothing: a mapped record whose tid is outside [0, n_ref) or whose pos is negative, a CIGAR
 * operation code above 8, an end beyond 2147483647.  l2r_last_error() names the smallest such record (0-based within the call) and the kind.
 *     l2r_bed_begin     once: the reference names (name t = ref_names[ref_off[t], ref_off[t + 1])) and the colour, copied to HBM
 *     l2r_bed_lines     one batch: *n_lines = lines, *n_bytes = bytes of its text, which stays in HBM until the next call.  The columns may
 *                       be a window of larger ones: cig_off[0] and name_off[0] need not be 0 (names as in l2r_name_records, 0..254 bytes).
 *                       The texts of consecutive batches, concatenated, are the text of the whole input however the records were cut.  A
 *                       batch whose summed line bounds (below) reach 2^32 - 64 bytes fails with an error of its own, before any launch
 *     l2r_bed_text_out  the text of the last l2r_bed_lines; cap < n_bytes fails and writes nothing, as does a call behind a failed batch
 *     l2r_bed_cut       no GPU, no context: *n_take = how many records from `first` one batch takes -- at most max_records, their summed
 *                       bounds below max_bytes, but always one.  A line's bound is made of its name length, its reference name's length,
 *                       the colour length and its operation count alone and is never below the line's bytes.  One record whose bound
 *                       alone reaches 2^32 - 64 is an error.  Only flag, tid, cig_off and name_off of the records are read
 * On the device (csrc/l2r_bed.hip.h): k_bed_measure -- per record the bytes of its line, its block count and span; one thread per record,
 * or one wave per record where the batch has more than 32 operations per record on average (L2R_BED_WAVE=0|1 forces one) -- k_scan_u32
 * over the lengths, and k_bed_write: one workgroup per L2R_BED_TILE records composes their text in an LDS image of L2R_BED_LDS_BYTES
 * and streams it out in aligned 16-byte stores; a tile with more text writes its lines directly.  The text buffer has 64 bytes of slack;
 * with L2R_CHECK=1 they are filled with a pattern in front of k_bed_write and looked at behind it.  L2R_BED_ROUTE=host (tests, the
 * comparator of tools/bench_bed.py): the exact host routine of csrc/l2r_bedplan.hip.h, same bytes, same errors.
 * l2r_bed_stats, of the last l2r_bed_lines: out[0] records, [1] lines, [2] bytes, [3] form of k_bed_measure (0 thread, 1 wave), [4] tiles
 * on the LDS path, [5] tiles on the direct path, [6] route (0 device, 1 host), [7] 1 where the guard bytes are intact or were not
 * checked; with L2R_BED_TIMING=1 in the environment (every launch is then waited for) device milliseconds of [8] k_bed_measure
 * [9] k_scan_u32 [10] k_bed_write; n = words of out (up to 11). */
#define L2R_BED_TILE 128                /* records, and threads, of one workgroup of k_bed_write */
#define L2R_BED_LDS_BYTES 32768         /* bytes of a tile's text its LDS image holds; a tile with more takes the direct path */
typedef struct { int64_t n, n_cigar; const uint16_t *flag; const int32_t *tid, *pos; const uint8_t *mapq;
                 const int64_t *cig_off; const uint32_t *cig;           /* len << 4 | op */
                 const int64_t *name_off; const uint8_t *names; } l2r_bed_records;   /* names as in l2r_name_records */
typedef struct { int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names; int32_t color_len; uint8_t color[12]; } l2r_bed_params;
int          l2r_bed_begin(l2r_ctx *ctx, const l2r_bed_params *prm);                         /* reference names and colour to HBM, once */
int          l2r_bed_lines(l2r_ctx *ctx, const l2r_bed_records *recs, int64_t *n_lines, int64_t *n_bytes);   /* one batch; the text stays in HBM */
int          l2r_bed_text_out(l2r_ctx *ctx, uint8_t *text, int64_t cap);                     /* of the last l2r_bed_lines; cap < n_bytes fails and writes nothing */
int          l2r_bed_cut(const l2r_bed_records *recs, const l2r_bed_params *prm, int64_t first, int64_t max_records, int64_t max_bytes, int64_t *n_take);  /* no GPU */
int          l2r_bed_stats(l2r_ctx *ctx, double *out, int n);

/* ---- `unique-gtf` (host/tail.c, host/cmds.c): merge_trans (src/update_gtf.c:98-163, check_iden src/gtf.c:54-92) over a list of
 * transcripts, exact to the host loop.  Transcript i has tid[i], strand rev[i] and the exons [ex_off[i], ex_off[i + 1]) of xs / xe
 * (1-based closed, ascending); its start is xs[ex_off[i]], its end xe[ex_off[i + 1] - 1].  The rule, stated once in
 * csrc/l2r_uniqplan.hip.h: every transcript in input order is offered to a growing list, which is scanned newest entry first; an entry
 * T stops the scan where t.tid > T.tid or t.start > T.end (the offer is then pushed as a new entry with coverage 1), is skipped under -s
 * where the strands differ, and otherwise is judged: single exon against single exon by -D on both ends and the overlap fraction >= -f
 * (a hit: coverage + 1, the entry's start lowered and end raised to the offer's), multi against multi by check_iden (identical: the same
 * mutation; the shorter chain contained in the longer: merged, nothing changes), mixed exon counts and everything else: skipped.  An
 * offer that reaches the front of the list is pushed.
 * Arguments that fail the call (-1): n of 2^31 or more, ex_off that does not start at 0 or descends, a transcript without exons or with
 * 2^31 or more, tid below -1, a negative coordinate.  Every other tid, 2147483647 included, is in the domain.  An exon of 2^31 bases
 * (start 0, end 2147483647) lies outside it: its length is formed in int, as exon_overlap_frac (src/update_gtf.c:80-89) forms it.
 *     l2r_uniq_merge   the verdicts of all n offers; *n_unique = entries of the list.  The results stay with the context
 *     l2r_uniq_out     of the last l2r_uniq_merge: merged[i] = 1 where offer i merged, uniq_of[i] = the rank of the entry it created or
 *                      merged into; per entry, in list order, u_src (the offer that created it), u_start / u_end (first start and last
 *                      end as the hits left them) and u_cov.  Any pointer may be null: that array is not written
 * On the device (csrc/l2r_uniq.hip.h) where (tid, start) does not descend over the input: a transcript that starts beyond every earlier
 * end on its chromosome heads a cluster, clusters are independent, and one wave merges one cluster with its lanes on the list entries.
 * Other input, and every input under L2R_UNIQ_ROUTE=host, takes the exact host routine uniq_host: same arrays.
 * l2r_uniq_stats, of the last l2r_uniq_merge: out[0] rows, [1] unique, [2] clusters, [3] offers of the largest cluster (both 0 where the
 * input is not in order), [4] route (0 device, 1 host), [5] hits identical, [6] hits contained, [7] hits single, [8] end extensions;
 * with L2R_SORT_TIMING=1 in the environment device milliseconds of [9] k_uniq_heads + the cluster cut, [10] k_uniq_merge, [11] the
 * scan of the list lengths + k_uniq_take; n = words of out (up to 12). */
#define L2R_UNIQ_PMAX_TILE 256          /* transcripts of one tile of the prefix maximum behind the cluster cut */
typedef struct { int64_t n; const int32_t *tid; const uint8_t *rev; const int64_t *ex_off /* n + 1 */; const int32_t *xs, *xe; } l2r_uniq_trans;
int          l2r_uniq_merge(l2r_ctx *ctx, const l2r_params *prm, const l2r_uniq_trans *trans, int64_t *n_unique);   /* results stay with the context */
int          l2r_uniq_out(l2r_ctx *ctx, uint8_t *merged /* n */, int32_t *uniq_of /* n */, int32_t *u_src, int32_t *u_start, int32_t *u_end, int32_t *u_cov /* n_unique each */);
int          l2r_uniq_stats(l2r_ctx *ctx, double *out, int n);

/* ---- the read classes of `update-gtf -y` (host/tail.c summary_and_bed; src/update_gtf.c:496-528): how many reads of the input are known,
 * novel with reliable junctions only, novel with an unreliable junction, and unrecognised, and how long the merge_trans list of every
 * class gets when its reads are offered to it in input order.  The class of a read, from its info word: L2R_INFO_KNOWN -> 0; else
 * L2R_INFO_KNOWN_SITE without L2R_INFO_UNREL -> 1; else L2R_INFO_KNOWN_SITE -> 2; else 3.  The merge rule is l2r_uniq_merge's, the strand
 * of a read is L2R_INFO_REV.  The rule and why one list does for the four: csrc/l2r_summaryplan.hip.h.
 *     l2r_summary_begin   the merge parameters (-s, -d, -D, -f of prm); the accumulators are emptied
 *     l2r_summary_add     n reads with their tid and results.  res == NULL: the results of the context's last l2r_run, where they lie in
 *                         HBM (n = its reads); otherwise the arrays of an l2r_download (n_reads = n, ex_off the running sum of the exon
 *                         counts in info), which are uploaded.  tid, info and the exon chains are appended to accumulators in HBM;
 *                         nothing is merged yet -- a shard's end falls inside clusters, and unique counts of shards do not add up.
 *                         n == 0 is fine.  -2: an allocation failed, the accumulators are as they were
 *     l2r_summary_finish  counts[0..3] = the reads of class 0..3, counts[4..7] = the unique transcripts of class 0..3
 * Domain errors fail l2r_summary_finish with -1 and name the smallest read that has one, and of its kinds the first: a tid outside
 * [0, 2^29), a read with no exon, a negative coordinate.  l2r_summary_add fails with -1 where the totals reach 2^31 reads or
 * 2^32 - 64 exons, or where the arrays of res do not fit together.
 * On the device (csrc/l2r_summary.hip.h) where (tid, start) descends inside no class; other input is fetched and takes the exact host
 * routine summary_host -- four uniq_host lists -- as every input does under L2R_SUMMARY_ROUTE=host (read at l2r_summary_begin: the engine
 * then keeps host copies).  L2R_SUMMARY_WAVE=0|1 forces the thread or the wave form of the gather kernel.
 * l2r_summary_stats: out[0] reads, [1] exons, [2] adds, [3] route (0 device, 1 host), [4] clusters, [5] offers of the largest cluster,
 * [6] 1 where the wave form gathered; with L2R_SORT_TIMING=1 in the environment device milliseconds of [7] k_sum_class + k_sum_place + the
 * scans, [8] k_sum_gather, [9] the cluster cut, [10] k_uniq_merge, [11] k_uniq_take + k_sum_count; n = words of out (up to 12). */
typedef struct { int64_t n; const int32_t *tid; const l2r_result *res; /* NULL: the results of the context's last l2r_run where they lie in HBM */ } l2r_summary_reads;
int          l2r_summary_begin(l2r_ctx *ctx, const l2r_params *prm);
int          l2r_summary_add(l2r_ctx *ctx, const l2r_summary_reads *reads);
int          l2r_summary_finish(l2r_ctx *ctx, int64_t counts[8]);
int          l2r_summary_stats(l2r_ctx *ctx, double *out, int n);

/* ---- the GTF block of `bam2gtf` and `unique-gtf` (host/cmds.c, host/tail.c): transcripts as GTF text, the text composed on the device.
 * The rule, stated here once.  A block describes one transcript: a reference tid, a strand rev, n >= 1 exons xs[k]..xe[k] in ascending
 * order, up to four names -- gene id g, transcript id t, gene name G, transcript name T -- and optionally the overrides start, end and
 * cov.  S = xs[0] and E = xe[n - 1]; where start / end are given, S = start and E = end, and they replace the first exon's start and the
 * last exon's end in the exon lines too.  Numbers are printed as %d.  With A the attribute text:
 *     transcript line   <ref>\t<src>\ttranscript\t<S>\t<E>\t.\t<+|->\t.\t<A><C>\n
 *     exon line         <ref>\t<src>\texon\t<xs>\t<xe>\t.\t<+|->\t.\t<A>\n
 * Form L2R_GTX_PLAIN (print_trans, src/gtf.c:597-604; `bam2gtf`): A = gene_id "<g>"; transcript_id "<t>"; -- both parts always, also for an
 * empty name -- <C> is empty, and the exons are written ascending whatever the strand.
 * Form L2R_GTX_READ (print_read_trans, src/gtf.c:607-632; `unique-gtf`): A = the concatenation, in the order gene_id, transcript_id,
 * gene_name, transcript_name, of ` <key> "<s>";` for every non-empty name, with the first space removed; <C> = ` transcript_cov "<cov>";`
 * (cov = 1 where no column is given); the exons are written descending where rev is set.  (With all four names empty the transcript line
 * holds `\t transcript_cov ...` with a blank in front, as host/tail.c's emit_gtf_named writes it; the reference would write none.)
 * Domain errors fail the call with -1 -- distinct from the other failures, as in l2r_uniq_merge -- and write nothing; l2r_last_error()
 * names the smallest block (0-based) and the kind: a selection index outside the transcripts, a tid outside [0, n_ref), a transcript
 * with no exon, a name id at or beyond names_len, a name of 255 or more bytes, a name without a NUL inside the table, a negative S, E,
 * xs, xe or cov; and a block whose text reaches 2^32 - 64 bytes.
 *     l2r_gtftext_begin   once: the reference names (as in l2r_bed_params), the source string (0..1023 bytes, no tab, newline or NUL) and
 *                         the form, copied to HBM
 *     l2r_gtftext_rows    the transcripts to HBM: tid, rev, the exons [ex_off[i], ex_off[i + 1]) of xs / xe, a table names[0, names_len)
 *                         of NUL-terminated strings and the id columns (byte offsets into it; gid and tids always, gname and tname in form
 *                         READ; they may alias).  xs == NULL: the exon chains of the context's last l2r_run, taken where they lie in HBM,
 *                         in read order -- n must equal the run's reads, ex_off and xe are not read and no exon crosses the bus
 *     l2r_gtftext_blocks  the selection: m blocks, block q is transcript sel[q] (sel == NULL: q), with the optional columns start, end and
 *                         cov.  k_gtx_measure runs over all m blocks, the lengths (4 bytes per block) come to the host; *n_lines and
 *                         *n_bytes are the totals.  The domain errors surface here
 *     l2r_gtftext_lines   one batch: blocks from `first` while their count stays within max_blocks and the sum of their measured bytes
 *                         within max_bytes and below 2^32 - 64 -- always at least one.  *n_taken blocks, *n_bytes of text, which stays in
 *                         HBM until the next call.  Batches concatenated are the text of the selection however it was cut
 *     l2r_gtftext_out     the text of the last l2r_gtftext_lines; cap < n_bytes fails and writes nothing, as does a call behind a failure
 * On the device (csrc/l2r_gtftext.hip.h): k_gtx_measure -- one thread per block, or one wave per block where the selection has more than 32
 * exons per block on average (L2R_GTX_WAVE=0|1 forces one) -- k_scan_u32 over the batch's lengths, and k_gtx_write: one workgroup per
 * L2R_GTX_TILE blocks spreads their lines over its lanes, composes the text in an LDS image of L2R_GTX_LDS_BYTES and streams it out in
 * aligned 16-byte stores; a tile with more text writes its lines directly.  The text buffer has 64 bytes of slack; with L2R_CHECK=1 they
 * are filled with a pattern in front of k_gtx_write and looked at behind it.  L2R_GTX_ROUTE=host: the exact host routine of
 * csrc/l2r_gtftextplan.hip.h, same bytes, same errors.
 * l2r_gtftext_stats: out[0] blocks of the selection, [1] lines and [2] bytes of the last batch, [3] form of k_gtx_measure (0 thread,
 * 1 wave), [4] tiles on the LDS path, [5] tiles on the direct path (both of the last batch), [6] route (0 device, 1 host), [7] 1 where the
 * guard bytes are intact or were not checked, [8] batches since l2r_gtftext_blocks; with L2R_GTX_TIMING=1 in the environment (every
 * launch is then waited for) device milliseconds of [9] k_gtx_measure, [10] k_scan_u32 and [11] k_gtx_write, the latter two summed over
 * the batches; n = words of out (up to 12). */
#define L2R_GTX_TILE 32                 /* blocks of one workgroup of k_gtx_write: about 300 lines, 28 KB of text at eight exons per block */
#define L2R_GTX_LDS_BYTES 32768         /* bytes of a tile's text its LDS image holds; a tile with more takes the direct path */
#define L2R_GTX_PLAIN 0
#define L2R_GTX_READ 1
#define L2R_GTX_NAME_MAX 254            /* bytes of a name */
#define L2R_GTX_SRC_MAX 1023            /* bytes of the source string */
typedef struct { int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names; int32_t form, src_len; const uint8_t *src; } l2r_gtx_params;
typedef struct { int64_t n; const int32_t *tid; const uint8_t *rev; const int64_t *ex_off /* n + 1 */; const int32_t *xs, *xe;
                 int64_t names_len; const uint8_t *names; const uint32_t *gid, *tids, *gname, *tname; } l2r_gtx_rows;
typedef struct { int64_t m; const int32_t *sel, *start, *end, *cov; } l2r_gtx_blocks;      /* any of the four may be null */
int          l2r_gtftext_begin(l2r_ctx *ctx, const l2r_gtx_params *prm);
int          l2r_gtftext_rows(l2r_ctx *ctx, const l2r_gtx_rows *rows);
int          l2r_gtftext_blocks(l2r_ctx *ctx, const l2r_gtx_blocks *sel, int64_t *n_lines, int64_t *n_bytes);
int          l2r_gtftext_lines(l2r_ctx *ctx, int64_t first, int64_t max_blocks, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes);
int          l2r_gtftext_out(l2r_ctx *ctx, uint8_t *text, int64_t cap);
int          l2r_gtftext_stats(l2r_ctx *ctx, double *out, int n);

/* ---- the read lists of `update-gtf -a / -k / -v / -u`: classified reads as GTF blocks of form L2R_GTX_READ, selected by class on the
 * device.  The rule, stated here once (src/update_gtf.c:837-913 and :939-964; host/tail.c).  Read i of a run, or of an uploaded
 * l2r_result, has n = info >> 8 exons xs[0..n), xe[0..n) with the flags f[0..n), ref = ref_tx[i], rev = (info & L2R_INFO_REV) != 0, its
 * reference tid[i] and its names qname[i] and tid_name[i] (byte offsets into the reads' table; tid_name == NULL: qname stands for it).
 * Two scalars come with the reads: has_sj (a junction table was set) and split (l2r_params.split_trans).
 * Lists, in read order:
 *     L2R_GTX_LIST_ALL      every read, whole
 *     L2R_GTX_LIST_KNOWN    reads with FULL && KNOWN, whole
 *     L2R_GTX_LIST_UNRECOG  reads with FULL && !KNOWN && !KNOWN_SITE, whole
 *     L2R_GTX_LIST_NOVEL    reads with FULL && !KNOWN && KNOWN_SITE: whole where !has_sj || SJ_PASS; else, where split, the read's pieces
 *                           k = 0, 1, ... in ascending order; else nothing
 * Pieces: walk j = 0 .. n - 1 with first = 0 and seen_novel = seen_known = 0.  For j < n - 1, L2R_EXF_NOVEL_JUNC of f[j] sets seen_novel,
 * its absence seen_known.  At j == n - 1, or where f[j] has L2R_EXF_UNREL_JUNC: if seen_novel && seen_known && j - first >= 1 the exons
 * [first, j] are piece k, and k += 1; in every case first = j + 1 and both flags are cleared.
 * A whole read is the block of form L2R_GTX_READ with ref = tid[i], S = xs[0], E = xe[n - 1], strand rev, cov 1, g = the gene id of
 * annotation transcript ref (`NA` where ref < 0), t = tid_name[i], G = the gene name of ref (or `NA`), T = qname[i], the exons descending
 * where rev; an empty name drops its attribute.  Piece k over the exons [first, last] (quirk Q2): its TRANSCRIPT line is that of a block
 * with reference 0, S = E = 0 and strand `+`; its EXON lines carry tid[i] and rev, and are ascending whatever the strand (the order follows
 * the transcript line's strand); t and T carry the suffix `.split.<k>` (%d); g, G and cov as for the whole read.
 * Domain errors, as for the GTF block (-1, nothing written, the smallest block of the list and its kind named), looked for in this order:
 * a tid outside [0, n_ref); a read with no exon; ref at or beyond the annotation's transcripts; the four names in the order g, t, G, T,
 * each with the id / 255-byte / NUL tests (g and G in the annotation's table, t and T in the reads'); a piece whose t or T with its suffix
 * has 100 or more bytes; a negative coordinate; a block of 2^32 - 64 bytes or more.
 *     l2r_gtftext_anno      once behind l2r_gtftext_begin with form READ: the annotation's gene tables, as in l2r_detail_params, to HBM
 *     l2r_gtftext_reads     the reads -- tid, the names table, qname, tid_name (may be NULL) -- to HBM, with res, the arrays of an
 *                           l2r_download (n_reads == n), which are uploaded; res == NULL: the results of the context's last l2r_run where
 *                           they lie in HBM (n must equal the run's reads, which must have kept its results).  It takes the place of
 *                           l2r_gtftext_rows
 *     l2r_gtftext_list      one list of the reads: k_rl_count (one thread per read: 0, 1 or its pieces), k_scan_u32, k_rl_take (read, first
 *                           exon, exon count, piece number or -1 per block, in read order) and k_rl_measure, all on the device; *m blocks,
 *                           and the totals.  It takes the place of l2r_gtftext_blocks, the domain errors surface here, and it may be
 *                           called for each list in turn on the same reads
 *     l2r_gtftext_list_out  the selection of the last l2r_gtftext_list (tests, tools): any column may be NULL
 * l2r_gtftext_lines, _out and _stats serve both; behind a list k_rl_write (csrc/l2r_readlist.hip.h) composes the text as k_gtx_write does,
 * with a per-block length of the transcript line beside that of the exon lines.  L2R_GTX_ROUTE=host: the exact host routine of
 * csrc/l2r_readlistplan.hip.h.  l2r_gtftext_stats has two more words behind a list: [12] device milliseconds of the selection (k_rl_count,
 * k_scan_u32, k_rl_take; with L2R_GTX_TIMING=1) and [13] the piece blocks of the list. */
#define L2R_GTX_LIST_ALL 0
#define L2R_GTX_LIST_KNOWN 1
#define L2R_GTX_LIST_NOVEL 2
#define L2R_GTX_LIST_UNRECOG 3
#define L2R_GTX_PIECE_NAME_MAX 100      /* bytes a piece's name with its suffix stays below */
typedef struct { int64_t n_tx, anno_names_len; const uint8_t *anno_names; const uint32_t *tx_gid, *tx_gname; } l2r_gtx_anno;
typedef struct { int64_t n; const int32_t *tid; int64_t names_len; const uint8_t *names; const uint32_t *qname, *tid_name /* may be NULL */;
                 const l2r_result *res; /* NULL: the results of the context's last l2r_run where they lie in HBM */
                 int32_t has_sj, split; } l2r_gtx_reads;
int          l2r_gtftext_anno(l2r_ctx *ctx, const l2r_gtx_anno *anno);
int          l2r_gtftext_reads(l2r_ctx *ctx, const l2r_gtx_reads *reads);
int          l2r_gtftext_list(l2r_ctx *ctx, int list, int64_t *m, int64_t *n_lines, int64_t *n_bytes);
int          l2r_gtftext_list_out(l2r_ctx *ctx, int32_t *read, int32_t *first, int32_t *count, int32_t *piece);

/* ---- the per-read detail table of `update-gtf -A` (host/cmds.c, host/tail.c print_detail): one text line per read, the text composed on
 * the device.  The rule, stated here once (print_bam_detail_trans, src/update_gtf.c:297-419).  For read i: n = info >> 8 exons with the
 * starts xs[0..n), the ends xe[0..n) and the flags f[0..n); ref = ref_tx[i].  Numbers are printed as %d.
 *     <qname>\t<chr>\t<+|->\t<cls>\t<gid>\t<gname>\t<n>\t<xs, comma separated>\t<xe, comma separated>\t<L1><L2><L3><L4>\n
 * +|- is L2R_INFO_REV (the strand after classification, not the record's); cls is 0 with L2R_INFO_KNOWN, else 1 with
 * L2R_INFO_KNOWN_SITE, else 2; gid and gname are the gene id and gene name of the annotation transcript ref, both `NA` where ref < 0.
 *     L1   over the exons j of [0, n) with L2R_EXF_NOVEL_EXON: j
 *     L2   over the junctions j of [0, n - 1): 2j where L2R_EXF_NOVEL_DON and 2j + 1 where L2R_EXF_NOVEL_ACC, in that order
 *     L3   over j of [0, n - 1) with L2R_EXF_NOVEL_JUNC: j
 *     L4   the same with L2R_EXF_UNREL_JUNC
 * A list is <count>\t and its members comma separated, or `NA` where the count is 0.  L1, L2 and L3 are followed by a tab.  L4 is followed
 * by a tab ONLY WHERE IT IS EMPTY (host/tail.c's index_list writes `NA\t` whatever its trailing_tab says, as the reference does): a line
 * ends `...\t0\tNA\t\n` or `...\t1\t1\n`.  This is the behaviour to keep.  A flag of the last exon that belongs to a junction list does
 * not appear: those lists stop at n - 1.  The header line (`ReadName\tchr\t...`) is the command's to write.
 * Domain errors fail the call with -1 and write nothing; l2r_last_error() names the smallest read (0-based) and the kind, in the order
 * they are looked for: a tid outside [0, n_ref); a read-name id at or beyond names_len, a read name of 255 or more bytes, or one without a
 * NUL; ref at or beyond the annotation's transcripts; a gene id or gene name with an id, length or NUL fault in the annotation's table; a
 * read with no exon; a negative start or end; a line of 2^32 - 64 bytes or more.
 *     l2r_detail_begin   once: the reference names (as in l2r_bed_params) and the annotation's gene tables -- anno_names[0, anno_names_len)
 *                        of NUL-terminated strings, tx_gid / tx_gname the byte offsets of transcript t's gene id / gene name -- to HBM
 *     l2r_detail_rows    the reads (struct l2r_detail_reads: C has one name space for typedefs and functions): tid, a table names[0, names_len) of NUL-terminated strings, qname the byte offsets of the read names,
 *                        and res, the arrays of an l2r_download (n_reads == n), which are uploaded; res == NULL: the results of the
 *                        context's last l2r_run where they lie in HBM -- n must equal the run's reads, the run must have kept its
 *                        results (L2R_WANT_RESULTS), and no exon, flag or result word crosses the bus.  k_detail_measure runs over all n
 *                        reads, the lengths (4 bytes per read) come to the host; *n_bytes is the total.  The domain errors surface here
 *     l2r_detail_lines   one batch: reads from `first` while their count stays within max_rows and the sum of their bytes within max_bytes
 *                        and below 2^32 - 64 -- always at least one.  *n_taken reads, *n_bytes of text, which stays in HBM until the next
 *                        call.  Batches concatenated are the text of the rows however it was cut
 *     l2r_detail_out     the text of the last l2r_detail_lines; cap < n_bytes fails and writes nothing, as does a call behind a failure
 * On the device (csrc/l2r_detail.hip.h): k_detail_measure -- one thread per read, or one wave per read where the rows have more than 32
 * exons per read on average (L2R_DETAIL_WAVE=0|1 forces one) -- leaves a line's length and where its seven segments (head, starts, ends,
 * L1..L4) begin; k_scan_u32 over the batch's lengths; k_detail_write: one workgroup per L2R_DETAIL_TILE reads takes their segments as its
 * work items, a lane per segment of a short read, a wave per segment of a long one, composes the text in an LDS image of
 * L2R_DETAIL_LDS_BYTES and streams it out in aligned 16-byte stores; a tile with more text writes straight to the text.  The text buffer
 * has 64 bytes of slack; with L2R_CHECK=1 they are filled with a pattern in front of k_detail_write and looked at behind it.
 * L2R_DETAIL_ROUTE=host: the exact host routine of csrc/l2r_detailplan.hip.h, same bytes, same errors.
 * l2r_detail_stats: out[0] rows, [1] lines and [2] bytes of the last batch, [3] form of k_detail_measure (0 thread, 1 wave), [4] tiles on
 * the LDS path, [5] tiles on the direct path (both of the last batch), [6] route (0 device, 1 host), [7] 1 where the guard bytes are intact
 * or were not checked, [8] batches since l2r_detail_rows; with L2R_DETAIL_TIMING=1 in the environment (every launch is then waited for)
 * device milliseconds of [9] k_detail_measure, [10] k_scan_u32 and [11] k_detail_write, the latter two summed over the batches; n = words
 * of out (up to 12). */
#define L2R_DETAIL_TILE 32              /* reads of one workgroup of k_detail_write: 224 segments, about 6 KB of text at eight exons per read */
#define L2R_DETAIL_LDS_BYTES 32768      /* bytes of a tile's text its LDS image holds; a tile with more takes the direct path */
#define L2R_DETAIL_NAME_MAX 254         /* bytes of a read name, a gene id, a gene name */
typedef struct { int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;          /* as l2r_bed_params */
                 int64_t n_tx, anno_names_len; const uint8_t *anno_names; const uint32_t *tx_gid, *tx_gname; } l2r_detail_params;
typedef struct { int64_t n; const int32_t *tid; int64_t names_len; const uint8_t *names; const uint32_t *qname;
                 const l2r_result *res; /* NULL: the results of the context's last l2r_run where they lie in HBM */ } l2r_detail_reads;
int          l2r_detail_begin(l2r_ctx *ctx, const l2r_detail_params *prm);
int          l2r_detail_rows(l2r_ctx *ctx, const l2r_detail_reads *rows, int64_t *n_bytes);
int          l2r_detail_lines(l2r_ctx *ctx, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes);
int          l2r_detail_out(l2r_ctx *ctx, uint8_t *text, int64_t cap);
int          l2r_detail_stats(l2r_ctx *ctx, double *out, int n);

/* ---- the novel list of `update-gtf` (host/tail.c h_update_tail, summary_and_bed; src/update_gtf.c:181-295, :421-587, :939-964): the novel
 * reads of a run merged into the list U behind the updated GTF, the kept novel exons, sites, junctions and genes behind `-E` and the
 * "Updated information" block of `-y`.  The rule, stated here once, for runs in which no read is split.
 * Offers.  Read i is an offer where FULL && !KNOWN && KNOWN_SITE and (!has_sj || SJ_PASS) -- read_route == T_NOVEL_WHOLE.  Its strand is
 * L2R_INFO_REV, its chain and exon flags are the results'.  A read with FULL && !KNOWN && KNOWN_SITE, has_sj && !SJ_PASS and split
 * (l2r_params.split_trans) set is split-route: such reads are counted, and where there is one l2r_novel_finish refuses (-3).
 * List U.  The offers in input order go to ONE merge_trans list; the rule is l2r_uniq_merge's with -c, -d, -D, -f of l2r_params.  Entry e
 * has src, the read that created it (global index: the reads added before + its place in its add), tid, rev and ref = ref_tx of src, its
 * coverage cov, the chain of src with xs[0] and xe[n - 1] replaced by the widened start and end, and the flags of src.
 * Novel items.  Over the entries in list order and j ascending, reading the entry's widened chain:
 *     exon          (tid, xs[j], xe[j]) where f[j] & NOVEL_EXON; it carries cov, rev and a type: T for j == 0 or j == n - 1 where n > 1,
 *                   I in between, S where n == 1
 *     donor         (tid, xe[j]) where j < n - 1 and NOVEL_DON          acceptor   (tid, xs[j + 1]) where j < n - 1 and NOVEL_ACC
 *     junction      (tid, xe[j], xs[j + 1]) where j < n - 1 and NOVEL_JUNC
 *     gene          (tid, gene(ref)) per entry
 *     known gene    (tid[i], gene(ref_tx[i])) of every read with KNOWN, whether FULL or not, in input order
 * gene() is the ordinal of the gene-id string among the annotation's distinct gene-id strings (tx_gene[ref]); ref < 0 stands for the
 * string `NA` and takes na_gene, which is the ordinal of an annotation gene called `NA` where there is one.
 * Every list keeps the first item of every key, in the order of first appearance; a kept exon row takes the type and strand of the first
 * item and score = the sum of cov over the key.  With tid not descending this is what the backward scans of summary_and_bed leave.
 * The two gene lists then lose what add_gene's order of tests drops on top: it compares the gene BEFORE it stops at a smaller tid, so
 * an item whose gene equals that of the newest kept row of a smaller tid is not kept either (one pass in list order; a row that goes
 * takes no part later).  Seen from the lists: the same gene on two tids counts twice unless it was the newest gene when the first ended.
 * BED line of a kept exon row: <ref>\t<start - 1>\t<end>\t<T|I|S>_exon\t<score>\t<+|->\n, numbers as %d (a start of 0 prints -1).
 * Counts, in the order of h_write_summary_text: counts[0] genes, [1] entries, [2] 0, [3] exons, [4] donors + acceptors, [5] junctions,
 * [6] 0 (not this unit's), [7] known genes.
 *     l2r_novel_begin        -c, -d, -D, -f and -s of prm; has_sj; the reference names (as in l2r_bed_params); tx_gene[0, n_tx) and
 *                            na_gene; the accumulators are emptied
 *     l2r_novel_add          n reads with their tid and results.  res == NULL: the results of the context's last l2r_run where they lie
 *                            in HBM (n = its reads); otherwise the arrays of an l2r_download, which are uploaded.  The offers' columns,
 *                            chains and flags and the known reads' (tid, gene) are appended to accumulators in HBM, which grow by
 *                            doubling.  n == 0 is fine.  -2: an allocation failed, the accumulators are as they were
 *     l2r_novel_finish       merges, makes and keeps; counts[0..7] as above.  -3 where there are split-route reads (it says how many)
 *     l2r_novel_entries_out  per entry src, start, end, cov; any pointer may be null
 *     l2r_novel_rows_out     the kept rows of one list (L2R_NOVEL_EXON ..): tid, a, b -- exon (start, end), site (coordinate, 0),
 *                            junction (donor, acceptor), gene (ordinal, 0) -- and for exons score and meta = type | rev << 2 (type 0 T,
 *                            1 I, 2 S); any pointer may be null.  Tests and tools
 *     l2r_novel_lines        one batch of text.  which = L2R_NOVEL_BED: kept exon rows from `first` while their count stays within
 *                            max_rows and the sum of their bytes within max_bytes and below 2^32 - 64 -- always at least one.  Batches
 *                            concatenated are the whole text.  which = L2R_NOVEL_GTF, behind l2r_novel_names: blocks (entries) of the
 *                            updated GTF, cut and composed by l2r_gtftext_lines
 *     l2r_novel_names        the updated GTF.  Entry e is the block of form L2R_GTX_READ with the overrides start, end and cov, g / G the
 *                            gene id / gene name of annotation transcript ref (`NA` where ref < 0), t = tid_name[e], T = qname[e] -- the
 *                            bytes print_merged writes for a whole entry.  The caller fetches src (l2r_novel_entries_out) and sends a
 *                            names table for the entries alone.  The GTF-text unit (l2r_gtftext_*) is set up over the offers where
 *                            they lie in HBM -- its rows are the accumulators' columns and chains, copied inside HBM, its blocks the
 *                            entries -- and measures; *n_lines and *n_bytes are the totals.  It takes that unit's state: rows, blocks
 *                            and text of an earlier l2r_gtftext_* call on the context are gone.  A caller that uses the read lists
 *                            (l2r_gtftext_reads / _list) on the same context calls this behind the last of them and sets them up again
 *                            afterwards.  qname / tid_name at or beyond names_len are refused (-4).  Under L2R_NOVEL_ROUTE=host the rows go
 *                            through l2r_gtftext_rows, which reads L2R_GTX_ROUTE itself: the text is still composed by the kernels
 *                            unless that is host as well.  The domain errors of a GTF block (a
 *                            name of 255 bytes or more, ...) surface here with -1.  Needs src and the gene tables at the begin
 *     l2r_novel_out          the text of the last l2r_novel_lines; cap < n_bytes fails and writes nothing
 * Domain errors fail l2r_novel_finish with -1 and name the smallest read (global index) that has one, and of its kinds the first: a
 * tid outside [0, n_ref), a read with no exon, ref at or beyond n_tx -- looked for in every read -- and a negative coordinate, looked for
 * in the chains of the offers.  l2r_novel_add fails with -1 where the totals reach 2^31 reads or 2^32 - 64 exons, or where the arrays of
 * res do not fit together.  A refusal leaves the unit usable: the next l2r_novel_begin starts afresh.
 * On the device (csrc/l2r_novel.hip.h) where (tid, start) does not descend over the offers and tid does not descend over the known
 * reads; other input is fetched and takes the exact host routine novel_host -- uniq_host and the literal backward scans -- as every input
 * does under L2R_NOVEL_ROUTE=host (read at l2r_novel_begin: the engine then keeps host copies).  L2R_NOVEL_WAVE=0|1 forces the thread
 * or the wave form of the chain copy.  The text buffer has 64 bytes of slack; with L2R_CHECK=1 they are filled with a pattern in front of
 * the write kernel and looked at behind it.
 * NOTE: route 0 does not mean that every kept row was made on the device alone.  The kernels keep the first item of every key of all six
 * lists; the rows of the two GENE lists then come to the host (at most genes x chromosomes of them), where add_gene's last test is made,
 * and l2r_novel_rows_out serves lists 4 and 5 from host memory on both routes.
 * l2r_novel_stats: out[0] reads, [1] offers, [2] split-route reads, [3] known reads, [4] adds, [5] route (0 device, 1 host), [6] clusters,
 * [7] offers of the largest cluster, [8] entries, [9] hits, [10] entries a hit has widened, [11..16] items and [17..22] kept rows of the
 * six lists, [23] 1 where the wave form copied the chains of the last add, [24] 1 where the guard bytes are intact or were not checked;
 * with L2R_SORT_TIMING=1 in the environment device milliseconds of [25] the selection (summed over the adds), [26] the merge, [27] the
 * items, [28] the two sort stages, [29] heads, sums and compaction, [30] k_nov_bed_measure, and, summed over the batches, [31] the
 * scans and [32] k_nov_bed_write; n = words of out (up to 33). */
#define L2R_NOVEL_GTF 0
#define L2R_NOVEL_BED 1
#define L2R_NOVEL_EXON 0
#define L2R_NOVEL_DON 1
#define L2R_NOVEL_ACC 2
#define L2R_NOVEL_JUNC 3
#define L2R_NOVEL_GENE 4
#define L2R_NOVEL_KNOWN_GENE 5
typedef struct { int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;          /* as l2r_bed_params */
                 int64_t n_tx; const uint32_t *tx_gene; uint32_t na_gene; int32_t has_sj;
                 int32_t src_len; const uint8_t *src;                       /* the updated GTF: the source string (NULL: no GTF text) ... */
                 int64_t anno_names_len; const uint8_t *anno_names; const uint32_t *tx_gid, *tx_gname;      /* ... and the gene tables, as in l2r_gtx_anno */
               } l2r_novel_params;
typedef struct { int64_t names_len; const uint8_t *names; const uint32_t *qname, *tid_name /* may be NULL */; } l2r_novel_name_table;   /* per entry: byte offsets into names */
int          l2r_novel_begin(l2r_ctx *ctx, const l2r_params *prm, const l2r_novel_params *np);
int          l2r_novel_add(l2r_ctx *ctx, const l2r_summary_reads *reads);
int          l2r_novel_finish(l2r_ctx *ctx, int64_t counts[8]);
int          l2r_novel_entries_out(l2r_ctx *ctx, int32_t *src, int32_t *start, int32_t *end, int32_t *cov);
int          l2r_novel_names(l2r_ctx *ctx, const l2r_novel_name_table *names, int64_t *n_lines, int64_t *n_bytes);
int          l2r_novel_rows_out(l2r_ctx *ctx, int list, int32_t *tid, int32_t *a, int32_t *b, int32_t *score, uint8_t *meta);
int          l2r_novel_lines(l2r_ctx *ctx, int which, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes);
int          l2r_novel_out(l2r_ctx *ctx, uint8_t *text, int64_t cap);
int          l2r_novel_stats(l2r_ctx *ctx, double *out, int n);

#ifdef __cplusplus
}
#endif
#endif
