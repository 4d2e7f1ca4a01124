// l2r_gtftextplan.hip.h -- the host side of l2r_gtftext_* (the GTF block of `bam2gtf` and `unique-gtf`): the argument checks, gtx_block_bytes
// (the exact bytes and lines of one block, and its domain error), the text of a domain error, and gtx_text_host, the exact routine that
// writes the same bytes on one core (L2R_GTX_ROUTE=host, and the comparator of tools/bench_gtx.py).  In front of them, what the detail
// table (l2r_detailplan.hip.h) and the read lists (l2r_readlistplan.hip.h) check and cut in the same way, stated once: text_check_ref_off
// (the walk of a reference-offset table), text_check_genes (the annotation's gene tables), text_check_reads (reads with their results)
// and batch_cut (the batch cut over the measured lengths).  Host arithmetic only: no HIP call, no context, no environment.
// tests/gtx_dump.hip runs it as a stand-alone program for tests/test_gtf_text_cpu.py.
//
// The rule is stated in include/lr2rmats_hip.h.  What both sides share beyond it: the order in which a block's domain errors are looked for
// (GTX_E_*: the first that applies is the block's kind; the names in the order gene id, transcript id, gene name, transcript name, each
// with its own id / length / NUL test before the next name is looked at), and the pieces a line's length is made of (gtx_line_fix).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

constexpr uint64_t GTX_BATCH_BYTES = 0xffffffffull - 63;  // 2^32 - 64: a block's bytes, and the summed bytes of one batch, stay below it (32-bit offsets)
constexpr int64_t GTX_REF_NAME_MAX = 65535;               // bytes of a reference name (l2r_gtftext_begin)

// kinds of a block's domain error, in the order they are looked for
enum { GTX_OK = 0, GTX_E_SEL, GTX_E_TID, GTX_E_NOEXON, GTX_E_NAME_ID, GTX_E_NAME_LONG, GTX_E_NAME_NUL, GTX_E_NEG, GTX_E_BIG, GTX_E_N };

static const char *gtx_kind_text(int kind)
{
    switch (kind) {
    case GTX_E_SEL: return "a selection index outside the transcripts";
    case GTX_E_TID: return "a reference outside the table";
    case GTX_E_NOEXON: return "a transcript with no exon";
    case GTX_E_NAME_ID: return "a name id at or beyond names_len";
    case GTX_E_NAME_LONG: return "a name of 255 or more bytes";
    case GTX_E_NAME_NUL: return "a name without a NUL inside the table";
    case GTX_E_NEG: return "a negative start, end, exon coordinate or coverage";
    case GTX_E_BIG: return "its text reaches 2^32 - 64 bytes";
    default: return "no error";
    }
}

static int gtx_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// the one text of a block's domain error, for both routes
static int gtx_block_fail(std::string &msg, int64_t q, int kind) { return gtx_fail(msg, "[l2r_gtftext_blocks] block %lld: %s", (long long)q, gtx_kind_text(kind)); }

// ---- what the text commands check and cut alike (who: the entry point a message names).  0, or -2 (an argument error, not a domain
// error) and the text of l2r_last_error().

// The walk of a reference-offset table of n_ref > 0 names, ref_off != NULL: it starts at 0, does not descend, no name is longer than
// GTX_REF_NAME_MAX, and where there are bytes there is a ref_names.
static int text_check_ref_off(int32_t n_ref, const int64_t *ref_off, const uint8_t *ref_names, std::string &msg, const char *who)
{
    if (ref_off[0] != 0) { gtx_fail(msg, "[%s] ref_off does not start at 0", who); return -2; }
    for (int32_t k = 0; k < n_ref; ++k) {
        const int64_t l = ref_off[k + 1] - ref_off[k];
        if (l < 0) { gtx_fail(msg, "[%s] ref_off descends at name %d", who, k); return -2; }
        if (l > GTX_REF_NAME_MAX) { gtx_fail(msg, "[%s] reference name %d has %lld bytes (at most %lld)", who, k, (long long)l, (long long)GTX_REF_NAME_MAX); return -2; }
    }
    if (ref_off[n_ref] > 0 && !ref_names) { gtx_fail(msg, "[%s] null ref_names", who); return -2; }
    return 0;
}

// The annotation's gene tables (l2r_detail_begin, l2r_gtftext_anno): sizes and pointers
static int text_check_genes(int64_t n_tx, int64_t anno_names_len, const uint8_t *anno_names, const uint32_t *tx_gid, const uint32_t *tx_gname, std::string &msg, const char *who)
{
    if (n_tx < 0 || n_tx >= ((int64_t)1 << 31)) { gtx_fail(msg, "[%s] %lld annotation transcripts (below 2^31)", who, (long long)n_tx); return -2; }
    if (anno_names_len < 0 || anno_names_len > 0xffffffffll) { gtx_fail(msg, "[%s] an annotation names table of %lld bytes (at most 2^32 - 1)", who, (long long)anno_names_len); return -2; }
    if (anno_names_len > 0 && !anno_names) { gtx_fail(msg, "[%s] null anno_names", who); return -2; }
    if (n_tx > 0 && (!tx_gid || !tx_gname)) { gtx_fail(msg, "[%s] null gene column", who); return -2; }
    return 0;
}

// Reads with their results (l2r_detail_rows: noun "rows", l2r_gtftext_reads: "reads"): sizes and pointers; with results (s != NULL, else
// those of the last l2r_run) their sizes, and ex_off against the exon counts of info -- the kernels take a read's exons from both.  What
// a read holds is the business of the lines and blocks (detail_line_bytes, rl_block_bytes).
static int text_check_reads(int64_t n, int64_t names_len, const uint8_t *names, const int32_t *tid, const uint32_t *qname, const l2r_result *s, std::string &msg,
                            const char *who, const char *noun)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) { gtx_fail(msg, "[%s] %lld reads (below 2^31)", who, (long long)n); return -2; }
    if (names_len < 0 || names_len > 0xffffffffll) { gtx_fail(msg, "[%s] a names table of %lld bytes (at most 2^32 - 1)", who, (long long)names_len); return -2; }
    if (names_len > 0 && !names) { gtx_fail(msg, "[%s] null names", who); return -2; }
    if (n > 0 && (!tid || !qname)) { gtx_fail(msg, "[%s] null column", who); return -2; }
    if (!s) return 0;                                       // (the results of the last l2r_run)
    if (s->n_reads != n) { gtx_fail(msg, "[%s] results of %lld reads for %lld %s", who, (long long)s->n_reads, (long long)n, noun); return -2; }
    if (s->n_exons < 0 || s->n_exons > 0xffffffffll) { gtx_fail(msg, "[%s] results of %lld exons (at most 2^32 - 1)", who, (long long)s->n_exons); return -2; }
    if (!s->ex_off) { gtx_fail(msg, "[%s] null ex_off", who); return -2; }
    if (n > 0 && (!s->info || !s->ref_tx)) { gtx_fail(msg, "[%s] null result column", who); return -2; }
    if (s->n_exons > 0 && (!s->ex_start || !s->ex_end || !s->ex_flag)) { gtx_fail(msg, "[%s] null exon column", who); return -2; }
    if (s->ex_off[0] != 0) { gtx_fail(msg, "[%s] ex_off does not start at 0", who); return -2; }
    for (int64_t i = 0; i < n; ++i)
        if (s->ex_off[i + 1] - s->ex_off[i] != (int64_t)L2R_INFO_NEXON(s->info[i])) {
            gtx_fail(msg, "[%s] read %lld: ex_off gives %lld exons, info %u", who, (long long)i, (long long)(s->ex_off[i + 1] - s->ex_off[i]), L2R_INFO_NEXON(s->info[i]));
            return -2;
        }
    if (s->ex_off[n] != s->n_exons) { gtx_fail(msg, "[%s] ex_off ends at %lld, the results hold %lld exons", who, (long long)s->ex_off[n], (long long)s->n_exons); return -2; }
    return 0;
}

// How many items (noun: "block", "row") from `first` one batch takes, over the measured lengths len[0, m): while their count stays within
// max_items and the 64-bit sum of their bytes within max_bytes and below 2^32 - 64 -- but always one.  *n_bytes = their sum.
static int batch_cut(const uint32_t *len, int64_t m, int64_t first, int64_t max_items, int64_t max_bytes, int64_t *n_take, int64_t *n_bytes, std::string &msg,
                    const char *who, const char *noun)
{
    if (!n_take || !n_bytes) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    *n_take = 0; *n_bytes = 0;
    if (first < 0 || first >= m) { gtx_fail(msg, "[%s] first %s %lld of %lld", who, noun, (long long)first, (long long)m); return -2; }
    if (max_items < 1 || max_bytes < 1) { gtx_fail(msg, "[%s] a batch of %lld %ss and %lld bytes", who, (long long)max_items, noun, (long long)max_bytes); return -2; }
    uint64_t sum = 0;
    int64_t k = 0;
    for (; first + k < m && k < max_items; ++k) {
        const uint64_t b = len[first + k];
        if (k > 0 && (sum + b > (uint64_t)max_bytes || sum + b >= GTX_BATCH_BYTES)) break;
        sum += b;
    }
    *n_take = k; *n_bytes = (int64_t)sum;
    return 0;
}
// ... of the blocks of l2r_gtftext_lines
static int gtx_cut(const uint32_t *len, int64_t m, int64_t first, int64_t max_blocks, int64_t max_bytes, int64_t *n_take, int64_t *n_bytes, std::string &msg)
{ return batch_cut(len, m, first, max_blocks, max_bytes, n_take, n_bytes, msg, "l2r_gtftext_lines", "block"); }

// ---- the GTF text

// 0, or -2 and the text.  The source string is read; ref_off is walked last, behind the form and the source.
static int gtx_check_params(const l2r_gtx_params *p, std::string &msg, const char *who = "l2r_gtftext_begin")
{
    if (!p) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    if (p->n_ref < 0) { gtx_fail(msg, "[%s] %d reference names", who, p->n_ref); return -2; }
    if (p->n_ref > 0 && !p->ref_off) { gtx_fail(msg, "[%s] null ref_off", who); return -2; }
    if (p->form != L2R_GTX_PLAIN && p->form != L2R_GTX_READ) { gtx_fail(msg, "[%s] form %d (0 plain, 1 read)", who, p->form); return -2; }
    if (p->src_len < 0 || p->src_len > L2R_GTX_SRC_MAX) { gtx_fail(msg, "[%s] a source string of %d bytes (0..%d)", who, p->src_len, L2R_GTX_SRC_MAX); return -2; }
    if (p->src_len > 0 && !p->src) { gtx_fail(msg, "[%s] null source string", who); return -2; }
    for (int32_t k = 0; k < p->src_len; ++k)
        if (p->src[k] == '\t' || p->src[k] == '\n' || p->src[k] == 0) { gtx_fail(msg, "[%s] the source string holds a tab, a newline or a NUL at byte %d", who, k); return -2; }
    if (p->n_ref > 0 && text_check_ref_off(p->n_ref, p->ref_off, p->ref_names, msg, who)) return -2;
    return 0;
}

// 0, or -2 and the text.  Sizes, pointers and ex_off are looked at; what a transcript holds is the blocks' business (gtx_block_bytes).
static int gtx_check_rows(const l2r_gtx_rows *r, int form, std::string &msg, const char *who = "l2r_gtftext_rows")
{
    if (!r) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    if (r->n < 0 || r->n >= ((int64_t)1 << 31)) { gtx_fail(msg, "[%s] %lld transcripts (below 2^31)", who, (long long)r->n); return -2; }
    if (r->names_len < 0 || r->names_len > 0xffffffffll) { gtx_fail(msg, "[%s] a names table of %lld bytes (at most 2^32 - 1)", who, (long long)r->names_len); return -2; }
    if (r->names_len > 0 && !r->names) { gtx_fail(msg, "[%s] null names", who); return -2; }
    if (r->n == 0) return 0;
    if (!r->tid || !r->rev || !r->gid || !r->tids) { gtx_fail(msg, "[%s] null column", who); return -2; }
    if (form == L2R_GTX_READ && (!r->gname || !r->tname)) { gtx_fail(msg, "[%s] null name column (form READ has four)", who); return -2; }
    if (!r->xs) return 0;                                   // (the chains of the last l2r_run: ex_off and xe are not read)
    if (!r->xe || !r->ex_off) { gtx_fail(msg, "[%s] null column", who); return -2; }
    if (r->ex_off[0] != 0) { gtx_fail(msg, "[%s] ex_off does not start at 0", who); return -2; }
    for (int64_t i = 0; i < r->n; ++i) {
        const int64_t k = r->ex_off[i + 1] - r->ex_off[i];
        if (k < 0) { gtx_fail(msg, "[%s] ex_off descends at transcript %lld", who, (long long)i); return -2; }
        if (k >= ((int64_t)1 << 31)) { gtx_fail(msg, "[%s] transcript %lld has %lld exons (below 2^31)", who, (long long)i, (long long)k); return -2; }
    }
    return 0;
}

static int gtx_check_blocks(const l2r_gtx_blocks *b, std::string &msg, const char *who = "l2r_gtftext_blocks")
{
    if (!b) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    if (b->m < 0 || b->m > 0xfffffffell) { gtx_fail(msg, "[%s] %lld blocks (at most 2^32 - 2)", who, (long long)b->m); return -2; }
    return 0;
}

__host__ __device__ inline uint32_t gtx_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// the key of the k-th name of form READ; around a name stand ` <key> "` and `";`
static const char *const GTX_KEY[4] = {"gene_id", "transcript_id", "gene_name", "transcript_name"};

// One name by its id: GTX_OK and *len, or its error.  At most 255 bytes are looked at.
__host__ __device__ inline int gtx_name_len(const uint8_t *names, int64_t names_len, uint32_t id, uint32_t *len)
{
    if ((int64_t)id >= names_len) return GTX_E_NAME_ID;
    const int64_t room = names_len - (int64_t)id;
    const uint32_t look = room < L2R_GTX_NAME_MAX + 1 ? (uint32_t)room : (uint32_t)(L2R_GTX_NAME_MAX + 1);
    for (uint32_t k = 0; k < look; ++k) if (names[(size_t)id + k] == 0) { *len = k; return GTX_OK; }
    return look == (uint32_t)(L2R_GTX_NAME_MAX + 1) ? GTX_E_NAME_LONG : GTX_E_NAME_NUL;
}

// the bytes of the attribute text A from the four name lengths (PLAIN reads the first two)
__host__ __device__ inline uint32_t gtx_attr_len(int form, const uint32_t len[4])
{
    if (form == L2R_GTX_PLAIN) return 29u + len[0] + len[1];               // gene_id "";_transcript_id "";
    constexpr uint32_t key_len[4] = {7u, 13u, 9u, 15u};                     // gene_id transcript_id gene_name transcript_name
    uint32_t a = 0;
    for (int k = 0; k < 4; ++k) if (len[k]) a += 1u + key_len[k] + 2u + len[k] + 2u;
    return a ? a - 1u : 0u;
}
// the bytes of an exon line without its two numbers: <ref>\t<src>\texon\t . \t . \t.\t<+|->\t.\t <A> \n
__host__ __device__ inline uint32_t gtx_line_fix(uint32_t ref_len, uint32_t src_len, uint32_t attr_len) { return ref_len + 1u + src_len + 1u + 5u + 1u + 7u + attr_len + 1u; }
// what the transcript line has beyond an exon line with the same numbers: "transcript" for "exon", and <C>
__host__ __device__ inline uint32_t gtx_head_extra(int form, uint32_t cov) { return 6u + (form == L2R_GTX_READ ? 19u + gtx_digits(cov) : 0u); }

// Block q of the selection: its transcript, its names and its numbers, or the kind of its domain error.  xs == NULL in the rows: the
// caller supplies the chains (cx: ex_off / xs / xe of the last run, fetched for the host route).
struct GtxChains { const int64_t *ex_off; const int32_t *xs, *xe; };
struct GtxBlock { int64_t t, off; int64_t n; int32_t S, E, cov; uint32_t len[4], attr_len; };

static int gtx_block(const l2r_gtx_params *p, const l2r_gtx_rows *r, const GtxChains &cx, const l2r_gtx_blocks *b, int64_t q, GtxBlock &k)
{
    const int64_t t = b->sel ? (int64_t)b->sel[q] : q;
    if (t < 0 || t >= r->n) return GTX_E_SEL;
    k.t = t;
    if (r->tid[t] < 0 || r->tid[t] >= p->n_ref) return GTX_E_TID;
    k.off = cx.ex_off[t]; k.n = cx.ex_off[t + 1] - k.off;
    if (k.n < 1) return GTX_E_NOEXON;
    const uint32_t *col[4] = {r->gid, r->tids, r->gname, r->tname};
    for (int c = 0; c < (p->form == L2R_GTX_READ ? 4 : 2); ++c) {
        const int e = gtx_name_len(r->names, r->names_len, col[c][t], &k.len[c]);
        if (e) return e;
    }
    if (p->form == L2R_GTX_PLAIN) k.len[2] = k.len[3] = 0;
    k.attr_len = gtx_attr_len(p->form, k.len);
    k.S = b->start ? b->start[q] : cx.xs[k.off];
    k.E = b->end ? b->end[q] : cx.xe[k.off + k.n - 1];
    k.cov = b->cov ? b->cov[q] : 1;
    if (k.S < 0 || k.E < 0 || k.cov < 0) return GTX_E_NEG;
    return GTX_OK;
}
// exon j of a block as it is printed: the overrides stand for the first start and the last end
static inline int32_t gtx_xs(const GtxChains &cx, const GtxBlock &k, int64_t j) { return j == 0 ? k.S : cx.xs[k.off + j]; }
static inline int32_t gtx_xe(const GtxChains &cx, const GtxBlock &k, int64_t j) { return j == k.n - 1 ? k.E : cx.xe[k.off + j]; }

// The exact bytes and lines of block q, or the kind of its domain error (then *bytes and *lines are 0).
static int gtx_block_bytes(const l2r_gtx_params *p, const l2r_gtx_rows *r, const GtxChains &cx, const l2r_gtx_blocks *b, int64_t q, uint64_t *bytes, uint64_t *lines)
{
    *bytes = 0; *lines = 0;
    GtxBlock k;
    int e = gtx_block(p, r, cx, b, q, k);
    if (e) return e;
    const int32_t tid = r->tid[k.t];
    const uint32_t fix = gtx_line_fix((uint32_t)(p->ref_off[tid + 1] - p->ref_off[tid]), (uint32_t)p->src_len, k.attr_len);
    uint64_t sum = (uint64_t)fix + gtx_head_extra(p->form, (uint32_t)k.cov) + gtx_digits((uint32_t)k.S) + gtx_digits((uint32_t)k.E);
    for (int64_t j = 0; j < k.n; ++j) {
        const int32_t s = gtx_xs(cx, k, j), x = gtx_xe(cx, k, j);
        if (s < 0 || x < 0) return GTX_E_NEG;
        sum += (uint64_t)fix + gtx_digits((uint32_t)s) + gtx_digits((uint32_t)x);
    }
    if (sum >= GTX_BATCH_BYTES) return GTX_E_BIG;
    *bytes = sum; *lines = (uint64_t)k.n + 1u;
    return GTX_OK;
}

static inline void gtx_put_num(std::vector<uint8_t> &out, uint32_t v)
{
    char d[12];
    int n = 0;
    do { d[n++] = (char)('0' + v % 10u); v /= 10u; } while (v);
    while (n) out.push_back((uint8_t)d[--n]);
}
static inline void gtx_put_str(std::vector<uint8_t> &out, const char *s) { out.insert(out.end(), s, s + strlen(s)); }

// The exact routine on one core: the text of the blocks [first, first + count) appended to `out` (left as it was on an error),
// *n_lines = lines written.  0, or -1 and the error of the smallest bad block.
static int gtx_text_host(const l2r_gtx_params *p, const l2r_gtx_rows *r, const GtxChains &cx, const l2r_gtx_blocks *b, int64_t first, int64_t count,
                         std::vector<uint8_t> &out, int64_t *n_lines, std::string &msg)
{
    const size_t keep = out.size();
    const uint32_t *col[4] = {r->gid, r->tids, r->gname, r->tname};
    std::vector<uint8_t> head, tail;                        // <ref>\t<src>\t and \t.\t<+|->\t.\t<A>
    int64_t lines = 0;
    for (int64_t q = first; q < first + count; ++q) {
        GtxBlock k;
        uint64_t bytes = 0, nl = 0;
        const int e = gtx_block_bytes(p, r, cx, b, q, &bytes, &nl);
        if (e) { out.resize(keep); return gtx_block_fail(msg, q, e); }
        (void)gtx_block(p, r, cx, b, q, k);
        const int32_t tid = r->tid[k.t];
        const bool rev = r->rev[k.t] != 0;
        head.clear(); tail.clear();
        head.insert(head.end(), p->ref_names + p->ref_off[tid], p->ref_names + p->ref_off[tid + 1]);
        head.push_back('\t');
        head.insert(head.end(), p->src, p->src + p->src_len);
        head.push_back('\t');
        gtx_put_str(tail, "\t.\t"); tail.push_back(rev ? '-' : '+'); gtx_put_str(tail, "\t.\t");
        if (p->form == L2R_GTX_PLAIN) {
            gtx_put_str(tail, "gene_id \""); tail.insert(tail.end(), r->names + col[0][k.t], r->names + col[0][k.t] + k.len[0]);
            gtx_put_str(tail, "\"; transcript_id \""); tail.insert(tail.end(), r->names + col[1][k.t], r->names + col[1][k.t] + k.len[1]);
            gtx_put_str(tail, "\";");
        } else {
            bool any = false;
            for (int c = 0; c < 4; ++c) if (k.len[c]) {
                if (any) tail.push_back(' ');
                any = true;
                gtx_put_str(tail, GTX_KEY[c]); gtx_put_str(tail, " \"");
                tail.insert(tail.end(), r->names + col[c][k.t], r->names + col[c][k.t] + k.len[c]);
                gtx_put_str(tail, "\";");
            }
        }
        out.insert(out.end(), head.begin(), head.end());
        gtx_put_str(out, "transcript\t"); gtx_put_num(out, (uint32_t)k.S); out.push_back('\t'); gtx_put_num(out, (uint32_t)k.E);
        out.insert(out.end(), tail.begin(), tail.end());
        if (p->form == L2R_GTX_READ) { gtx_put_str(out, " transcript_cov \""); gtx_put_num(out, (uint32_t)k.cov); gtx_put_str(out, "\";"); }
        out.push_back('\n');
        for (int64_t i = 0; i < k.n; ++i) {
            const int64_t j = (p->form == L2R_GTX_READ && rev) ? k.n - 1 - i : i;
            out.insert(out.end(), head.begin(), head.end());
            gtx_put_str(out, "exon\t"); gtx_put_num(out, (uint32_t)gtx_xs(cx, k, j)); out.push_back('\t'); gtx_put_num(out, (uint32_t)gtx_xe(cx, k, j));
            out.insert(out.end(), tail.begin(), tail.end());
            out.push_back('\n');
        }
        lines += k.n + 1;
    }
    if (n_lines) *n_lines = lines;
    return 0;
}

}  // namespace l2r
