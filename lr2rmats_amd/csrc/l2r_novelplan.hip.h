// l2r_novelplan.hip.h -- the rule of l2r_novel_* (the novel list of `update-gtf`: the merged list U behind the updated GTF, novel_exon.bed and
// the "Updated information" block of summary.txt), once, for the host and for the kernels of l2r_novel.hip.h: the offer, split and known
// predicates, the item rules, the argument checks, the bytes of a BED line, the batch cut, and novel_host, the exact routine on one core
// (L2R_NOVEL_ROUTE=host, input that is not in order, and the comparator of tools/bench_novel.py).  No HIP call, no context, no
// environment.  tests/novel_dump.hip runs it as a stand-alone program for tests/test_novel_cpu.py.
//
// The rule is stated in include/lr2rmats_hip.h ("the novel list of update-gtf").  Two steps on both routes.  The selection
// (novel_select; k_nov_flag .. k_nov_chain) turns the reads of one add into what the accumulators hold: per offer its tid, strand, ref,
// global read index and exon count, its chain and flags one behind the other; per known read (tid, gene).  The finish (novel_host; the
// kernels behind l2r_novel_finish) merges the offers as ONE merge_trans list (l2r_uniqplan.hip.h), walks the entries' widened chains
// for the items of the six lists and keeps the first item of every key.  novel_host does the latter with the literal backward scans of
// host/tail.c summary_and_bed / add_gene, which stop at a smaller tid; with tid not descending -- the device route's condition -- a scan
// that stops has passed every item of its tid, and "no equal key in front" is what the kernels compute by sorting.  The gene lists
// need one thing more, because add_gene compares the gene before it tests the stop: novel_gene_rows.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "l2r_gtftextplan.hip.h"
#include "l2r_uniqplan.hip.h"

namespace l2r {

// the six lists, in the order of their items and kept rows
enum { NOV_EXON = 0, NOV_DON, NOV_ACC, NOV_JUNC, NOV_GENE, NOV_KNOWN_GENE, NOV_LISTS };
enum { NOV_TYPE_T = 0, NOV_TYPE_I, NOV_TYPE_S };        // an exon row's type: meta = type | rev << 2
enum { NOV_TID_BITS = 29 };                             // a sort key's top word is list << 29 | tid
// kinds of a domain error (the smallest read that has one is named, and of its kinds the first)
enum { NOV_OK = 0, NOV_E_TID, NOV_E_NO_EXON, NOV_E_REF, NOV_E_NEGATIVE, NOV_E_N };
// slots of l2r_novel_stats
enum { NVS_READS = 0, NVS_OFFERS, NVS_SPLIT, NVS_KNOWN, NVS_ADDS, NVS_ROUTE, NVS_CLUSTERS, NVS_LARGEST, NVS_ENTRIES, NVS_HITS, NVS_WIDENED, NVS_ITEMS, NVS_KEPT = NVS_ITEMS + NOV_LISTS,
       NVS_WAVE = NVS_KEPT + NOV_LISTS, NVS_GUARD, NVS_K_SELECT, NVS_K_MERGE, NVS_K_ITEMS, NVS_K_SORT, NVS_K_KEEP, NVS_K_MEASURE, NVS_K_SCAN, NVS_K_WRITE, NVS_N };
static_assert(NVS_ITEMS == 11 && NVS_KEPT == 17 && NVS_WAVE == 23 && NVS_GUARD == 24, "l2r_novel_stats: the words of include/lr2rmats_hip.h");

constexpr int64_t NOV_MAX_READS = (int64_t)1 << 31;                 // totals at or beyond: refused (as l2r_summary_add)
constexpr int64_t NOV_MAX_EXONS = ((int64_t)1 << 32) - 64;
constexpr int64_t NOV_MAX_ITEMS = ((int64_t)1 << 32) - 64;          // the items of the six lists together

struct NovelPrm { int32_t n_ref; int64_t n_tx; uint32_t na_gene; int32_t has_sj, split; };

// host/tail.c read_route: T_NOVEL_WHOLE, T_NOVEL_SPLIT; the known reads of summary_and_bed (KNOWN, whether FULL or not)
__host__ __device__ inline bool novel_candidate(uint32_t info) { return (info & L2R_INFO_FULL) && !(info & L2R_INFO_KNOWN) && (info & L2R_INFO_KNOWN_SITE); }
__host__ __device__ inline bool novel_offer(uint32_t info, int has_sj) { return novel_candidate(info) && (!has_sj || (info & L2R_INFO_SJ_PASS)); }
__host__ __device__ inline bool novel_split(uint32_t info, int has_sj, int split) { return novel_candidate(info) && has_sj && !(info & L2R_INFO_SJ_PASS) && split; }
__host__ __device__ inline bool novel_known(uint32_t info) { return (info & L2R_INFO_KNOWN) != 0; }
// gene(): the ordinal of the gene-id string of annotation transcript ref; NA's where ref < 0
__host__ __device__ inline uint32_t novel_gene(int32_t ref, const uint32_t *tx_gene, uint32_t na_gene) { return ref < 0 ? na_gene : tx_gene[ref]; }
// the type of exon j of n
__host__ __device__ inline int novel_exon_type(uint32_t j, uint32_t n) { return n > 1u ? ((j == 0u || j == n - 1u) ? NOV_TYPE_T : NOV_TYPE_I) : NOV_TYPE_S; }
// The per-read kinds of a domain error (a negative coordinate is looked for in the chains of the offers, behind these)
__host__ __device__ inline int novel_read_kind(int32_t tid, uint32_t info, int32_t ref, int32_t n_ref, int64_t n_tx)
{
    if (tid < 0 || tid >= n_ref) return NOV_E_TID;
    if (L2R_INFO_NEXON(info) == 0) return NOV_E_NO_EXON;
    if ((int64_t)ref >= n_tx) return NOV_E_REF;
    return NOV_OK;
}

static int novel_read_fail(std::string &msg, int64_t read, int kind)
{
    static const char *const what[NOV_E_N] = {"", "a tid outside the reference table", "no exon", "ref at or beyond the annotation's transcripts", "a negative coordinate"};
    return uniq_fail(msg, "[l2r_novel_finish] read %lld: %s", (long long)read, what[kind > 0 && kind < NOV_E_N ? kind : 0]);
}

// l2r_novel_begin: 0, or -1 and the text
static int novel_check_begin(const l2r_params *prm, int32_t n_ref, const int64_t *ref_off, const uint8_t *ref_names, int64_t n_tx, const uint32_t *tx_gene, std::string &msg)
{
    if (!prm) return uniq_fail(msg, "[l2r_novel_begin] null argument");
    if (n_ref < 1 || n_ref > ((int32_t)1 << NOV_TID_BITS)) return uniq_fail(msg, "[l2r_novel_begin] %d references (1 .. 2^29)", n_ref);
    if (!ref_off) return uniq_fail(msg, "[l2r_novel_begin] null ref_off");
    if (text_check_ref_off(n_ref, ref_off, ref_names, msg, "l2r_novel_begin")) return -1;
    if (n_tx < 0 || n_tx >= ((int64_t)1 << 31)) return uniq_fail(msg, "[l2r_novel_begin] %lld annotation transcripts (below 2^31)", (long long)n_tx);
    if (n_tx > 0 && !tx_gene) return uniq_fail(msg, "[l2r_novel_begin] null tx_gene");
    return 0;
}

// the totals once `n` reads of `exons` exons have joined `have_n` reads of `have_x` exons
static int novel_check_totals(int64_t have_n, int64_t have_x, int64_t n, int64_t exons, std::string &msg)
{
    if (n < 0 || exons < 0) return uniq_fail(msg, "[l2r_novel_add] negative size");
    if (have_n + n >= NOV_MAX_READS) return uniq_fail(msg, "[l2r_novel_add] %lld reads in all (below 2^31)", (long long)(have_n + n));
    if (have_x + exons >= NOV_MAX_EXONS) return uniq_fail(msg, "[l2r_novel_add] %lld exons in all (below 2^32 - 64)", (long long)(have_x + exons));
    return 0;
}

// The arrays of an l2r_download as l2r_novel_add takes them: n reads, offsets that are the running sum of the exon counts in info
static int novel_check_result(int64_t n, const int32_t *tid, const l2r_result *res, std::string &msg)
{
    if (n < 0) return uniq_fail(msg, "[l2r_novel_add] negative size");
    if (n == 0) return 0;
    if (!tid) return uniq_fail(msg, "[l2r_novel_add] null tid");
    if (!res) return 0;
    if (res->n_reads != n) return uniq_fail(msg, "[l2r_novel_add] %lld reads, the results hold %lld", (long long)n, (long long)res->n_reads);
    if (!res->ex_off || !res->info || !res->ref_tx || res->n_exons < 0 || (res->n_exons && (!res->ex_start || !res->ex_end || !res->ex_flag))) return uniq_fail(msg, "[l2r_novel_add] null column");
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (res->ex_off[i] != at) return uniq_fail(msg, "[l2r_novel_add] ex_off is not the running sum of the exon counts at read %lld", (long long)i);
        at += (int64_t)L2R_INFO_NEXON(res->info[i]);
    }
    if (at != res->n_exons || res->ex_off[n] != at) return uniq_fail(msg, "[l2r_novel_add] the exon counts add up to %lld, the results hold %lld exons", (long long)at, (long long)res->n_exons);
    return 0;
}

// What the accumulators hold (the host's copy: the host route, and the device's fetched for novel_host)
struct NovelAcc {
    int64_t reads = 0, split = 0;
    int64_t bad = -1; int bad_kind = NOV_OK;                            // the smallest read outside the domain
    std::vector<int32_t> o_tid, o_ref, o_read; std::vector<uint8_t> o_rev; std::vector<uint32_t> o_nex;      // per offer
    std::vector<int32_t> xs, xe; std::vector<uint8_t> f;               // the offers' chains, one behind the other
    std::vector<int32_t> k_tid; std::vector<uint32_t> k_gene;          // per known read
};

static void novel_note_bad(NovelAcc &a, int64_t read, int kind) { if (a.bad < 0 || read < a.bad) { a.bad = read; a.bad_kind = kind; } }

// The selection over the n reads of one add (the arguments have passed novel_check_result)
static void novel_select(NovelAcc &a, const NovelPrm &p, const uint32_t *tx_gene, int64_t n, const int32_t *tid, const l2r_result *res)
{
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t info = res->info[i], k = L2R_INFO_NEXON(info);
        const int32_t ref = res->ref_tx[i];
        const int64_t read = a.reads + i, off = res->ex_off[i];
        const int kind = novel_read_kind(tid[i], info, ref, p.n_ref, p.n_tx);
        if (kind) { novel_note_bad(a, read, kind); continue; }
        if (novel_split(info, p.has_sj, p.split)) ++a.split;
        if (novel_known(info)) { a.k_tid.push_back(tid[i]); a.k_gene.push_back(novel_gene(ref, tx_gene, p.na_gene)); }
        if (!novel_offer(info, p.has_sj)) continue;
        int32_t sign = 0;
        for (uint32_t j = 0; j < k; ++j) sign |= res->ex_start[off + j] | res->ex_end[off + j];
        if (sign < 0) { novel_note_bad(a, read, NOV_E_NEGATIVE); continue; }
        a.o_tid.push_back(tid[i]); a.o_ref.push_back(ref); a.o_read.push_back((int32_t)read); a.o_rev.push_back((info & L2R_INFO_REV) != 0); a.o_nex.push_back(k);
        a.xs.insert(a.xs.end(), res->ex_start + off, res->ex_start + off + k); a.xe.insert(a.xe.end(), res->ex_end + off, res->ex_end + off + k);
        a.f.insert(a.f.end(), res->ex_flag + off, res->ex_flag + off + k);
    }
    a.reads += n;
}

// What l2r_novel_finish leaves: the entries and, per list, the kept rows in the order of first appearance.  A row is (tid, a, b): exon
// (start, end), site (coordinate, 0), junction (donor, acceptor), gene (ordinal, 0); exon rows have a score and meta.
struct NovelRows { std::vector<int32_t> tid, a, b, score; std::vector<uint8_t> meta; };
struct NovelOut {
    UniqResult u;
    std::vector<int32_t> e_src, e_start, e_end, e_cov;                 // per entry: the read that created it, the widened ends, the coverage
    NovelRows rows[NOV_LISTS];
    int64_t items[NOV_LISTS] = {0, 0, 0, 0, 0, 0};
    int64_t widened = 0, clusters = 0, largest = 0;
    bool in_order = false;
};

// counts[0..7] in the order of h_write_summary_text: genes, entries, 0 (no piece entries), exons, sites, junctions, 0, known genes
static void novel_counts(const int64_t kept[NOV_LISTS], int64_t entries, int64_t counts[8])
{
    counts[0] = kept[NOV_GENE]; counts[1] = entries; counts[2] = 0; counts[3] = kept[NOV_EXON]; counts[4] = kept[NOV_DON] + kept[NOV_ACC];
    counts[5] = kept[NOV_JUNC]; counts[6] = 0; counts[7] = kept[NOV_KNOWN_GENE];
}

static l2r_uniq_trans novel_trans(const NovelAcc &a, std::vector<int64_t> &off)
{
    const size_t N = a.o_tid.size();
    off.assign(N + 1, 0);
    for (size_t o = 0; o < N; ++o) off[o + 1] = off[o] + (int64_t)a.o_nex[o];
    return l2r_uniq_trans{(int64_t)N, a.o_tid.data(), a.o_rev.data(), off.data(), a.xs.data(), a.xe.data()};
}

// The route test: (tid, start) does not descend over the offers, tid does not descend over the known reads
static bool novel_in_order(const NovelAcc &a)
{
    std::vector<int64_t> off;
    const l2r_uniq_trans t = novel_trans(a, off);
    if (!uniq_in_order(&t)) return false;
    for (size_t i = 1; i < a.k_tid.size(); ++i) if (a.k_tid[i] < a.k_tid[i - 1]) return false;
    return true;
}

// one backward scan of summary_and_bed: an equal key first, then the stop at a smaller tid.  The row that holds the key, or -1
static int64_t novel_find(const NovelRows &r, int32_t tid, int32_t a, int32_t b)
{
    for (int64_t k = (int64_t)r.tid.size() - 1; k >= 0; --k) {
        if (r.tid[(size_t)k] == tid && r.a[(size_t)k] == a && r.b[(size_t)k] == b) return k;
        if (tid > r.tid[(size_t)k]) break;
    }
    return -1;
}
// add_gene compares the gene first, whatever the tid, then stops
static int64_t novel_find_gene(const NovelRows &r, int32_t tid, int32_t gene)
{
    for (int64_t k = (int64_t)r.tid.size() - 1; k >= 0; --k) {
        if (r.a[(size_t)k] == gene) return k;
        if (tid > r.tid[(size_t)k]) break;
    }
    return -1;
}
static void novel_push(NovelRows &r, int32_t tid, int32_t a, int32_t b, int32_t score, uint8_t meta)
{
    r.tid.push_back(tid); r.a.push_back(a); r.b.push_back(b); r.score.push_back(score); r.meta.push_back(meta);
}

// What add_gene's order of tests adds to "the first item of every (tid, gene)", with tid not descending: the scan of an item compares the
// gene with every kept row of its own tid and then, BEFORE it stops there, with the last kept row of a smaller tid -- a gene that is the
// newest row when its chromosome ends is not counted again on the next one.  In: the first items of every (tid, gene) in order of
// first appearance, as the kernels leave them.  Out: the rows add_gene keeps.  One pass; a row that goes takes no part later.
static void novel_gene_rows(NovelRows &r)
{
    size_t kept = 0;
    bool have_edge = false; int32_t edge = 0, cur = 0;     // the gene of the newest kept row of a smaller tid
    for (size_t k = 0; k < r.tid.size(); ++k) {
        if (k == 0 || r.tid[k] != cur) { cur = r.tid[k]; have_edge = kept > 0; if (kept) edge = r.a[kept - 1]; }
        if (have_edge && r.a[k] == edge) continue;
        r.tid[kept] = r.tid[k]; r.a[kept] = r.a[k]; r.b[kept] = r.b[k]; r.score[kept] = r.score[k]; r.meta[kept] = r.meta[k];
        ++kept;
    }
    r.tid.resize(kept); r.a.resize(kept); r.b.resize(kept); r.score.resize(kept); r.meta.resize(kept);
}

// The exact routine on one core, any input order: uniq_host over the offers, then the literal backward scans (a gene list compares the
// gene first, whatever the tid).  The accumulators hold no read outside the domain.
static void novel_host(const NovelAcc &a, const UniqPrm &p, const uint32_t *tx_gene, uint32_t na_gene, NovelOut &out)
{
    out = NovelOut();
    std::vector<int64_t> off;
    const l2r_uniq_trans t = novel_trans(a, off);
    uniq_host(&t, p, out.u);
    out.in_order = novel_in_order(a);
    if (out.in_order && t.n) { std::vector<uint8_t> head; uniq_clusters(&t, head, &out.clusters, &out.largest); }
    const size_t U = out.u.u_src.size();
    std::vector<int32_t> xs, xe;
    for (size_t e = 0; e < U; ++e) {
        const size_t o = (size_t)out.u.u_src[e];
        const int64_t x0 = off[o]; const uint32_t n = a.o_nex[o];
        const int32_t tid = a.o_tid[o], cov = out.u.u_cov[e];
        const uint8_t rev = a.o_rev[o];
        out.e_src.push_back(a.o_read[o]); out.e_start.push_back(out.u.u_start[e]); out.e_end.push_back(out.u.u_end[e]); out.e_cov.push_back(cov);
        xs.assign(a.xs.begin() + x0, a.xs.begin() + x0 + n); xe.assign(a.xe.begin() + x0, a.xe.begin() + x0 + n);
        if (xs[0] != out.u.u_start[e] || xe[n - 1] != out.u.u_end[e]) ++out.widened;
        xs[0] = out.u.u_start[e]; xe[n - 1] = out.u.u_end[e];
        const uint8_t *f = a.f.data() + x0;
        ++out.items[NOV_GENE];
        {   const int32_t g = (int32_t)novel_gene(a.o_ref[o], tx_gene, na_gene);
            if (novel_find_gene(out.rows[NOV_GENE], tid, g) < 0) novel_push(out.rows[NOV_GENE], tid, g, 0, 0, 0); }
        for (uint32_t j = 0; j < n; ++j) if (f[j] & L2R_EXF_NOVEL_EXON) {
            ++out.items[NOV_EXON];
            const int64_t k = novel_find(out.rows[NOV_EXON], tid, xs[j], xe[j]);
            if (k >= 0) out.rows[NOV_EXON].score[(size_t)k] += cov;
            else novel_push(out.rows[NOV_EXON], tid, xs[j], xe[j], cov, (uint8_t)(novel_exon_type(j, n) | rev << 2));
        }
        for (uint32_t j = 0; j + 1 < n; ++j) if (f[j] & L2R_EXF_NOVEL_DON) {
            ++out.items[NOV_DON];
            if (novel_find(out.rows[NOV_DON], tid, xe[j], 0) < 0) novel_push(out.rows[NOV_DON], tid, xe[j], 0, 0, 0);
        }
        for (uint32_t j = 0; j + 1 < n; ++j) if (f[j] & L2R_EXF_NOVEL_ACC) {
            ++out.items[NOV_ACC];
            if (novel_find(out.rows[NOV_ACC], tid, xs[j + 1], 0) < 0) novel_push(out.rows[NOV_ACC], tid, xs[j + 1], 0, 0, 0);
        }
        for (uint32_t j = 0; j + 1 < n; ++j) if (f[j] & L2R_EXF_NOVEL_JUNC) {
            ++out.items[NOV_JUNC];
            if (novel_find(out.rows[NOV_JUNC], tid, xe[j], xs[j + 1]) < 0) novel_push(out.rows[NOV_JUNC], tid, xe[j], xs[j + 1], 0, 0);
        }
    }
    out.items[NOV_KNOWN_GENE] = (int64_t)a.k_tid.size();
    for (size_t i = 0; i < a.k_tid.size(); ++i)
        if (novel_find_gene(out.rows[NOV_KNOWN_GENE], a.k_tid[i], (int32_t)a.k_gene[i]) < 0) novel_push(out.rows[NOV_KNOWN_GENE], a.k_tid[i], (int32_t)a.k_gene[i], 0, 0, 0);
}

// ---- the BED line of a kept exon row: <ref>\t<start - 1>\t<end>\t<T|I|S>_exon\t<score>\t<+|->\n, numbers as %d
static uint32_t novel_digits(int64_t v) { uint32_t d = v < 0 ? 2u : 1u; for (v = v < 0 ? -v : v; v >= 10; v /= 10) ++d; return d; }
static uint32_t novel_bed_bytes(const int64_t *ref_off, int32_t tid, int32_t start, int32_t end, int32_t score)
{
    return (uint32_t)(ref_off[tid + 1] - ref_off[tid]) + novel_digits((int64_t)start - 1) + novel_digits(end) + novel_digits(score) + 13u;
}
static void novel_bed_line(std::vector<uint8_t> &text, const int64_t *ref_off, const uint8_t *ref_names, int32_t tid, int32_t start, int32_t end, int32_t score, uint8_t meta)
{
    char buf[96];
    text.insert(text.end(), ref_names + ref_off[tid], ref_names + ref_off[tid + 1]);
    const int k = snprintf(buf, sizeof buf, "\t%d\t%d\t%c_exon\t%d\t%c\n", start - 1, end, "TIS"[meta & 3u], score, "+-"[(meta >> 2) & 1u]);
    text.insert(text.end(), buf, buf + k);
}
// the rows [first, first + take) as text
static void novel_bed_host(const NovelRows &r, const int64_t *ref_off, const uint8_t *ref_names, int64_t first, int64_t take, std::vector<uint8_t> &text)
{
    text.clear();
    for (int64_t q = first; q < first + take; ++q) novel_bed_line(text, ref_off, ref_names, r.tid[(size_t)q], r.a[(size_t)q], r.b[(size_t)q], r.score[(size_t)q], r.meta[(size_t)q]);
}
// the batch cut over the measured lines of l2r_novel_lines
static int novel_cut(const uint32_t *len, int64_t m, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_take, int64_t *n_bytes, std::string &msg)
{ return batch_cut(len, m, first, max_rows, max_bytes, n_take, n_bytes, msg, "l2r_novel_lines", "row"); }

}  // namespace l2r
