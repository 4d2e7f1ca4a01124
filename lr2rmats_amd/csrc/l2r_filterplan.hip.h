// l2r_filterplan.hip.h -- the host half of `filter` and `fusion` (l2r_filter_score / l2r_filter_select / l2r_fusion_segments /
// l2r_fusion_select), once, for the engine and for a stand-alone program: the argument checks as functions that return the message,
// the table of the -r transcripts a record of every chromosome can meet (filter_spans_build) and the lookup in it (filter_span_hit,
// __host__ __device__: k_filter_score of l2r_filter.hip.h calls the same function).  No HIP call, no context, no environment.
// tests/filter_dump.hip runs it as a stand-alone program for tests/test_filter_plan_cpu.py.
//
// The table (reference src/bam_filter.c:48-59 remove_overlap).  The reference walks the transcripts of the -r GTF in FILE order, answers
// 1 at the first one of the record's tid that the record meets and stops at the first one of a LARGER tid.  So a record of tid v can meet
// the transcripts of tid v in front of first_gt[v], the first transcript (file order) with tid > v.  Per tid they are kept sorted by start
// with the running maximum of their ends: "some transcript with start <= hi and end >= lo" is one binary search.  A transcript of tid -1
// (a chromosome the header does not know) stops nothing and meets only a mapped record that has no chromosome either.
#pragma once
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

// n_tid = 1 + the largest tid (0 without a transcript of tid >= 0).  Chromosome v, -1 <= v < n_tid, owns the rows [off[v + 1], off[v + 2]) of
// start / pmax_end: off has n_tid + 2 words whatever the input, [0, 0] without a transcript.  The row of tid -1 is there because the reference
// compares tids as numbers: a mapped record without a chromosome (tid -1) meets the transcripts of tid -1 in front of the first one of a
// chromosome the header knows.  (BAM has no tid below -1; a transcript of such a tid meets nothing and stops nothing.)
struct FilterSpanTable { std::vector<int64_t> off; std::vector<int32_t> start, pmax_end; int32_t n_tid = 0; };

static void filter_spans_build(const l2r_filter_spans *rm, FilterSpanTable &t)
{
    t = FilterSpanTable();
    const int64_t n = rm && rm->n > 0 ? rm->n : 0;
    int32_t n_tid = 0;
    for (int64_t j = 0; j < n; ++j) n_tid = std::max(n_tid, rm->tid[j] + 1);
    // first_gt[v + 1]: first transcript (file order) with tid > v = where remove_overlap() stops for a record of tid v
    std::vector<int64_t> first_gt((size_t)n_tid + 1, n);
    int32_t seen = -1;                                 // largest tid so far
    for (int64_t j = 0; j < n; ++j) if (rm->tid[j] > seen) { for (int32_t v = seen; v < rm->tid[j]; ++v) first_gt[(size_t)(v + 1)] = std::min(first_gt[(size_t)(v + 1)], j); seen = rm->tid[j]; }
    std::vector<std::vector<std::pair<int32_t, int32_t>>> per((size_t)n_tid + 1);
    for (int64_t j = 0; j < n; ++j) { const int32_t v = rm->tid[j]; if (v >= -1 && j < first_gt[(size_t)(v + 1)]) per[(size_t)(v + 1)].push_back({rm->start[j], rm->end[j]}); }
    t.n_tid = n_tid;
    t.off.assign((size_t)n_tid + 2, 0);
    for (int32_t v = -1; v < n_tid; ++v) {
        auto &list = per[(size_t)(v + 1)];
        std::sort(list.begin(), list.end());
        int32_t run = INT32_MIN;
        for (auto &se : list) { run = std::max(run, se.second); t.start.push_back(se.first); t.pmax_end.push_back(run); }
        t.off[(size_t)(v + 2)] = (int64_t)t.start.size();
    }
}

// remove_overlap() for a record of chromosome `tid` that covers [lo, hi] (lo = pos, hi = pos + rlen - 1; the reference compares the
// 0-based position with 1-based transcript coordinates: kept as is): some transcript with end >= lo and start <= hi
__host__ __device__ inline bool filter_span_hit(const int64_t *off, const int32_t *start, const int32_t *pmax_end, int32_t n_tid, int32_t tid, int32_t lo, int32_t hi)
{
    if (tid < -1 || tid >= n_tid) return false;
    const int64_t a = off[tid + 1], b = off[tid + 2];
    int64_t l = a, r = b;                              // first index with start > hi
    while (l < r) { const int64_t m = (l + r) >> 1; if (start[m] <= hi) l = m + 1; else r = m; }
    return l > a && pmax_end[l - 1] >= lo;
}

static int filter_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// The argument checks of the four entry points: 0, or -1 and the text of l2r_last_error().  `ctx` is only tested against NULL.  Where the
// size is 0 the answer is 0 and the entry point returns at once, its outputs untouched.

// the columns of n records whose CIGAR words are cig[cig_off[i], cig_off[i + 1])
static int filter_cigar_check(const l2r_filter_records *r, bool columns_ok, std::string &msg, const char *who)
{
    if (!columns_ok || !r->cig_off || (r->n_cigar && !r->cig)) return filter_fail(msg, "[%s] null column", who);
    if (r->cig_off[0] != 0 || r->cig_off[r->n] != r->n_cigar) return filter_fail(msg, "[%s] cig_off does not span the CIGAR array", who);
    for (int64_t i = 0; i < r->n; ++i) if (r->cig_off[i + 1] < r->cig_off[i]) return filter_fail(msg, "[%s] cig_off descends at record %lld", who, (long long)i);
    return 0;
}

static int filter_score_check(const void *ctx, const l2r_filter_records *r, const l2r_filter_params *prm, const l2r_filter_spans *rm,
                              const void *drop, const void *score, const void *intron_n, std::string &msg)
{
    const char *who = "l2r_filter_score";
    if (!ctx || !r || !prm || !drop || !score || !intron_n) return filter_fail(msg, "[%s] null argument", who);
    if (r->n < 0 || r->n_cigar < 0) return filter_fail(msg, "[%s] negative size", who);
    if (r->n == 0) return 0;
    if (rm && rm->n > 0 && (!rm->tid || !rm->start || !rm->end)) return filter_fail(msg, "[%s] null span column", who);
    return filter_cigar_check(r, r->flag && r->tid && r->pos && r->l_qseq && r->nm, msg, who);
}

static int filter_groups_check(int64_t n_groups, const int64_t *group_off, std::string &msg, const char *who)
{
    if (group_off[0] < 0) return filter_fail(msg, "[%s] negative group offset", who);
    for (int64_t g = 0; g < n_groups; ++g) if (group_off[g + 1] <= group_off[g]) return filter_fail(msg, "[%s] group %lld is empty", who, (long long)g);
    return 0;
}

static int filter_select_check(const void *ctx, int64_t n_groups, const int64_t *group_off, const int32_t *score, const int32_t *intron_n,
                               const l2r_filter_params *prm, const void *winner, std::string &msg)
{
    const char *who = "l2r_filter_select";
    if (!ctx || !prm || n_groups < 0 || (n_groups && (!group_off || !score || !intron_n || !winner))) return filter_fail(msg, "[%s] bad argument", who);
    if (n_groups == 0) return 0;
    return filter_groups_check(n_groups, group_off, msg, who);
}

static int fusion_segments_check(const void *ctx, const l2r_fusion_records *r, const void *read_start, const void *read_end, const void *ref_start,
                                 const void *ref_end, const void *qlen, std::string &msg)
{
    const char *who = "l2r_fusion_segments";
    if (!ctx || !r || !read_start || !read_end || !ref_start || !ref_end || !qlen) return filter_fail(msg, "[%s] null argument", who);
    if (r->n < 0 || r->n_cigar < 0) return filter_fail(msg, "[%s] negative size", who);
    if (r->n == 0) return 0;
    return filter_cigar_check(r, r->flag && r->pos, msg, who);
}

static int fusion_select_check(const void *ctx, int64_t n_groups, const int64_t *group_off, const int32_t *score, const int32_t *ed, const int32_t *tid,
                               const int32_t *read_start, const int32_t *read_end, const int32_t *ref_start, const int32_t *ref_end,
                               const int32_t *rlen_of_group, const l2r_fusion_params *prm, const void *first, const void *second, std::string &msg)
{
    const char *who = "l2r_fusion_select";
    if (!ctx || !prm || n_groups < 0 || (n_groups && (!group_off || !score || !ed || !tid || !read_start || !read_end || !ref_start || !ref_end ||
                                                      !rlen_of_group || !first || !second))) return filter_fail(msg, "[%s] bad argument", who);
    if (n_groups == 0) return 0;
    return filter_groups_check(n_groups, group_off, msg, who);
}

}  // namespace l2r
