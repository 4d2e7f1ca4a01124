// l2r_uniqplan.hip.h -- the rule of l2r_uniq_merge (`unique-gtf`), once, for the host and for the kernels of l2r_uniq.hip.h: the argument
// checks, the route test, the judgement of one offer against one list entry and the mutation of a hit as __host__ __device__ inline
// functions, the cluster cut on the host (stats and tests), and uniq_host, the exact routine on one core (input that is not in order,
// L2R_UNIQ_ROUTE=host, and the comparator of tools/bench_uniq.py).  No HIP call, no context, no environment.  tests/uniq_dump.hip runs it
// as a stand-alone program for tests/test_uniq_cpu.py.
//
// The rule (host/tail.c m_merge / chains_match; src/update_gtf.c:98-163 merge_trans, src/gtf.c:54-92 check_iden).  Transcripts are
// offered in input order to a list that starts empty.  An offer t scans the list from its newest entry T to its oldest:
//   stop       t.tid > T.tid or t.start > T.end: the scan ends, t is pushed (entries further back are never looked at, even one that
//              would match: the early stop)
//   skip       -s and the strands differ (behind the stop test: -s skips, it does not stop); single exon against multi exon, either way
//              (neither branch is taken); a judgement that finds nothing
//   single     both have one exon: |t.start - T.start| <= -D, |t.end - T.end| <= -D and the overlap fraction (a double divide, returned as
//              float) >= -f compared as float
//   identical  both have several and the same number: first starts within -D, every inner boundary within -d, last ends within -D
//   contained  both have several, different numbers: first starts within -D (!), the shorter one's first intron found among the longer
//              one's, the boundaries behind it within -d as far as both reach, last ends within -D (!); check_iden never answers 1, so
//              a longer t that contains T merges into T and is dropped (Q8).  The walk over the matched introns advances the OUTER index
//              and breaks: a second candidate position is never tried
// single and identical raise T's coverage by one, lower T's first start to t's and raise T's last end to t's; contained changes nothing.
// All three end the scan: t merged.  A scan that runs out of entries pushes t.  A pushed entry has t's chain, coverage 1; only its first
// start and its last end ever change, and only to the start / end of a later offer.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

enum { UNIQ_STOP = 0, UNIQ_SKIP, UNIQ_IDENT, UNIQ_CONTAINED, UNIQ_SINGLE };     // the verdict of one offer against one entry
// slots of l2r_uniq_stats
enum { UQS_ROWS = 0, UQS_UNIQUE, UQS_CLUSTERS, UQS_LARGEST, UQS_ROUTE, UQS_IDENT, UQS_CONTAINED, UQS_SINGLE, UQS_END_EXT, UQS_K_CUT, UQS_K_MERGE, UQS_K_TAKE, UQS_N };

struct UniqPrm { int32_t force_strand, ss_dis, end_dis; float frac; };
static inline UniqPrm uniq_prm(const l2r_params *p) { return UniqPrm{p->force_strand, p->ss_dis, p->end_dis, p->single_exon_ovlp_frac}; }

// A chain as the judgement reads it: exon j starts at (j == 0 ? first : xs[j]) and ends at (j == n - 1 ? last : xe[j]).  An offer has
// first = xs[0], last = xe[n - 1]; a list entry has the chain of the offer that created it and its two mutable words.
struct UniqChain { const int32_t *xs, *xe; int32_t n, first, last, tid; uint32_t rev; };
__host__ __device__ inline int32_t uniq_s(const UniqChain &c, int32_t j) { return j == 0 ? c.first : c.xs[j]; }
__host__ __device__ inline int32_t uniq_e(const UniqChain &c, int32_t j) { return j == c.n - 1 ? c.last : c.xe[j]; }
// (coordinates are not negative: the difference cannot overflow)
__host__ __device__ inline int32_t uniq_dist(int32_t a, int32_t b) { return a > b ? a - b : b - a; }

// src/update_gtf.c:80-89 exon_overlap_frac (Q6).  The kernels take overlap_frac of the classification kernels (l2r_kernels.hip.h, device
// only); the host the same arithmetic.
__host__ __device__ inline float uniq_frac(int32_t s1, int32_t e1, int32_t s2, int32_t e2)
{
#if defined(__HIP_DEVICE_COMPILE__) && defined(L2R_UNIQ_KERNELS)
    return overlap_frac(s1, e1, s2, e2);
#else
    if (s1 > e2 || s2 > e1) return 0.0f;
    const int32_t hi = e1 < e2 ? e1 : e2, lo = s1 > s2 ? s1 : s2;
    const int32_t l1 = e1 - s1 + 1, l2 = e2 - s2 + 1, mn = l1 < l2 ? l1 : l2;
    return (float)((double)(hi - lo + 1) / ((double)mn + 0.0));
#endif
}

// check_iden(t1 = a, t2 = b) for two chains of more than one exon: UNIQ_IDENT, UNIQ_CONTAINED or UNIQ_SKIP
__host__ __device__ inline int uniq_chains(const UniqChain &a, const UniqChain &b, int32_t ss, int32_t ed)
{
    if (a.n == b.n) {
        if (uniq_dist(a.first, b.first) > ed) return UNIQ_SKIP;
        for (int32_t i = 0; i + 1 < a.n; ++i) {
            if (uniq_dist(uniq_e(a, i), uniq_e(b, i)) > ss) return UNIQ_SKIP;
            if (uniq_dist(uniq_s(a, i + 1), uniq_s(b, i + 1)) > ss) return UNIQ_SKIP;
        }
        if (uniq_dist(a.last, b.last) > ed) return UNIQ_SKIP;
        return UNIQ_IDENT;
    }
    const bool a_long = a.n > b.n;
    const UniqChain l = a_long ? a : b, s = a_long ? b : a;     // (by value: references to one of two structs put them in scratch on the device)
    int verdict = UNIQ_SKIP;
    if (uniq_dist(l.first, s.first) > ed) return UNIQ_SKIP;
    for (int32_t i = 0; i + 1 < l.n; ++i) {
        if (uniq_dist(uniq_e(l, i), uniq_e(s, 0)) <= ss && uniq_dist(uniq_s(l, i + 1), uniq_s(s, 1)) <= ss) {
            verdict = UNIQ_CONTAINED;
            int32_t j = 1;
            for (i = i + 1; i + 1 < l.n && j + 1 < s.n; ++i, ++j) {
                if (uniq_dist(uniq_e(l, i), uniq_e(s, j)) > ss) return UNIQ_SKIP;
                if (uniq_dist(uniq_s(l, i + 1), uniq_s(s, j + 1)) > ss) return UNIQ_SKIP;
            }
            break;
        }
    }
    if (uniq_dist(l.last, s.last) > ed) return UNIQ_SKIP;
    return verdict;
}

// the offer t against the entry T
__host__ __device__ inline int uniq_judge(const UniqChain &t, const UniqChain &T, const UniqPrm &p)
{
    if (t.tid > T.tid || t.first > T.last) return UNIQ_STOP;
    if (p.force_strand && t.rev != T.rev) return UNIQ_SKIP;
    if (t.n == 1 && T.n == 1) {
        if (uniq_dist(t.first, T.first) > p.end_dis) return UNIQ_SKIP;
        if (uniq_dist(t.last, T.last) > p.end_dis) return UNIQ_SKIP;
        return uniq_frac(t.first, t.last, T.first, T.last) >= p.frac ? UNIQ_SINGLE : UNIQ_SKIP;
    }
    if (t.n > 1 && T.n > 1) return uniq_chains(t, T, p.ss_dis, p.end_dis);
    return UNIQ_SKIP;
}

// What a hit does to the entry's words (contained: nothing).  Returns 1 where the end was raised.
__host__ __device__ inline int uniq_apply(int verdict, const UniqChain &t, int32_t &T_first, int32_t &T_last, int32_t &T_cov)
{
    if (verdict != UNIQ_IDENT && verdict != UNIQ_SINGLE) return 0;
    ++T_cov;
    if (t.first < T_first) T_first = t.first;
    if (t.last > T_last) { T_last = t.last; return 1; }
    return 0;
}

// the keys of the route test and of the cluster cut: (tid + 1) in the high word (tid >= -1), a coordinate in the low one.  The sum is
// formed unsigned: tid -1 gives 0 and tid 2147483647 gives 0x80000000
__host__ __device__ inline uint64_t uniq_key(int32_t tid, int32_t coord) { return (uint64_t)((uint32_t)tid + 1u) << 32 | (uint32_t)coord; }

static int uniq_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// 0, or -1 and the text of l2r_last_error()
static int uniq_check(const l2r_uniq_trans *t, std::string &msg, const char *who = "l2r_uniq_merge")
{
    if (!t) return uniq_fail(msg, "[%s] null argument", who);
    if (t->n < 0) return uniq_fail(msg, "[%s] negative size", who);
    if (t->n >= ((int64_t)1 << 31)) return uniq_fail(msg, "[%s] %lld transcripts (below 2^31)", who, (long long)t->n);
    if (!t->ex_off) return uniq_fail(msg, "[%s] null ex_off", who);
    if (t->ex_off[0] != 0) return uniq_fail(msg, "[%s] ex_off does not start at 0", who);
    if (t->n == 0) return 0;
    if (!t->tid || !t->rev || !t->xs || !t->xe) return uniq_fail(msg, "[%s] null column", who);
    for (int64_t i = 0; i < t->n; ++i) {
        const int64_t k = t->ex_off[i + 1] - t->ex_off[i];
        if (k < 0) return uniq_fail(msg, "[%s] ex_off descends at transcript %lld", who, (long long)i);
        if (k == 0) return uniq_fail(msg, "[%s] transcript %lld has no exon", who, (long long)i);
        if (k >= ((int64_t)1 << 31)) return uniq_fail(msg, "[%s] transcript %lld has %lld exons (below 2^31)", who, (long long)i, (long long)k);
        if (t->tid[i] < -1) return uniq_fail(msg, "[%s] transcript %lld: tid %d", who, (long long)i, t->tid[i]);
    }
    const int64_t nx = t->ex_off[t->n];
    int32_t sign = 0;
    for (int64_t k = 0; k < nx; ++k) sign |= t->xs[k] | t->xe[k];
    if (sign < 0)
        for (int64_t i = 0; i < t->n; ++i)
            for (int64_t k = t->ex_off[i]; k < t->ex_off[i + 1]; ++k)
                if (t->xs[k] < 0 || t->xe[k] < 0) return uniq_fail(msg, "[%s] transcript %lld: a negative coordinate", who, (long long)i);
    return 0;
}

static inline int32_t uniq_start(const l2r_uniq_trans *t, int64_t i) { return t->xs[t->ex_off[i]]; }
static inline int32_t uniq_end(const l2r_uniq_trans *t, int64_t i) { return t->xe[t->ex_off[i + 1] - 1]; }
static inline UniqChain uniq_offer(const l2r_uniq_trans *t, int64_t i)
{
    const int64_t off = t->ex_off[i];
    const int32_t n = (int32_t)(t->ex_off[i + 1] - off);
    return UniqChain{t->xs + off, t->xe + off, n, t->xs[off], t->xe[off + n - 1], t->tid[i], (uint32_t)(t->rev[i] != 0)};
}

// the route test: (tid, start) does not descend over the input (k_uniq_heads makes the same test on the device)
static bool uniq_in_order(const l2r_uniq_trans *t)
{
    for (int64_t i = 1; i < t->n; ++i)
        if (uniq_key(t->tid[i], uniq_start(t, i)) < uniq_key(t->tid[i - 1], uniq_start(t, i - 1))) return false;
    return true;
}

// The cluster cut of input that is in order: head[i] = 1 where transcript i starts beyond every earlier end on its chromosome (or is the
// first of all).  Why clusters are independent: every T.end is the end of an earlier offer of T's chromosome, so the head h stops at the
// entry in front of it and is pushed; an offer behind h that scans as far as h's entry and beyond meets, in the entry in front, an end
// below h.start <= its own start and stops there -- by induction nothing behind h ever judges, or mutates, an entry in front of h.
static void uniq_clusters(const l2r_uniq_trans *t, std::vector<uint8_t> &head, int64_t *n_clusters, int64_t *largest)
{
    head.assign((size_t)t->n, 0);
    uint64_t reach = 0;
    int64_t n_c = 0, big = 0, first = 0;
    for (int64_t i = 0; i < t->n; ++i) {
        if (i == 0 || uniq_key(t->tid[i], uniq_start(t, i)) > reach) {
            head[(size_t)i] = 1; ++n_c;
            if (i - first > big) big = i - first;
            first = i;
        }
        const uint64_t e = uniq_key(t->tid[i], uniq_end(t, i));
        if (e > reach) reach = e;
    }
    if (t->n - first > big) big = t->n - first;
    *n_clusters = n_c; *largest = big;
}

struct UniqResult {
    std::vector<uint8_t> merged; std::vector<int32_t> uniq_of;              // per offer
    std::vector<int32_t> u_src, u_start, u_end, u_cov;                      // per entry, in list order
    int64_t hits[3] = {0, 0, 0}, end_ext = 0;                               // identical, contained, single; ends raised
};

// The exact routine on one core, any input order.  The arguments have passed uniq_check.
static void uniq_host(const l2r_uniq_trans *t, const UniqPrm &p, UniqResult &r)
{
    r = UniqResult();
    r.merged.assign((size_t)t->n, 0); r.uniq_of.assign((size_t)t->n, 0);
    for (int64_t i = 0; i < t->n; ++i) {
        const UniqChain c = uniq_offer(t, i);
        int verdict = UNIQ_STOP;
        int64_t k = (int64_t)r.u_src.size() - 1;
        for (; k >= 0; --k) {
            UniqChain T = uniq_offer(t, r.u_src[(size_t)k]);
            T.first = r.u_start[(size_t)k]; T.last = r.u_end[(size_t)k];
            verdict = uniq_judge(c, T, p);
            if (verdict != UNIQ_SKIP) break;
        }
        if (k < 0 || verdict == UNIQ_STOP) {
            r.uniq_of[(size_t)i] = (int32_t)r.u_src.size();
            r.u_src.push_back((int32_t)i); r.u_start.push_back(c.first); r.u_end.push_back(c.last); r.u_cov.push_back(1);
            continue;
        }
        r.merged[(size_t)i] = 1; r.uniq_of[(size_t)i] = (int32_t)k;
        r.end_ext += uniq_apply(verdict, c, r.u_start[(size_t)k], r.u_end[(size_t)k], r.u_cov[(size_t)k]);
        ++r.hits[verdict == UNIQ_IDENT ? 0 : verdict == UNIQ_CONTAINED ? 1 : 2];
    }
}

}  // namespace l2r
