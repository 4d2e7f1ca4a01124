// l2r_summaryplan.hip.h -- the rule of l2r_summary_* (the read classes and unique counts of `update-gtf -y`), once, for the host and for the
// kernels of l2r_summary.hip.h: the class of a read, the merge key of the class-major concatenation, the argument checks, and
// summary_host, the exact routine on one core (L2R_SUMMARY_ROUTE=host, input that is not in order, and the comparator of
// tools/bench_summary.py).  No HIP call, no context, no environment.  tests/summary_dump.hip runs it as a stand-alone program for
// tests/test_summary_cpu.py.
//
// The rule (host/tail.c summary_and_bed; src/update_gtf.c:496-528 print_trans_summary).  Every read of the input belongs to one of four
// classes by its info word -- 0 known, 1 novel with reliable junctions only, 2 novel with an unreliable junction, 3 unrecognised -- and is
// offered, in input order, to its class's own merge_trans list (l2r_uniqplan.hip.h).  The summary wants the reads of every class and the
// length every list reaches.
//
// One list instead of four.  The reads in class-major order, input order inside a class, with the merge key
// tid' = class << 29 | tid, offered to ONE list give the verdicts of the four: an offer of class c can meet an entry of a lower class
// only as a stop (t.tid' > T.tid'), and a stop pushes -- which is what reaching the front of its own list does; entries of a higher class do
// not exist yet.  A class's unique count is the number of its offers that were pushed.  Hence the bound on tid: below 2^29.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "l2r_uniqplan.hip.h"

namespace l2r {

enum { SUM_CLASSES = 4, SUM_TID_BITS = 29 };
// kinds of a domain error (the smallest read that has one is named, and of its kinds the first)
enum { SUM_OK = 0, SUM_E_TID, SUM_E_NO_EXON, SUM_E_NEGATIVE, SUM_E_N };
// slots of l2r_summary_stats
enum { SMS_READS = 0, SMS_EXONS, SMS_ADDS, SMS_ROUTE, SMS_CLUSTERS, SMS_LARGEST, SMS_WAVE, SMS_K_CLASS, SMS_K_GATHER, SMS_K_CUT, SMS_K_MERGE, SMS_K_TAKE, SMS_N };

constexpr int64_t SUM_MAX_READS = (int64_t)1 << 31;                 // totals at or beyond: refused
constexpr int64_t SUM_MAX_EXONS = ((int64_t)1 << 32) - 64;

// host/tail.c:495-497.  L2R_INFO_FULL plays no part; KNOWN with UNREL is class 0.
__host__ __device__ inline int summary_class(uint32_t info)
{
    if (info & L2R_INFO_KNOWN) return 0;
    if (info & L2R_INFO_KNOWN_SITE) return (info & L2R_INFO_UNREL) ? 2 : 1;
    return 3;
}
__host__ __device__ inline bool summary_tid_ok(int32_t tid) { return tid >= 0 && tid < ((int32_t)1 << SUM_TID_BITS); }
__host__ __device__ inline int32_t summary_key(int cls, int32_t tid) { return (int32_t)((uint32_t)cls << SUM_TID_BITS | (uint32_t)tid); }

static int summary_read_fail(std::string &msg, int64_t read, int kind)
{
    static const char *const what[SUM_E_N] = {"", "a tid outside [0, 2^29)", "no exon", "a negative coordinate"};
    return uniq_fail(msg, "[l2r_summary_finish] read %lld: %s", (long long)read, what[kind > 0 && kind < SUM_E_N ? kind : 0]);
}

// the totals once `n` reads of `exons` exons have joined `have_n` reads of `have_x` exons
static int summary_check_totals(int64_t have_n, int64_t have_x, int64_t n, int64_t exons, std::string &msg)
{
    if (n < 0 || exons < 0) return uniq_fail(msg, "[l2r_summary_add] negative size");
    if (have_n + n >= SUM_MAX_READS) return uniq_fail(msg, "[l2r_summary_add] %lld reads in all (below 2^31)", (long long)(have_n + n));
    if (have_x + exons >= SUM_MAX_EXONS) return uniq_fail(msg, "[l2r_summary_add] %lld exons in all (below 2^32 - 64)", (long long)(have_x + exons));
    return 0;
}

// The arrays of an l2r_download as l2r_summary_add takes them: n reads, offsets that are the running sum of the exon counts in info
static int summary_check_result(int64_t n, const int32_t *tid, const l2r_result *res, std::string &msg)
{
    if (n < 0) return uniq_fail(msg, "[l2r_summary_add] negative size");
    if (n == 0) return 0;
    if (!tid) return uniq_fail(msg, "[l2r_summary_add] null tid");
    if (!res) return 0;
    if (res->n_reads != n) return uniq_fail(msg, "[l2r_summary_add] %lld reads, the results hold %lld", (long long)n, (long long)res->n_reads);
    if (!res->ex_off || !res->info || res->n_exons < 0 || (res->n_exons && (!res->ex_start || !res->ex_end))) return uniq_fail(msg, "[l2r_summary_add] null column");
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (res->ex_off[i] != at) return uniq_fail(msg, "[l2r_summary_add] ex_off is not the running sum of the exon counts at read %lld", (long long)i);
        at += (int64_t)L2R_INFO_NEXON(res->info[i]);
    }
    if (at != res->n_exons || res->ex_off[n] != at) return uniq_fail(msg, "[l2r_summary_add] the exon counts add up to %lld, the results hold %lld exons", (long long)at, (long long)res->n_exons);
    return 0;
}

// The reads in read order as the host routine takes them: read i has L2R_INFO_NEXON(info[i]) exons from ex_off[i] on
struct SummaryReads { int64_t n; const int32_t *tid; const uint32_t *info; const int64_t *ex_off; const int32_t *xs, *xe; };

// 0, or -1 and the smallest read outside the domain with its kind
static int summary_check(const SummaryReads &r, std::string &msg)
{
    for (int64_t i = 0; i < r.n; ++i) {
        if (!summary_tid_ok(r.tid[i])) return summary_read_fail(msg, i, SUM_E_TID);
        const int64_t k = (int64_t)L2R_INFO_NEXON(r.info[i]), off = r.ex_off[i];
        if (k == 0) return summary_read_fail(msg, i, SUM_E_NO_EXON);
        int32_t sign = 0;
        for (int64_t j = 0; j < k; ++j) sign |= r.xs[off + j] | r.xe[off + j];
        if (sign < 0) return summary_read_fail(msg, i, SUM_E_NEGATIVE);
    }
    return 0;
}

// The exact routine on one core, any input order: four uniq_host lists in read order.  counts[0..3]: the reads of every class,
// counts[4..7]: the entries of its list.  The arguments have passed summary_check.
static void summary_host(const SummaryReads &r, const UniqPrm &p, int64_t counts[8])
{
    for (int c = 0; c < SUM_CLASSES; ++c) {
        std::vector<int32_t> tid, xs, xe; std::vector<uint8_t> rev; std::vector<int64_t> off(1, 0);
        for (int64_t i = 0; i < r.n; ++i) {
            if (summary_class(r.info[i]) != c) continue;
            const int64_t k = (int64_t)L2R_INFO_NEXON(r.info[i]), o = r.ex_off[i];
            tid.push_back(r.tid[i]); rev.push_back((r.info[i] & L2R_INFO_REV) != 0);
            xs.insert(xs.end(), r.xs + o, r.xs + o + k); xe.insert(xe.end(), r.xe + o, r.xe + o + k);
            off.push_back(off.back() + k);
        }
        const l2r_uniq_trans t{(int64_t)tid.size(), tid.data(), rev.data(), off.data(), xs.data(), xe.data()};
        UniqResult res;
        uniq_host(&t, p, res);
        counts[c] = t.n; counts[SUM_CLASSES + c] = (int64_t)res.u_src.size();
    }
}

// The route test on the host (stats, tests): (tid', start) does not descend over the class-major concatenation, that is inside no class
static bool summary_in_order(const SummaryReads &r)
{
    uint64_t last[SUM_CLASSES] = {0, 0, 0, 0};
    for (int64_t i = 0; i < r.n; ++i) {
        const int c = summary_class(r.info[i]);
        const uint64_t key = uniq_key(r.tid[i], r.xs[r.ex_off[i]]);
        if (key < last[c]) return false;
        last[c] = key;
    }
    return true;
}

}  // namespace l2r
