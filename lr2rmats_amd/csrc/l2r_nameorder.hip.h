// l2r_nameorder.hip.h -- the host side of l2r_name_order (`sort -n`, `filter -N`, `fusion -N`): the argument checks, which pass before any
// column but the offsets is read and before anything is launched, and name_order_host, the exact routine the engine falls back to when
// both hash seeds of l2r_names.hip.h left a pair of neighbours with one hash and two names.  Host arithmetic only: no HIP call, no
// context, no environment.  tests/name_dump.hip runs both as a stand-alone program for tests/test_name_order_cpu.py.
//
// The name order (include/lr2rmats_hip.h): records with one name are consecutive, the groups follow each other by the input index of
// their first record, the records of a group keep their input order.  No equality with the output of any samtools release is claimed.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

static int name_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// 0, or -1 and the text of l2r_last_error().  Only r->n, the pointers themselves and name_off[0, n] are looked at.
static int name_check(const l2r_name_records *r, const uint32_t *order_out, const int64_t *n_groups, std::string &msg)
{
    if (!r || !n_groups) return name_fail(msg, "[l2r_name_order] null argument");
    if (r->n < 0) return name_fail(msg, "[l2r_name_order] %lld records", (long long)r->n);
    if (r->n > (int64_t)0xffffffffll - L2R_SORT_TILE)
        return name_fail(msg, "[l2r_name_order] %lld records: one order takes 2^32 - 1 - %d at most (the index of a record is a 32-bit word)", (long long)r->n, L2R_SORT_TILE);
    if (r->n == 0) return 0;
    if (!r->name_off || !r->names || !order_out) return name_fail(msg, "[l2r_name_order] null column");
    if (r->name_off[0] < 0) return name_fail(msg, "[l2r_name_order] name_off[0] = %lld: an offset is not negative", (long long)r->name_off[0]);
    for (int64_t i = 0; i < r->n; ++i) {
        const int64_t len = r->name_off[i + 1] - r->name_off[i];
        if (len < 0) return name_fail(msg, "[l2r_name_order] name_off descends at record %lld (%lld behind %lld)", (long long)i, (long long)r->name_off[i + 1], (long long)r->name_off[i]);
        if (len > L2R_NAME_MAX) return name_fail(msg, "[l2r_name_order] the name of record %lld has %lld bytes (%d at most)", (long long)i, (long long)len, L2R_NAME_MAX);
    }
    return 0;
}

// order[k] = the record at rank k of the name order, n words; returns the groups.  The records are sorted by (name bytes, length,
// index), so a run of one name starts with its smallest index; the runs are then placed as the device places them: a run's size at the
// slot of its first record, one exclusive sum over the slots, every record behind its run's base.
static int64_t name_order_host(int64_t n, const int64_t *off, const uint8_t *names, uint32_t *order)
{
    if (n <= 0) return 0;
    const size_t N = (size_t)n;
    std::vector<uint32_t> idx(N);
    for (size_t i = 0; i < N; ++i) idx[i] = (uint32_t)i;
    const auto cmp = [&](uint32_t a, uint32_t b) {          // <0, 0, >0 by bytes, then by length
        const int64_t la = off[a + (size_t)1] - off[a], lb = off[b + (size_t)1] - off[b];
        const int64_t m = la < lb ? la : lb;
        const int c = m ? memcmp(names + off[a], names + off[b], (size_t)m) : 0;
        return c ? c : (la < lb ? -1 : la > lb ? 1 : 0);
    };
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { const int c = cmp(a, b); return c ? c < 0 : a < b; });
    std::vector<uint32_t> base(N + 1, 0u), head_of(N);
    int64_t n_groups = 0;
    size_t h = 0;
    for (size_t k = 0; k < N; ++k) {
        if (k == 0 || cmp(idx[k - 1], idx[k]) != 0) { h = k; ++n_groups; }
        head_of[k] = (uint32_t)h;
        base[idx[h]] += 1u;
    }
    uint32_t sum = 0;
    for (size_t i = 0; i <= N; ++i) { const uint32_t t = base[i]; base[i] = sum; sum += t; }
    for (size_t k = 0; k < N; ++k) order[(size_t)base[idx[head_of[k]]] + (k - head_of[k])] = idx[k];
    return n_groups;
}

}  // namespace l2r
