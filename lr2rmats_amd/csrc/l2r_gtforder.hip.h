// l2r_gtforder.hip.h -- the host side of l2r_gtf_order (`sort-gtf`, `sort-gtf-check`): the argument checks, the chromosome ranking of the
// heads the device sends (l2r_gtf.hip.h), the text of a domain error, and gtf_order_host, the exact routine over the whole text with
// 64-bit offsets that the engine takes where the text or the rows are beyond one device call, and that `sort-gtf-check` runs.  Host
// arithmetic only: no HIP call, no context, no environment.  tests/gtf_dump.hip runs it as a stand-alone program for
// tests/test_gtf_order_cpu.py.
//
// The order (include/lr2rmats_hip.h).  Lines end at '\n', a last line without one counts, line numbers start at 1.  Fields are runs of
// bytes that are neither space nor tab.  A line is KEPT iff its byte 0 is not '#' and its third field contains "transcript" or equals
// "exon"; it is a TRANSCRIPT line iff that field equals "transcript".  A transcript line sets the current key (c, s, e): s and e its
// fourth and fifth fields as decimal numbers, c the rank of its first field -- chr1..chr22 1..22, chrX 23, chrY 24, chrM 25, any other
// name 26, 27, ... by its first appearance on a transcript line.  Every kept line carries the current key, (0, 0, 0) before the first
// transcript line, and the kept lines are ordered by (c, s, e, line number).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

constexpr uint32_t GTF_TABLE_NAMES = 25;                 // chr1..chr22, chrX, chrY, chrM

static int gtf_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// 0, or -1 and the text of l2r_last_error().  Only the size and the pointers themselves are looked at.
static int gtf_check(const l2r_gtf_text *t, const int64_t *n_rows, std::string &msg)
{
    if (!t || !n_rows) return gtf_fail(msg, "[l2r_gtf_order] null argument");
    if (t->n_bytes < 0) return gtf_fail(msg, "[l2r_gtf_order] %lld bytes of text", (long long)t->n_bytes);
    if (t->n_bytes > 0 && !t->text) return gtf_fail(msg, "[l2r_gtf_order] null text of %lld bytes", (long long)t->n_bytes);
    return 0;
}

// The route of a text: the device takes texts below 2^32 - 64 bytes (every offset, and the offset behind the last byte, is a 32-bit word)
static bool gtf_text_fits_device(int64_t n_bytes) { return n_bytes < (int64_t)0xffffffffll - 63; }
// ... and as many kept rows as one sort takes
static bool gtf_rows_fit_device(int64_t n_rows) { return n_rows <= (int64_t)0xffffffffll - L2R_SORT_TILE; }

static inline bool gtf_blank(uint8_t b) { return b == ' ' || b == '\t'; }

// The rank of a transcript line's first field: the fixed table, then 26, 27, ... in the order rank() first sees a name.
struct GtfChrRanks {
    std::unordered_map<std::string, uint32_t> seen;
    uint32_t beyond = 0;                                 // distinct names ranked beyond the table
    uint32_t table_seen = 0;                             // bit r: the table name of rank r was ranked
    static uint32_t table(const uint8_t *s, size_t len)
    {
        if (len < 4 || len > 5 || memcmp(s, "chr", 3) != 0) return 0;
        if (len == 4) {
            if (s[3] >= '1' && s[3] <= '9') return (uint32_t)(s[3] - '0');
            return s[3] == 'X' ? 23u : s[3] == 'Y' ? 24u : s[3] == 'M' ? 25u : 0u;
        }
        if (s[3] < '1' || s[3] > '2' || s[4] < '0' || s[4] > '9') return 0;
        const uint32_t v = (uint32_t)(s[3] - '0') * 10u + (uint32_t)(s[4] - '0');
        return v <= 22u ? v : 0u;
    }
    int64_t distinct() const { return (int64_t)__builtin_popcount(table_seen) + (int64_t)beyond; }
    uint32_t rank(const uint8_t *s, size_t len)
    {
        const uint32_t t = table(s, len);
        if (t) { table_seen |= 1u << t; return t; }
        const auto at = seen.emplace(std::string((const char *)s, len), GTF_TABLE_NAMES + 1u + beyond);
        if (at.second) ++beyond;
        return at.first->second;
    }
};

// The heads the device compacted (a transcript whose first field differs from the previous transcript's), in line order: rank[h].
// Every first appearance of a name is a head, so the ranks are those of the whole text.  -1: a head reaches beyond the text.
static int gtf_rank_heads(const uint8_t *text, uint64_t n_bytes, const uint32_t *off, const uint32_t *len, size_t n_heads, uint32_t *rank, GtfChrRanks &ranks)
{
    for (size_t h = 0; h < n_heads; ++h) {
        if ((uint64_t)off[h] + len[h] > n_bytes) return -1;
        rank[h] = ranks.rank(text + off[h], len[h]);
    }
    return 0;
}

// The head of one line: what k_gtf_fields makes of it.
struct GtfLine {
    bool kept = false, tx = false, bad = false;
    uint64_t f1 = 0, f1_len = 0;                         // field 1 (transcript lines)
    uint32_t s = 0, e = 0;
    int why = 0;                                         // bad: 1 fewer than five fields, 2 the fourth field, 3 the fifth
};

// value of the decimal digits [p, q), false where they are none, not all digits, or above 4294967295
static bool gtf_number(const uint8_t *p, const uint8_t *q, uint32_t *out)
{
    if (p >= q) return false;
    uint64_t v = 0;
    for (; p < q; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10u + (uint64_t)(*p - '0');
        if (v > 0xffffffffull) return false;
    }
    *out = (uint32_t)v;
    return true;
}

static GtfLine gtf_line(const uint8_t *text, uint64_t b, uint64_t e)
{
    GtfLine r;
    if (b < e && text[b] == '#') return r;
    uint64_t fs[5], fe[5];
    int nf = 0;
    for (uint64_t p = b; nf < 5;) {
        while (p < e && gtf_blank(text[p])) ++p;
        if (p >= e) break;
        fs[nf] = p;
        while (p < e && !gtf_blank(text[p])) ++p;
        fe[nf++] = p;
    }
    if (nf < 3) return r;
    const uint8_t *t = text + fs[2];
    const uint64_t tl = fe[2] - fs[2];
    static const char word[] = "transcript";
    bool has = false;
    for (uint64_t k = 0; k + 10 <= tl && !has; ++k) has = memcmp(t + k, word, 10) == 0;
    r.kept = has || (tl == 4 && memcmp(t, "exon", 4) == 0);
    r.tx = has && tl == 10;
    if (!r.tx) return r;
    r.f1 = fs[0]; r.f1_len = fe[0] - fs[0];
    if (nf < 5) { r.bad = true; r.why = 1; return r; }
    if (!gtf_number(text + fs[3], text + fe[3], &r.s)) { r.bad = true; r.why = 2; }
    else if (!gtf_number(text + fs[4], text + fe[4], &r.e)) { r.bad = true; r.why = 3; }
    return r;
}

// The error of the smallest bad line, for both routes: `line` is 1-based, [b, e) its bytes.
static int gtf_line_error(const uint8_t *text, uint64_t b, uint64_t e, int64_t line, std::string &msg)
{
    if (b < e && memchr(text + b, 0, (size_t)(e - b))) return gtf_fail(msg, "[l2r_gtf_order] line %lld: a NUL byte in the text", (long long)line);
    const GtfLine g = gtf_line(text, b, e);
    if (g.why == 1) return gtf_fail(msg, "[l2r_gtf_order] line %lld: a transcript line with fewer than five fields (no start or no end)", (long long)line);
    return gtf_fail(msg, "[l2r_gtf_order] line %lld: the %s of a transcript line is not a decimal number of at most 4294967295", (long long)line, g.why == 2 ? "start" : "end");
}

// [b, e) of the 1-based line `line` (e without the '\n'); false where the text has fewer lines
static bool gtf_find_line(const uint8_t *text, uint64_t n, int64_t line, uint64_t *b, uint64_t *e)
{
    uint64_t p = 0;
    for (int64_t k = 1; p < n || k == 1; ++k) {
        const uint8_t *nl = p < n ? (const uint8_t *)memchr(text + p, '\n', (size_t)(n - p)) : nullptr;
        const uint64_t q = nl ? (uint64_t)(nl - text) : n;
        if (k == line) { *b = p; *e = q; return true; }
        if (!nl) break;
        p = q + 1;
    }
    return false;
}

// the 1-based line that holds the text's first NUL byte, 0 where it has none
static int64_t gtf_first_nul_line(const uint8_t *text, uint64_t n)
{
    const uint8_t *z = n ? (const uint8_t *)memchr(text, 0, (size_t)n) : nullptr;
    if (!z) return 0;
    int64_t line = 1;
    for (const uint8_t *p = text; (p = (const uint8_t *)memchr(p, '\n', (size_t)(z - p))); ++p) ++line;
    return line;
}

struct GtfOrder {
    std::vector<uint64_t> start;                         // the kept lines in the order: offset, length without '\n', 1-based line number
    std::vector<uint32_t> len, line;
    int64_t n_lines = 0, n_tx = 0, n_heads = 0, n_beyond = 0, n_names = 0;
    int64_t descent_line = 0;                            // the first kept line whose triple is below its predecessor's, 0: none (the order is the identity)
};

// The exact routine: split, keep, carry, then a stable sort by the triple (sort = false: the rows stay in line order, for the check).
// 0, or -1 and the error of the smallest bad line.
static int gtf_order_host(const uint8_t *text, uint64_t n, GtfOrder &out, std::string &msg, bool sort = true)
{
    out = GtfOrder();
    struct Key { uint32_t c, s, e; };
    std::vector<Key> key;
    GtfChrRanks ranks;
    Key cur{0, 0, 0};
    uint64_t prev_f1 = 0, prev_len = 0;
    const int64_t nul_line = gtf_first_nul_line(text, n);
    int64_t line = 0;
    for (uint64_t p = 0; p < n;) {
        const uint8_t *nl = (const uint8_t *)memchr(text + p, '\n', (size_t)(n - p));
        const uint64_t q = nl ? (uint64_t)(nl - text) : n;
        ++line;
        if (line == nul_line) return gtf_line_error(text, p, q, line, msg);
        if (line > (int64_t)0xffffffffll || q - p > 0xffffffffull) return gtf_fail(msg, "[l2r_gtf_order] line %lld: beyond 2^32 - 1 lines or bytes of one line", (long long)line);
        const GtfLine g = gtf_line(text, p, q);
        if (g.bad) return gtf_line_error(text, p, q, line, msg);
        if (g.tx) {
            if (out.n_tx == 0 || g.f1_len != prev_len || memcmp(text + g.f1, text + prev_f1, (size_t)prev_len) != 0) ++out.n_heads;
            prev_f1 = g.f1; prev_len = g.f1_len;
            ++out.n_tx;
            cur = Key{ranks.rank(text + g.f1, (size_t)g.f1_len), g.s, g.e};
        }
        if (g.kept) {
            if (!key.empty() && !out.descent_line) {
                const Key &b = key.back();
                if (cur.c != b.c ? cur.c < b.c : cur.s != b.s ? cur.s < b.s : cur.e < b.e) out.descent_line = line;
            }
            key.push_back(cur);
            out.start.push_back(p); out.len.push_back((uint32_t)(q - p)); out.line.push_back((uint32_t)line);
        }
        p = q + 1;
    }
    out.n_lines = line;
    out.n_beyond = ranks.beyond;
    out.n_names = ranks.distinct();
    if (!out.descent_line || !sort) return 0;
    const size_t R = key.size();
    std::vector<size_t> idx(R);
    for (size_t i = 0; i < R; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        const Key &x = key[a], &y = key[b];
        return x.c != y.c ? x.c < y.c : x.s != y.s ? x.s < y.s : x.e < y.e;
    });
    GtfOrder o;
    o.start.resize(R); o.len.resize(R); o.line.resize(R);
    for (size_t k = 0; k < R; ++k) { o.start[k] = out.start[idx[k]]; o.len[k] = out.len[idx[k]]; o.line[k] = out.line[idx[k]]; }
    out.start.swap(o.start); out.len.swap(o.len); out.line.swap(o.line);
    return 0;
}

}  // namespace l2r
