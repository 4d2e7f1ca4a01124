// l2r_bedplan.hip.h -- the host side of l2r_bed_lines (`bam2bed`): the argument checks, the upper bound of a line's bytes and the batch cut
// made from it (l2r_bed_cut), the text of a domain error, and bed_lines_host, the exact routine that writes the same bytes on one core
// (L2R_BED_ROUTE=host, and the comparator of tools/bench_bed.py).  Host arithmetic only: no HIP call, no context, no environment.
// tests/bed_dump.hip runs it as a stand-alone program for tests/test_bed12_cpu.py.
//
// The rule (include/lr2rmats_hip.h).  A record with FLAG & 4 writes nothing.  Every other record writes, in input order, twelve
// tab-separated columns and '\n': reference name, pos, pos + span, QNAME (+ "/1" with FLAG & 0x40, else "/2" with FLAG & 0x80), MAPQ,
// '-' with FLAG & 16 else '+', pos, pos + span, the colour, the block count, the block sizes and the block starts (commas between, none
// behind the last).  The blocks: cur = 0, len = 0, starts = [0]; M = X D add their length to cur and len; N appends len to the sizes,
// adds its length to cur, appends cur to the starts, len = 0; I S H P add nothing; at the end len is appended and span = cur.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

constexpr uint64_t BED_BATCH_BYTES = 0xffffffffull - 63;  // 2^32 - 64: the summed bounds of one device batch stay below it (32-bit line offsets)
constexpr int64_t BED_POS_MAX = 2147483647;               // BAM's own limit of a coordinate
constexpr uint32_t BED_ADVANCE = 0x18du;                  // bit op: M D N = X move along the reference (the kernels of l2r_bed.hip.h too)
constexpr uint32_t BED_OP_N = 3u;

enum { BED_OK = 0, BED_E_TID, BED_E_POS, BED_E_OP, BED_E_END };     // kinds of a record's domain error, in the order they are looked for

static int bed_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// 0, or -1 and the text of l2r_last_error().  ref_off is walked; the names are not read.
static int bed_check_params(const l2r_bed_params *p, std::string &msg, const char *who = "l2r_bed_begin")
{
    if (!p) return bed_fail(msg, "[%s] null argument", who);
    if (p->n_ref < 0) return bed_fail(msg, "[%s] %d reference names", who, p->n_ref);
    if (p->n_ref > 0 && !p->ref_off) return bed_fail(msg, "[%s] null ref_off", who);
    if (p->color_len < 0 || p->color_len > 12) return bed_fail(msg, "[%s] a colour of %d bytes (0..12)", who, p->color_len);
    if (p->n_ref > 0) {
        if (p->ref_off[0] != 0) return bed_fail(msg, "[%s] ref_off does not start at 0", who);
        for (int32_t k = 0; k < p->n_ref; ++k) if (p->ref_off[k + 1] < p->ref_off[k]) return bed_fail(msg, "[%s] ref_off descends at name %d", who, k);
        if (p->ref_off[p->n_ref] > 0 && !p->ref_names) return bed_fail(msg, "[%s] null ref_names", who);
    }
    return 0;
}

// 0, or -1 and the text.  Only the sizes, the pointers themselves and the two offset columns are looked at.  A batch may be a window of
// larger columns: cig_off[0] and name_off[0] need not be 0, cig_off[n] <= n_cigar.
static int bed_check_records(const l2r_bed_records *r, std::string &msg, const char *who = "l2r_bed_lines", bool columns = true)
{
    if (!r) return bed_fail(msg, "[%s] null argument", who);
    if (r->n < 0 || r->n_cigar < 0) return bed_fail(msg, "[%s] negative size", who);
    if (r->n == 0) return 0;
    if (!r->flag || !r->tid || !r->cig_off || !r->name_off) return bed_fail(msg, "[%s] null column", who);
    if (columns && (!r->pos || !r->mapq)) return bed_fail(msg, "[%s] null column", who);
    if (r->cig_off[0] < 0 || r->name_off[0] < 0) return bed_fail(msg, "[%s] negative offset", who);
    for (int64_t i = 0; i < r->n; ++i) {
        if (r->cig_off[i + 1] < r->cig_off[i]) return bed_fail(msg, "[%s] cig_off descends at record %lld", who, (long long)i);
        const int64_t l = r->name_off[i + 1] - r->name_off[i];
        if (l < 0) return bed_fail(msg, "[%s] name_off descends at record %lld", who, (long long)i);
        if (l > L2R_NAME_MAX) return bed_fail(msg, "[%s] record %lld: a name of %lld bytes (at most %d)", who, (long long)i, (long long)l, L2R_NAME_MAX);
    }
    if (r->cig_off[r->n] > r->n_cigar) return bed_fail(msg, "[%s] cig_off reaches beyond the CIGAR array", who);
    if (columns && r->cig_off[r->n] > r->cig_off[0] && !r->cig) return bed_fail(msg, "[%s] null CIGAR array", who);
    if (columns && r->name_off[r->n] > r->name_off[0] && !r->names) return bed_fail(msg, "[%s] null names", who);
    return 0;
}

// An upper bound of the bytes of record i's line, from the name length, the chromosome name length, the colour length and the operation
// count alone: four coordinates, the block count and every block's size and start at ten digits (inside the domain no number is above
// 2147483647), one block more than operations, MAPQ at three, the mate suffix, eleven tabs and the '\n'.  0 for an unmapped record.
static uint64_t bed_line_bound(const l2r_bed_records *r, const l2r_bed_params *p, int64_t i)
{
    if (r->flag[i] & 4u) return 0;
    const int32_t t = r->tid[i];
    const uint64_t chrom = (t >= 0 && t < p->n_ref) ? (uint64_t)(p->ref_off[t + 1] - p->ref_off[t]) : 0;
    const uint64_t ops = (uint64_t)(r->cig_off[i + 1] - r->cig_off[i]);
    return chrom + 4 * 10 + (uint64_t)(r->name_off[i + 1] - r->name_off[i]) + 2 + 3 + 1 + (uint64_t)p->color_len + 10 + 22 * (ops + 1) + 12;
}

// How many records from `first` one batch takes: as many as max_records, with their summed bounds below max_bytes -- but always one.
// -1 where that one record's bound alone reaches 2^32 - 64 (no device batch holds it).
static int bed_cut(const l2r_bed_records *r, const l2r_bed_params *p, int64_t first, int64_t max_records, int64_t max_bytes, int64_t *n_take, std::string &msg)
{
    if (!n_take) return bed_fail(msg, "[l2r_bed_cut] null argument");
    *n_take = 0;
    if (bed_check_params(p, msg, "l2r_bed_cut") || bed_check_records(r, msg, "l2r_bed_cut", false)) return -1;
    if (first < 0 || first > r->n) return bed_fail(msg, "[l2r_bed_cut] first record %lld of %lld", (long long)first, (long long)r->n);
    if (max_records < 1 || max_bytes < 1) return bed_fail(msg, "[l2r_bed_cut] a batch of %lld records and %lld bytes", (long long)max_records, (long long)max_bytes);
    uint64_t sum = 0;
    int64_t k = 0;
    for (; first + k < r->n && k < max_records; ++k) {
        const uint64_t b = bed_line_bound(r, p, first + k);
        if (b >= BED_BATCH_BYTES) {
            if (k == 0) return bed_fail(msg, "[l2r_bed_cut] record %lld: the bound of its line, %llu bytes, is beyond one batch (2^32 - 64)", (long long)first, (unsigned long long)b);
            break;
        }
        if (k > 0 && (sum + b >= (uint64_t)max_bytes || sum + b >= BED_BATCH_BYTES)) break;
        sum += b;
    }
    *n_take = k;
    return 0;
}

// the summed bounds of a whole batch, saturated at 2^32 - 64
static uint64_t bed_batch_bound(const l2r_bed_records *r, const l2r_bed_params *p)
{
    uint64_t sum = 0;
    for (int64_t i = 0; i < r->n && sum < BED_BATCH_BYTES; ++i) sum += bed_line_bound(r, p, i);
    return sum < BED_BATCH_BYTES ? sum : BED_BATCH_BYTES;
}

// The blocks of one record by the rule.  size / start: null, or room for operations + 1 words.  Returns the kind of its domain error.
static int bed_blocks(const l2r_bed_records *r, const l2r_bed_params *p, int64_t i, uint64_t *size, uint64_t *start, uint64_t *n_blocks, uint64_t *span)
{
    const int32_t t = r->tid[i];
    if (t < 0 || t >= p->n_ref) return BED_E_TID;
    if (r->pos[i] < 0) return BED_E_POS;
    uint64_t cur = 0, len = 0, nb = 0;
    if (start) start[0] = 0;
    for (int64_t k = r->cig_off[i]; k < r->cig_off[i + 1]; ++k) {
        const uint32_t w = r->cig[k], op = w & 0xfu, l = w >> 4;
        if (op > 8u) return BED_E_OP;
        if (op == BED_OP_N) {
            if (size) size[nb] = len;
            cur += l; ++nb; len = 0;
            if (start) start[nb] = cur;
        } else if ((BED_ADVANCE >> op) & 1u) { cur += l; len += l; }
    }
    if (size) size[nb] = len;
    *n_blocks = nb + 1; *span = cur;
    return (int64_t)r->pos[i] + (int64_t)cur > BED_POS_MAX ? BED_E_END : BED_OK;
}

// The error of record i (0-based within the call), for both routes; BED_OK: the record has none and msg is left alone.
static int bed_record_error(const l2r_bed_records *r, const l2r_bed_params *p, int64_t i, std::string &msg)
{
    if (r->flag[i] & 4u) return BED_OK;
    uint64_t nb = 0, span = 0;
    const int kind = bed_blocks(r, p, i, nullptr, nullptr, &nb, &span);
    switch (kind) {
    case BED_E_TID: bed_fail(msg, "[l2r_bed_lines] record %lld: a mapped record with reference %d of %d", (long long)i, r->tid[i], p->n_ref); break;
    case BED_E_POS: bed_fail(msg, "[l2r_bed_lines] record %lld: a mapped record at position %d", (long long)i, r->pos[i]); break;
    case BED_E_OP: bed_fail(msg, "[l2r_bed_lines] record %lld: a CIGAR operation code above 8", (long long)i); break;
    case BED_E_END: bed_fail(msg, "[l2r_bed_lines] record %lld: the end %lld is beyond 2147483647", (long long)i, (long long)r->pos[i] + (long long)span); break;
    default: break;
    }
    return kind;
}

static inline void bed_put_num(std::vector<uint8_t> &out, uint64_t v)
{
    char d[24];
    int n = 0;
    do { d[n++] = (char)('0' + v % 10u); v /= 10u; } while (v);
    while (n) out.push_back((uint8_t)d[--n]);
}

// The exact routine on one core: the text of the batch appended to `out` (left as it was on an error), *n_lines = lines written.
// 0, or -1 and the error of the smallest bad record.
static int bed_lines_host(const l2r_bed_records *r, const l2r_bed_params *p, std::vector<uint8_t> &out, int64_t *n_lines, std::string &msg)
{
    const size_t keep = out.size();
    std::vector<uint64_t> size, start;
    int64_t lines = 0;
    for (int64_t i = 0; i < r->n; ++i) {
        if (r->flag[i] & 4u) continue;
        const size_t ops = (size_t)(r->cig_off[i + 1] - r->cig_off[i]);
        if (size.size() < ops + 1) { size.resize(ops + 1); start.resize(ops + 1); }
        uint64_t nb = 0, span = 0;
        if (bed_blocks(r, p, i, size.data(), start.data(), &nb, &span)) { out.resize(keep); (void)bed_record_error(r, p, i, msg); return -1; }
        const int32_t t = r->tid[i];
        const uint64_t b = (uint64_t)r->pos[i], e = b + span;
        const uint32_t f = r->flag[i];
        out.insert(out.end(), p->ref_names + p->ref_off[t], p->ref_names + p->ref_off[t + 1]);
        out.push_back('\t'); bed_put_num(out, b); out.push_back('\t'); bed_put_num(out, e); out.push_back('\t');
        out.insert(out.end(), r->names + r->name_off[i], r->names + r->name_off[i + 1]);
        if (f & 0xc0u) { out.push_back('/'); out.push_back((f & 0x40u) ? '1' : '2'); }
        out.push_back('\t'); bed_put_num(out, r->mapq[i]); out.push_back('\t'); out.push_back((f & 16u) ? '-' : '+');
        out.push_back('\t'); bed_put_num(out, b); out.push_back('\t'); bed_put_num(out, e); out.push_back('\t');
        out.insert(out.end(), p->color, p->color + p->color_len);
        out.push_back('\t'); bed_put_num(out, nb); out.push_back('\t');
        for (uint64_t k = 0; k < nb; ++k) { if (k) out.push_back(','); bed_put_num(out, size[k]); }
        out.push_back('\t');
        for (uint64_t k = 0; k < nb; ++k) { if (k) out.push_back(','); bed_put_num(out, start[k]); }
        out.push_back('\n');
        ++lines;
    }
    if (n_lines) *n_lines = lines;
    return 0;
}

}  // namespace l2r
