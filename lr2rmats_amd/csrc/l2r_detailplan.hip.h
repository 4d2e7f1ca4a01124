// l2r_detailplan.hip.h -- the host side of l2r_detail_* (the per-read detail table of `update-gtf -A`): the argument checks, the kinds of a
// read's domain error in the order they are looked for and their one text, detail_line_bytes (the exact bytes of one line and where its
// segments begin, or its error kind) and detail_text_host, the exact routine that writes the same bytes on one core
// (L2R_DETAIL_ROUTE=host, and the comparator of tools/bench_detail.py).  The checks themselves and the batch cut are those of
// l2r_gtftextplan.hip.h (text_check_*, batch_cut).  Host arithmetic only: no HIP call, no context, no environment.  tests/detail_dump.hip
// runs it as a stand-alone program for tests/test_detail_cpu.py.
//
// The rule is stated in include/lr2rmats_hip.h.  What both sides share beyond it, in functions the host and the kernels both compile: the
// class of a read (detail_cls), the members an exon brings to one of the four index lists (detail_members), the bytes of a list
// (detail_list_len), of the head (detail_head_len) and the split of a line into its seven segments (detail_split).  A line is laid out
// as   head | starts | ends | L1 | L2 | L3 | L4   where every member of a comma list counts its digits and ONE byte behind them -- the
// comma, or for the last member what ends the list: the tab, and for L4 the line's newline.  An empty list is <0>\tNA\t, and an empty
// L4 has the newline behind that.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/lr2rmats_hip.h"
#include "l2r_gtftextplan.hip.h"                        // gtx_digits, gtx_name_len, GTX_BATCH_BYTES, text_check_*, batch_cut

namespace l2r {

static_assert(L2R_DETAIL_NAME_MAX == L2R_GTX_NAME_MAX, "detail: names are looked at by gtx_name_len");
constexpr uint64_t DETAIL_BATCH_BYTES = GTX_BATCH_BYTES;  // 2^32 - 64: a line's bytes, and the summed bytes of one batch, stay below it (32-bit offsets)
constexpr int DETAIL_SEGS = 7;                            // head, starts, ends, L1, L2, L3, L4
constexpr int DETAIL_SPLIT = DETAIL_SEGS - 1;             // words of a line's split: where the segments 1..6 begin in the line

// kinds of a read's domain error, in the order they are looked for
enum { DET_OK = 0, DET_E_TID, DET_E_QNAME_ID, DET_E_QNAME_LONG, DET_E_QNAME_NUL, DET_E_REF, DET_E_GENE_ID, DET_E_GENE_LONG, DET_E_GENE_NUL,
       DET_E_NOEXON, DET_E_NEG, DET_E_BIG, DET_E_N };
static_assert(DET_E_N <= 16, "detail: read << 4 | kind");

static const char *detail_kind_text(int kind)
{
    switch (kind) {
    case DET_E_TID: return "a reference outside the table";
    case DET_E_QNAME_ID: return "a read-name id at or beyond names_len";
    case DET_E_QNAME_LONG: return "a read name of 255 or more bytes";
    case DET_E_QNAME_NUL: return "a read name without a NUL inside the table";
    case DET_E_REF: return "a transcript index at or beyond the annotation's transcripts";
    case DET_E_GENE_ID: return "a gene id or gene name id at or beyond anno_names_len";
    case DET_E_GENE_LONG: return "a gene id or gene name of 255 or more bytes";
    case DET_E_GENE_NUL: return "a gene id or gene name without a NUL inside the table";
    case DET_E_NOEXON: return "a read with no exon";
    case DET_E_NEG: return "a negative exon start or end";
    case DET_E_BIG: return "its line reaches 2^32 - 64 bytes";
    default: return "no error";
    }
}

// the one text of a read's domain error, for both routes
static int detail_row_fail(std::string &msg, int64_t i, int kind) { return gtx_fail(msg, "[l2r_detail_rows] read %lld: %s", (long long)i, detail_kind_text(kind)); }

// 0, or -2 (an argument error, not a domain error) and the text of l2r_last_error().  ref_off is walked.
static int detail_check_params(const l2r_detail_params *p, std::string &msg, const char *who = "l2r_detail_begin")
{
    if (!p) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    if (p->n_ref < 0) { gtx_fail(msg, "[%s] %d reference names", who, p->n_ref); return -2; }
    if (p->n_ref > 0) {
        if (!p->ref_off) { gtx_fail(msg, "[%s] null ref_off", who); return -2; }
        if (text_check_ref_off(p->n_ref, p->ref_off, p->ref_names, msg, who)) return -2;
    }
    return text_check_genes(p->n_tx, p->anno_names_len, p->anno_names, p->tx_gid, p->tx_gname, msg, who);
}

static int detail_check_rows(const l2r_detail_reads *r, std::string &msg, const char *who = "l2r_detail_rows")
{
    if (!r) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    return text_check_reads(r->n, r->names_len, r->names, r->tid, r->qname, r->res, msg, who, "rows");
}

// ---- what the host and the kernels both compile

__host__ __device__ inline uint32_t detail_cls(uint32_t info) { return (info & L2R_INFO_KNOWN) ? 0u : (info & L2R_INFO_KNOWN_SITE) ? 1u : 2u; }

// The members exon j of n, with the flags f, brings to list k (0: L1 .. 3: L4): their count (0..2), and the values v[0 .. count)
__host__ __device__ inline uint32_t detail_member_vals(uint32_t j, uint32_t n, uint32_t f, int k, uint32_t v[2])
{
    v[0] = j; v[1] = 2u * j + 1u;
    if (k == 0) return (f & L2R_EXF_NOVEL_EXON) ? 1u : 0u;
    if (j + 1u >= n) return 0u;                             // (the junction lists stop at n - 1)
    if (k == 1) {
        const bool don = (f & L2R_EXF_NOVEL_DON) != 0, acc = (f & L2R_EXF_NOVEL_ACC) != 0;
        v[0] = don ? 2u * j : 2u * j + 1u;
        return (don ? 1u : 0u) + (acc ? 1u : 0u);
    }
    return (f & (k == 2 ? L2R_EXF_NOVEL_JUNC : L2R_EXF_UNREL_JUNC)) ? 1u : 0u;
}
// ... and their bytes: digits and the one byte behind them
__host__ __device__ inline void detail_members(uint32_t j, uint32_t n, uint32_t f, int k, uint32_t &cnt, uint32_t &bytes)
{
    uint32_t v[2];
    cnt = detail_member_vals(j, n, f, k, v);
    bytes = (cnt > 0u ? gtx_digits(v[0]) + 1u : 0u) + (cnt > 1u ? gtx_digits(v[1]) + 1u : 0u);
}
// the bytes of list k with cnt members of mem bytes: <cnt>\t and the members, or NA\t; an empty L4 has the newline behind it
__host__ __device__ inline uint64_t detail_list_len(int k, uint32_t cnt, uint64_t mem) { return (uint64_t)gtx_digits(cnt) + 1u + (cnt ? mem : (k == 3 ? 4u : 3u)); }
// <qname>\t<chr>\t<+|->\t<cls>\t<gid>\t<gname>\t<n>\t
__host__ __device__ inline uint32_t detail_head_len(uint32_t qname, uint32_t chr, uint32_t gid, uint32_t gname, uint32_t n) { return qname + 1u + chr + 1u + 4u + gid + 1u + gname + 1u + gtx_digits(n) + 1u; }

// what a read's exons add up to: the bytes of the starts and the ends (digits and one byte each), the lists' members and their bytes
struct DetailSums { uint64_t xs, xe; uint32_t cnt[4]; uint64_t mem[4]; };
// where the segments 1..6 begin in the line; returns the line's bytes (from DETAIL_BATCH_BYTES on the split means nothing)
__host__ __device__ inline uint64_t detail_split(uint32_t head, const DetailSums &s, uint32_t split[DETAIL_SPLIT])
{
    uint64_t at = head;
    split[0] = (uint32_t)at; at += s.xs;
    split[1] = (uint32_t)at; at += s.xe;
#pragma unroll
    for (int k = 0; k < 4; ++k) { split[2 + k] = (uint32_t)at; at += detail_list_len(k, s.cnt[k], s.mem[k]); }
    return at;
}

// ---- the host alone

// Read i: its names, or the kind of its domain error (the kinds up to DET_E_NOEXON)
struct DetailRow { const uint8_t *qname, *chr, *gid, *gname; uint32_t len[4]; int64_t off; uint32_t n, info; };
static const uint8_t DETAIL_NA[3] = {'N', 'A', 0};

static int detail_row(const l2r_detail_params *p, const l2r_detail_reads *r, int64_t i, DetailRow &k)
{
    const l2r_result *s = r->res;
    const int32_t tid = r->tid[i];
    if (tid < 0 || tid >= p->n_ref) return DET_E_TID;
    k.chr = p->ref_names + p->ref_off[tid]; k.len[1] = (uint32_t)(p->ref_off[tid + 1] - p->ref_off[tid]);
    int e = gtx_name_len(r->names, r->names_len, r->qname[i], &k.len[0]);
    if (e) return e == GTX_E_NAME_ID ? DET_E_QNAME_ID : e == GTX_E_NAME_LONG ? DET_E_QNAME_LONG : DET_E_QNAME_NUL;
    k.qname = r->names + r->qname[i];
    const int32_t ref = s->ref_tx[i];
    if (ref >= 0 && (int64_t)ref >= p->n_tx) return DET_E_REF;
    if (ref < 0) { k.gid = k.gname = DETAIL_NA; k.len[2] = k.len[3] = 2u; }
    else {
        const uint32_t id[2] = {p->tx_gid[ref], p->tx_gname[ref]};
        for (int c = 0; c < 2; ++c) {
            e = gtx_name_len(p->anno_names, p->anno_names_len, id[c], &k.len[2 + c]);
            if (e) return e == GTX_E_NAME_ID ? DET_E_GENE_ID : e == GTX_E_NAME_LONG ? DET_E_GENE_LONG : DET_E_GENE_NUL;
        }
        k.gid = p->anno_names + id[0]; k.gname = p->anno_names + id[1];
    }
    k.info = s->info[i]; k.n = L2R_INFO_NEXON(k.info); k.off = s->ex_off[i];
    if (k.n < 1u) return DET_E_NOEXON;
    return DET_OK;
}

// The exact bytes of read i's line and its split, or the kind of its domain error (then *bytes is 0).  res != NULL.
static int detail_line_bytes(const l2r_detail_params *p, const l2r_detail_reads *r, int64_t i, uint64_t *bytes, uint32_t split[DETAIL_SPLIT])
{
    *bytes = 0;
    for (int k = 0; k < DETAIL_SPLIT; ++k) split[k] = 0u;
    DetailRow k;
    const int e = detail_row(p, r, i, k);
    if (e) return e;
    const l2r_result *s = r->res;
    DetailSums sum = {0, 0, {0u, 0u, 0u, 0u}, {0, 0, 0, 0}};
    for (uint32_t j = 0; j < k.n; ++j) {
        const int32_t a = s->ex_start[k.off + j], b = s->ex_end[k.off + j];
        if (a < 0 || b < 0) return DET_E_NEG;
        sum.xs += gtx_digits((uint32_t)a) + 1u; sum.xe += gtx_digits((uint32_t)b) + 1u;
        for (int l = 0; l < 4; ++l) {
            uint32_t c, m;
            detail_members(j, k.n, s->ex_flag[k.off + j], l, c, m);
            sum.cnt[l] += c; sum.mem[l] += m;
        }
    }
    const uint64_t total = detail_split(detail_head_len(k.len[0], k.len[1], k.len[2], k.len[3], k.n), sum, split);
    if (total >= DETAIL_BATCH_BYTES) return DET_E_BIG;
    *bytes = total;
    return DET_OK;
}

// the batch cut over the measured lengths of the rows of l2r_detail_lines
static int detail_cut(const uint32_t *len, int64_t n, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_take, int64_t *n_bytes, std::string &msg)
{ return batch_cut(len, n, first, max_rows, max_bytes, n_take, n_bytes, msg, "l2r_detail_lines", "row"); }

// list k of a read: <cnt>\t, the members comma separated or NA, and what stands behind (a tab; behind L4 only where it is empty)
static void detail_put_list(std::vector<uint8_t> &out, const uint8_t *f, uint32_t n, int k)
{
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < n; ++j) { uint32_t c, m; detail_members(j, n, f[j], k, c, m); cnt += c; }
    gtx_put_num(out, cnt); out.push_back('\t');
    if (!cnt) { gtx_put_str(out, "NA\t"); return; }
    bool first = true;
    const uint32_t stop = k == 0 ? n : n - 1u;
    for (uint32_t j = 0; j < stop; ++j) {
        if (k == 1) {
            if (f[j] & L2R_EXF_NOVEL_DON) { if (!first) out.push_back(','); first = false; gtx_put_num(out, 2u * j); }
            if (f[j] & L2R_EXF_NOVEL_ACC) { if (!first) out.push_back(','); first = false; gtx_put_num(out, 2u * j + 1u); }
        } else if (f[j] & (k == 0 ? L2R_EXF_NOVEL_EXON : k == 2 ? L2R_EXF_NOVEL_JUNC : L2R_EXF_UNREL_JUNC)) {
            if (!first) out.push_back(',');
            first = false; gtx_put_num(out, j);
        }
    }
    if (k != 3) out.push_back('\t');
}

// The exact routine on one core: the lines of the rows [first, first + count) appended to `out` (left as it was on an error).
// 0, or -1 and the error of the smallest bad row.  res != NULL.
static int detail_text_host(const l2r_detail_params *p, const l2r_detail_reads *r, int64_t first, int64_t count, std::vector<uint8_t> &out, std::string &msg)
{
    const size_t keep = out.size();
    const l2r_result *s = r->res;
    for (int64_t i = first; i < first + count; ++i) {
        uint64_t bytes = 0; uint32_t split[DETAIL_SPLIT];
        const int e = detail_line_bytes(p, r, i, &bytes, split);
        if (e) { out.resize(keep); return detail_row_fail(msg, i, e); }
        DetailRow k;
        (void)detail_row(p, r, i, k);
        out.insert(out.end(), k.qname, k.qname + k.len[0]); out.push_back('\t');
        out.insert(out.end(), k.chr, k.chr + k.len[1]); out.push_back('\t');
        out.push_back((k.info & L2R_INFO_REV) ? '-' : '+'); out.push_back('\t');
        out.push_back((uint8_t)('0' + detail_cls(k.info))); out.push_back('\t');
        out.insert(out.end(), k.gid, k.gid + k.len[2]); out.push_back('\t');
        out.insert(out.end(), k.gname, k.gname + k.len[3]); out.push_back('\t');
        gtx_put_num(out, k.n); out.push_back('\t');
        for (uint32_t j = 0; j < k.n; ++j) { if (j) out.push_back(','); gtx_put_num(out, (uint32_t)s->ex_start[k.off + j]); }
        out.push_back('\t');
        for (uint32_t j = 0; j < k.n; ++j) { if (j) out.push_back(','); gtx_put_num(out, (uint32_t)s->ex_end[k.off + j]); }
        out.push_back('\t');
        for (int l = 0; l < 4; ++l) detail_put_list(out, s->ex_flag + k.off, k.n, l);
        out.push_back('\n');
    }
    return 0;
}

}  // namespace l2r
