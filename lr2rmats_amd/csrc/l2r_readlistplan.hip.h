// l2r_readlistplan.hip.h -- the host side of the read lists of `update-gtf -a / -k / -v / -u` (l2r_gtftext_anno / _reads / _list): the
// argument checks (over text_check_genes and text_check_reads of l2r_gtftextplan.hip.h, whose batch_cut also cuts the batches), what the
// host and the kernels of l2r_readlist.hip.h both compile (the list a read belongs to, the piece walk, the length pieces of a block),
// rl_select (the selection of one list), rl_block_bytes (the exact bytes and lines of one block, and its domain error) and rl_text_host, the exact routine that writes the same bytes on one core (L2R_GTX_ROUTE=host, and the comparator of
// tools/bench_lists.py).  Host arithmetic only: no HIP call, no context, no environment.  tests/lists_dump.hip runs it as a stand-alone
// program for tests/test_read_lists_cpu.py.
//
// The rule is stated in include/lr2rmats_hip.h.  What both sides share beyond it: the order in which a block's domain errors are looked
// for (RL_E_*: the first that applies is the block's kind), and that a block has TWO line lengths without the numbers -- `fix` of its exon
// lines and `hfix` of its transcript line, which for a piece stands on reference 0.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "l2r_gtftextplan.hip.h"

namespace l2r {

// kinds of a block's domain error, in the order they are looked for
enum { RL_OK = 0, RL_E_TID, RL_E_NOEXON, RL_E_REF, RL_E_NAME_ID, RL_E_NAME_LONG, RL_E_NAME_NUL, RL_E_PIECE_NAME, RL_E_NEG, RL_E_BIG, RL_E_N };
static_assert(RL_E_N <= 16, "a kind travels in four bits");

static const char *rl_kind_text(int kind)
{
    switch (kind) {
    case RL_E_TID: return "a reference outside the table";
    case RL_E_NOEXON: return "a read with no exon";
    case RL_E_REF: return "an annotation transcript at or beyond n_tx";
    case RL_E_NAME_ID: return "a name id at or beyond its table";
    case RL_E_NAME_LONG: return "a name of 255 or more bytes";
    case RL_E_NAME_NUL: return "a name without a NUL inside the table";
    case RL_E_PIECE_NAME: return "a piece name of 100 or more bytes";
    case RL_E_NEG: return "a negative exon coordinate";
    case RL_E_BIG: return "its text reaches 2^32 - 64 bytes";
    default: return "no error";
    }
}
// the one text of a block's domain error, for both routes
static int rl_block_fail(std::string &msg, int64_t q, int kind) { return gtx_fail(msg, "[l2r_gtftext_list] block %lld: %s", (long long)q, rl_kind_text(kind)); }

static int rl_check_anno(const l2r_gtx_anno *a, std::string &msg, const char *who = "l2r_gtftext_anno")
{
    if (!a) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    return text_check_genes(a->n_tx, a->anno_names_len, a->anno_names, a->tx_gid, a->tx_gname, msg, who);
}

static int rl_check_reads(const l2r_gtx_reads *r, std::string &msg, const char *who = "l2r_gtftext_reads")
{
    if (!r) { gtx_fail(msg, "[%s] null argument", who); return -2; }
    return text_check_reads(r->n, r->names_len, r->names, r->tid, r->qname, r->res, msg, who, "reads");
}

static int rl_check_list(int list, std::string &msg, const char *who = "l2r_gtftext_list")
{
    if (list < L2R_GTX_LIST_ALL || list > L2R_GTX_LIST_UNRECOG) { gtx_fail(msg, "[%s] list %d (0 all, 1 known, 2 novel, 3 unrecognised)", who, list); return -2; }
    return 0;
}

// ---- what the host and the kernels both compile

// What read `info` brings to `list`: nothing, itself, or its pieces (then its flags are walked)
enum { RL_NONE = 0, RL_WHOLE, RL_PIECES };
__host__ __device__ inline int rl_mode(int list, uint32_t info, bool has_sj, bool split)
{
    if (list == L2R_GTX_LIST_ALL) return RL_WHOLE;
    if (!(info & L2R_INFO_FULL)) return RL_NONE;
    if (info & L2R_INFO_KNOWN) return list == L2R_GTX_LIST_KNOWN ? RL_WHOLE : RL_NONE;
    if (!(info & L2R_INFO_KNOWN_SITE)) return list == L2R_GTX_LIST_UNRECOG ? RL_WHOLE : RL_NONE;
    if (list != L2R_GTX_LIST_NOVEL) return RL_NONE;
    if (!has_sj || (info & L2R_INFO_SJ_PASS)) return RL_WHOLE;
    return split ? RL_PIECES : RL_NONE;
}

// The piece walk over the flags f[0, n): emit(k, first, last) for piece k; the pieces' count
template <typename Emit>
__host__ __device__ inline uint32_t rl_pieces(const uint8_t *f, int64_t n, Emit emit)
{
    int64_t first = 0;
    bool seen_novel = false, seen_known = false;
    uint32_t k = 0;
    for (int64_t j = 0; j < n; ++j) {
        const bool at_end = j == n - 1;
        const uint32_t fj = f[j];
        if (!at_end) { if (fj & L2R_EXF_NOVEL_JUNC) seen_novel = true; else seen_known = true; }
        if (at_end || (fj & L2R_EXF_UNREL_JUNC)) {
            if (seen_novel && seen_known && j - first >= 1) { emit(k, first, j); ++k; }
            first = j + 1; seen_novel = seen_known = false;
        }
    }
    return k;
}

// the bytes `.split.<k>` adds to a name
__host__ __device__ inline uint32_t rl_suffix_len(int32_t piece) { return piece < 0 ? 0u : 7u + gtx_digits((uint32_t)piece); }

// `NA`, the name of a gene no annotation transcript gives
__host__ __device__ inline uint32_t rl_na_len() { return 2u; }

// ---- the host routine

struct RlReads {                                            // the reads and their results, on the host
    int64_t n; const int32_t *tid; int64_t names_len; const uint8_t *names; const uint32_t *qname, *tid_name /* never null here */;
    const int64_t *ex_off; const uint32_t *info; const int32_t *ref_tx, *xs, *xe; const uint8_t *f;
    bool has_sj, split;
};
struct RlSel { std::vector<int32_t> read, first, count, piece; int64_t n_pieces = 0; int64_t m() const { return (int64_t)read.size(); } };

// the selection of one list, in read order
static void rl_select(const RlReads &r, int list, RlSel &s)
{
    s.read.clear(); s.first.clear(); s.count.clear(); s.piece.clear(); s.n_pieces = 0;
    auto push = [&](int64_t i, int64_t first, int64_t count, int32_t piece) {
        s.read.push_back((int32_t)i); s.first.push_back((int32_t)first); s.count.push_back((int32_t)count); s.piece.push_back(piece);
    };
    for (int64_t i = 0; i < r.n; ++i) {
        const uint32_t info = r.info[i];
        const int64_t n = (int64_t)L2R_INFO_NEXON(info);
        const int mode = rl_mode(list, info, r.has_sj, r.split);
        if (mode == RL_WHOLE) push(i, 0, n, -1);
        else if (mode == RL_PIECES) s.n_pieces += rl_pieces(r.f + r.ex_off[i], n, [&](uint32_t k, int64_t first, int64_t last) { push(i, first, last - first + 1, (int32_t)k); });
    }
}

// Block q of a selection: its names and their lengths, or the kind of its domain error
struct RlBlock { int64_t i, off, n; int32_t piece; bool rev; const uint8_t *name[4]; uint32_t len[4], sfx, attr_len, fix, hfix; };

static int rl_block(const l2r_gtx_params *p, const l2r_gtx_anno *a, const RlReads &r, const RlSel &s, int64_t q, RlBlock &k)
{
    static const uint8_t na[3] = {'N', 'A', 0};
    k.i = s.read[(size_t)q]; k.piece = s.piece[(size_t)q]; k.n = s.count[(size_t)q];
    k.off = r.ex_off[k.i] + s.first[(size_t)q];
    k.rev = (r.info[k.i] & L2R_INFO_REV) != 0;
    const int32_t tid = r.tid[k.i];
    if (tid < 0 || tid >= p->n_ref) return RL_E_TID;
    if (k.n < 1) return RL_E_NOEXON;
    const int32_t ref = r.ref_tx[k.i];
    if (ref >= 0 && (int64_t)ref >= a->n_tx) return RL_E_REF;
    for (int c = 0; c < 4; ++c) {
        const bool gene = c == 0 || c == 2;
        if (gene && ref < 0) { k.name[c] = na; k.len[c] = rl_na_len(); continue; }
        const uint8_t *table = gene ? a->anno_names : r.names;
        const int64_t table_len = gene ? a->anno_names_len : r.names_len;
        const uint32_t id = c == 0 ? a->tx_gid[ref] : c == 2 ? a->tx_gname[ref] : c == 1 ? r.tid_name[k.i] : r.qname[k.i];
        const int e = gtx_name_len(table, table_len, id, &k.len[c]);
        if (e) return e == GTX_E_NAME_ID ? RL_E_NAME_ID : e == GTX_E_NAME_LONG ? RL_E_NAME_LONG : RL_E_NAME_NUL;
        k.name[c] = table + id;
    }
    k.sfx = rl_suffix_len(k.piece);
    if (k.piece >= 0 && (k.len[1] + k.sfx >= L2R_GTX_PIECE_NAME_MAX || k.len[3] + k.sfx >= L2R_GTX_PIECE_NAME_MAX)) return RL_E_PIECE_NAME;
    const uint32_t len[4] = {k.len[0], k.len[1] + k.sfx, k.len[2], k.len[3] + k.sfx};
    k.attr_len = gtx_attr_len(L2R_GTX_READ, len);
    const uint32_t ref_len = (uint32_t)(p->ref_off[tid + 1] - p->ref_off[tid]), head_ref_len = k.piece < 0 ? ref_len : (uint32_t)(p->ref_off[1] - p->ref_off[0]);
    k.fix = gtx_line_fix(ref_len, (uint32_t)p->src_len, k.attr_len);
    k.hfix = gtx_line_fix(head_ref_len, (uint32_t)p->src_len, k.attr_len) + gtx_head_extra(L2R_GTX_READ, 1u);
    return RL_OK;
}

// The exact bytes and lines of block q, or the kind of its domain error (then *bytes and *lines are 0).
static int rl_block_bytes(const l2r_gtx_params *p, const l2r_gtx_anno *a, const RlReads &r, const RlSel &s, int64_t q, uint64_t *bytes, uint64_t *lines)
{
    *bytes = 0; *lines = 0;
    RlBlock k;
    const int e = rl_block(p, a, r, s, q, k);
    if (e) return e;
    uint64_t sum = (uint64_t)k.hfix + (k.piece < 0 ? 0u : 2u);
    for (int64_t j = 0; j < k.n; ++j) {
        const int32_t xs = r.xs[k.off + j], xe = r.xe[k.off + j];
        if (xs < 0 || xe < 0) return RL_E_NEG;
        sum += (uint64_t)k.fix + gtx_digits((uint32_t)xs) + gtx_digits((uint32_t)xe);
    }
    if (k.piece < 0) sum += gtx_digits((uint32_t)r.xs[k.off]) + gtx_digits((uint32_t)r.xe[k.off + k.n - 1]);
    if (sum >= GTX_BATCH_BYTES) return RL_E_BIG;
    *bytes = sum; *lines = (uint64_t)k.n + 1u;
    return RL_OK;
}

// The exact routine on one core: the text of the blocks [first, first + count) of the selection appended to `out` (left as it was on an
// error), *n_lines = lines written.  0, or -1 and the error of the smallest bad block.
static int rl_text_host(const l2r_gtx_params *p, const l2r_gtx_anno *a, const RlReads &r, const RlSel &s, int64_t first, int64_t count,
                        std::vector<uint8_t> &out, int64_t *n_lines, std::string &msg)
{
    const size_t keep = out.size();
    std::vector<uint8_t> front, tail;                       // <ref>\t<src>\t of the exon lines, and <A>
    int64_t lines = 0;
    for (int64_t q = first; q < first + count; ++q) {
        RlBlock k;
        uint64_t bytes = 0, nl = 0;
        const int e = rl_block_bytes(p, a, r, s, q, &bytes, &nl);
        if (e) { out.resize(keep); return rl_block_fail(msg, q, e); }
        (void)rl_block(p, a, r, s, q, k);
        const int32_t tid = r.tid[k.i], head_tid = k.piece < 0 ? tid : 0;
        front.clear(); tail.clear();
        front.insert(front.end(), p->ref_names + p->ref_off[tid], p->ref_names + p->ref_off[tid + 1]);
        front.push_back('\t');
        front.insert(front.end(), p->src, p->src + p->src_len);
        front.push_back('\t');
        bool any = false;
        for (int c = 0; c < 4; ++c) {
            const bool sfx = k.piece >= 0 && (c == 1 || c == 3);
            if (!k.len[c] && !sfx) continue;
            if (any) tail.push_back(' ');
            any = true;
            gtx_put_str(tail, GTX_KEY[c]); gtx_put_str(tail, " \"");
            tail.insert(tail.end(), k.name[c], k.name[c] + k.len[c]);
            if (sfx) { gtx_put_str(tail, ".split."); gtx_put_num(tail, (uint32_t)k.piece); }
            gtx_put_str(tail, "\";");
        }
        // the transcript line: of a piece on reference 0, 0 .. 0, `+`
        out.insert(out.end(), p->ref_names + p->ref_off[head_tid], p->ref_names + p->ref_off[head_tid + 1]);
        out.push_back('\t');
        out.insert(out.end(), p->src, p->src + p->src_len);
        gtx_put_str(out, "\ttranscript\t");
        gtx_put_num(out, k.piece < 0 ? (uint32_t)r.xs[k.off] : 0u); out.push_back('\t'); gtx_put_num(out, k.piece < 0 ? (uint32_t)r.xe[k.off + k.n - 1] : 0u);
        gtx_put_str(out, "\t.\t"); out.push_back(k.piece < 0 && k.rev ? '-' : '+'); gtx_put_str(out, "\t.\t");
        out.insert(out.end(), tail.begin(), tail.end());
        gtx_put_str(out, " transcript_cov \"1\";\n");
        for (int64_t x = 0; x < k.n; ++x) {
            const int64_t j = (k.piece < 0 && k.rev) ? k.n - 1 - x : x;
            out.insert(out.end(), front.begin(), front.end());
            gtx_put_str(out, "exon\t"); gtx_put_num(out, (uint32_t)r.xs[k.off + j]); out.push_back('\t'); gtx_put_num(out, (uint32_t)r.xe[k.off + j]);
            gtx_put_str(out, "\t.\t"); out.push_back(k.rev ? '-' : '+'); gtx_put_str(out, "\t.\t");
            out.insert(out.end(), tail.begin(), tail.end());
            out.push_back('\n');
        }
        lines += k.n + 1;
    }
    if (n_lines) *n_lines = lines;
    return 0;
}

}  // namespace l2r
