// lists_dump.hip -- the host side of the read lists of `update-gtf -a / -k / -v / -u` (lr2rmats_amd/csrc/l2r_readlistplan.hip.h) as a
// stand-alone host program, for tests/test_read_lists_cpu.py:
//     lists_dump <case file> <output file> [<case file> <output file> ...]
//     lists_dump faults        (one line per argument fault of l2r_gtftext_anno and l2r_gtftext_reads: tests/text_faults.hip.h)
// runs the argument checks and then, for each of the four lists, rl_select, rl_block_bytes of every block, gtx_cut from the case's first
// block to the last, and rl_text_host, the exact routine behind L2R_GTX_ROUTE=host, over the whole list and batch by batch.  No HIP
// function is called and no GPU is needed; `make -C lr2rmats_amd/csrc lists-dump` builds it with ASan + UBSan on the host code.
//
// Case file: sixteen int64 -- reads, exons, bytes of the reads' names table, 1 where a tid_name column follows, reference names, bytes of
// the source string, annotation transcripts, bytes of the annotation's names table, has_sj, split, first block of the cuts, max_blocks,
// max_bytes, sums_only, and two zeros -- then tid (int32), qname (uint32), tid_name (uint32, where announced), the names table, ex_off
// (int64, n + 1), info (uint32), ref_tx (int32), xs and xe (int32), the exon flags (uint8), ref_off (int64, n_ref + 1), the reference
// name bytes, the source string, the annotation's names table, tx_gid and tx_gname (uint32, n_tx each).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` of the checks and
// `error`, or per list L = 0..3 `read_L`, `first_L`, `count_L`, `piece_L`, `pieces_L`, and per block `kind_L`, `bytes_L`, `lines_L`; then,
// where no block has an error, `text_L` with `n_lines_L`, `cut_L` (the blocks each batch took) and `text_cut_L` (the batches' texts
// concatenated); else `text_rc_L` and `error_L` of rl_text_host.  The seconds rl_select and rl_text_host took go to stderr (tools/bench_lists.py
// reads them from the build without sanitizers, `make -C lr2rmats_amd/csrc lists-host`).  sums_only != 0 (a text of gigabytes): the text is
// made batch by batch as gtx_cut cuts it and only `n_bytes_L`, `n_lines_L` and `sums_L` leave -- the sum of its bytes and the sum of
// byte * (1 + position mod 251).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_readlistplan.hip.h"
#include "text_faults.hip.h"

using namespace l2r;

static FILE *g_out = nullptr;

static void put(const char *name, int list, const char *type, const void *data, size_t size, int64_t count)
{
    char head[32];
    memset(head, 0, sizeof head);
    if (list < 0) snprintf(head, 24, "%s", name); else snprintf(head, 24, "%s_%d", name, list);
    snprintf(head + 24, 8, "%s", type);
    fwrite(head, 1, sizeof head, g_out);
    fwrite(&count, 8, 1, g_out);
    if (count) fwrite(data, size, (size_t)count, g_out);
}
static void put_i64(const char *name, int list, int64_t v) { put(name, list, "<i8", &v, 8, 1); }

// exactly `count` elements: a read beyond them is the sanitizer's to report
template <typename T> static bool get(FILE *f, std::vector<T> &v, int64_t count)
{
    if (count < 0) count = 0;
    v.assign((size_t)count, T());
    v.shrink_to_fit();
    return count == 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}

static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

static int run(const char *in_fn, const char *out_fn)
{
    FILE *f = fopen(in_fn, "rb");
    if (!f) { perror(in_fn); return 2; }
    int64_t h[16];
    if (fread(h, 8, 16, f) != 16) { fprintf(stderr, "lists_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], n_ex = h[1], names_len = h[2], has_tn = h[3], n_ref = h[4], src_len = h[5], n_tx = h[6], anno_len = h[7], first = h[10], max_blocks = h[11], max_bytes = h[12];
    std::vector<int32_t> tid, ref_tx, xs, xe; std::vector<uint32_t> qname, tid_name, info, tx_gid, tx_gname; std::vector<uint8_t> names, fl, ref_names, src, anno;
    std::vector<int64_t> ex_off, ref_off;
    bool ok = get(f, tid, n) && get(f, qname, n) && get(f, tid_name, has_tn ? n : 0) && get(f, names, names_len) && get(f, ex_off, n + 1) && get(f, info, n) && get(f, ref_tx, n) &&
              get(f, xs, n_ex) && get(f, xe, n_ex) && get(f, fl, n_ex) && get(f, ref_off, n_ref + 1);
    ok = ok && get(f, ref_names, n_ref > 0 ? ref_off[(size_t)n_ref] : 0) && get(f, src, src_len) && get(f, anno, anno_len) && get(f, tx_gid, n_tx) && get(f, tx_gname, n_tx);
    fclose(f);
    if (!ok) { fprintf(stderr, "lists_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_gtx_params p = {(int32_t)n_ref, ref_off.data(), ref_names.empty() ? nullptr : ref_names.data(), L2R_GTX_READ, (int32_t)src_len, src.empty() ? nullptr : src.data()};
    const l2r_gtx_anno a = {n_tx, anno_len, anno.empty() ? nullptr : anno.data(), tx_gid.data(), tx_gname.data()};
    l2r_result res = {n, n_ex, n_ex, ex_off.data(), xs.data(), xe.data(), fl.data(), info.data(), ref_tx.data()};
    const l2r_gtx_reads rd = {n, tid.data(), names_len, names.empty() ? nullptr : names.data(), qname.data(), has_tn ? tid_name.data() : nullptr, &res, (int32_t)h[8], (int32_t)h[9]};
    std::string msg;
    int rc = gtx_check_params(&p, msg);
    if (!rc) rc = rl_check_anno(&a, msg);
    if (!rc) rc = rl_check_reads(&rd, msg);
    if (!rc && rl_check_list(4, msg) != -2) { fprintf(stderr, "lists_dump: list 4 passed the check\n"); return 2; }
    if (!rc) msg.clear();
    put_i64("rc", -1, rc);
    if (rc) {
        put("error", -1, "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    const RlReads r = {n, tid.data(), names_len, names.data(), qname.data(), has_tn ? tid_name.data() : qname.data(), ex_off.data(), info.data(), ref_tx.data(),
                       xs.data(), xe.data(), fl.data(), h[8] != 0, h[9] != 0};
    for (int list = 0; list < 4; ++list) {
        RlSel s;
        auto t0 = std::chrono::steady_clock::now();
        rl_select(r, list, s);
        const double t_sel = since(t0);
        const int64_t m = s.m();
        put("read", list, "<i4", s.read.data(), 4, m); put("first", list, "<i4", s.first.data(), 4, m); put("count", list, "<i4", s.count.data(), 4, m);
        put("piece", list, "<i4", s.piece.data(), 4, m); put_i64("pieces", list, s.n_pieces);
        std::vector<int64_t> kind((size_t)m);
        std::vector<uint64_t> bytes((size_t)m), lines((size_t)m);
        std::vector<uint32_t> len((size_t)m);
        bool any_bad = false;
        for (int64_t q = 0; q < m; ++q) {
            kind[(size_t)q] = rl_block_bytes(&p, &a, r, s, q, &bytes[(size_t)q], &lines[(size_t)q]);
            len[(size_t)q] = (uint32_t)bytes[(size_t)q];
            any_bad |= kind[(size_t)q] != RL_OK;
        }
        put("kind", list, "<i8", kind.data(), 8, m); put("bytes", list, "<u8", bytes.data(), 8, m); put("lines", list, "<u8", lines.data(), 8, m);
        std::vector<uint8_t> text;
        int64_t n_lines = 0;
        if (h[13] != 0 && !any_bad) {
            uint64_t sums[2] = {0, 0}, at_byte = 0;
            double secs = 0;
            for (int64_t at = 0; at < m;) {
                int64_t take = 0, sum = 0, lines_here = 0;
                if (gtx_cut(len.data(), m, at, max_blocks, max_bytes, &take, &sum, msg) || take < 1) { fprintf(stderr, "lists_dump: %s\n", msg.c_str()); return 2; }
                text.clear();
                t0 = std::chrono::steady_clock::now();
                if (rl_text_host(&p, &a, r, s, at, take, text, &lines_here, msg)) { fprintf(stderr, "lists_dump: %s\n", msg.c_str()); return 2; }
                secs += since(t0);
                for (size_t k = 0; k < text.size(); ++k, ++at_byte) { sums[0] += text[k]; sums[1] += (uint64_t)text[k] * (1u + at_byte % 251u); }
                n_lines += lines_here; at += take;
            }
            fprintf(stderr, "rl_text_host: list %d, %lld blocks, %lld lines, %lld bytes, select %.6f s, text %.6f s\n", list, (long long)m, (long long)n_lines, (long long)at_byte, t_sel, secs);
            put_i64("n_bytes", list, (int64_t)at_byte); put_i64("n_lines", list, n_lines); put("sums", list, "<u8", sums, 8, 2);
            continue;
        }
        t0 = std::chrono::steady_clock::now();
        rc = rl_text_host(&p, &a, r, s, 0, m, text, &n_lines, msg);
        fprintf(stderr, "rl_text_host: list %d, %lld blocks, %lld lines, %lld bytes, select %.6f s, text %.6f s\n", list, (long long)m, (long long)n_lines, (long long)text.size(), t_sel, since(t0));
        put_i64("text_rc", list, rc);
        if (rc) { put("error", list, "|u1", msg.data(), 1, (int64_t)msg.size()); continue; }
        if (any_bad) { fprintf(stderr, "lists_dump: rl_text_host wrote a text over a block with an error\n"); return 2; }
        put("text", list, "|u1", text.data(), 1, (int64_t)text.size()); put_i64("n_lines", list, n_lines);
        std::vector<int64_t> cut;
        std::vector<uint8_t> text_cut;
        for (int64_t at = first; at < m;) {
            int64_t take = 0, sum = 0;
            std::string cmsg;
            if (gtx_cut(len.data(), m, at, max_blocks, max_bytes, &take, &sum, cmsg) || take < 1) { fprintf(stderr, "lists_dump: gtx_cut at %lld: %s\n", (long long)at, cmsg.c_str()); return 2; }
            if (rl_text_host(&p, &a, r, s, at, take, text_cut, nullptr, cmsg)) { fprintf(stderr, "lists_dump: a batch failed behind a sound list: %s\n", cmsg.c_str()); return 2; }
            cut.push_back(take); at += take;
        }
        put("cut", list, "<i8", cut.data(), 8, (int64_t)cut.size());
        put("text_cut", list, "|u1", text_cut.data(), 1, (int64_t)text_cut.size());
    }
    return fclose(g_out) ? 2 : 0;
}

// `lists_dump faults`: the argument faults of l2r_gtftext_anno and l2r_gtftext_reads (text_faults.hip.h)
static int faults()
{
    static const uint8_t bytes[4] = {'g', '1', 'g', '2'};
    static const uint32_t ids[2] = {0, 2};
    const l2r_gtx_anno sound = {2, 4, bytes, ids, ids};
    { std::string msg; const int rc = rl_check_anno(nullptr, msg); text_faults::say("anno_null", rc, msg); }
    text_faults::genes(sound, [](const l2r_gtx_anno *a, std::string &msg) { return rl_check_anno(a, msg); });
    text_faults::reads<l2r_gtx_reads>([](const l2r_gtx_reads *r, std::string &msg) { return rl_check_reads(r, msg); });
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "faults") == 0) return faults();
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: lists_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
