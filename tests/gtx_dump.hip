// gtx_dump.hip -- the host side of l2r_gtftext_* (lr2rmats_amd/csrc/l2r_gtftextplan.hip.h) as a stand-alone host program, for
// tests/test_gtf_text_cpu.py:
//     gtx_dump <case file> <output file> [<case file> <output file> ...]
//     gtx_dump faults        (one line per argument fault of l2r_gtftext_begin's reference table and l2r_gtftext_lines: tests/text_faults.hip.h)
// runs the argument checks, gtx_block_bytes of every block, gtx_cut from the case's first block to the last, and gtx_text_host, the exact
// routine behind L2R_GTX_ROUTE=host, over the whole selection and batch by batch.  No HIP function is called and no GPU is needed;
// `make -C lr2rmats_amd/csrc gtx-dump` builds it with ASan + UBSan on the host code.
//
// Case file: twelve int64 -- transcripts, exons, bytes of the names table, reference names, form, bytes of the source string, blocks,
// columns (bit 0 sel, 1 start, 2 end, 3 cov), first block of the cuts, max_blocks, max_bytes, sums_only -- then tid (int32), rev (uint8), ex_off
// (int64, n + 1), xs and xe (int32), the names table, gid, tids, gname and tname (uint32, n each), ref_off (int64, n_ref + 1), the
// reference name bytes, the source string, and the selection's columns that the bits name (int32, m each).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` of the checks and
// `error`, or per block `kind`, `bytes` and `lines`; then, where no block has an error, `cut` (the blocks each batch took), `cut_bytes`,
// `text` with `n_lines`, and `text_cut` (the batches' texts concatenated); else `text_rc` and `error` of gtx_text_host.  The seconds
// gtx_text_host took go to stderr (tools/bench_gtx.py reads them from the build without sanitizers, `make -C lr2rmats_amd/csrc gtx-host`).
// sums_only != 0 (a text of gigabytes): the text is made batch by batch as gtx_cut cuts it and only `n_bytes`, `n_lines` and `sums` leave --
// the sum of its bytes and the sum of byte * (1 + position mod 251).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_gtftextplan.hip.h"
#include "text_faults.hip.h"

using namespace l2r;

static FILE *g_out = nullptr;

static void put(const char *name, const char *type, const void *data, size_t size, int64_t count)
{
    char head[32];
    memset(head, 0, sizeof head);
    snprintf(head, 24, "%s", name);
    snprintf(head + 24, 8, "%s", type);
    fwrite(head, 1, sizeof head, g_out);
    fwrite(&count, 8, 1, g_out);
    if (count) fwrite(data, size, (size_t)count, g_out);
}
static void put_i64(const char *name, int64_t v) { put(name, "<i8", &v, 8, 1); }

// exactly `count` elements: a read beyond them is the sanitizer's to report
template <typename T> static bool get(FILE *f, std::vector<T> &v, int64_t count)
{
    if (count < 0) count = 0;
    v.assign((size_t)count, T());
    v.shrink_to_fit();
    return count == 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}

static int run(const char *in_fn, const char *out_fn)
{
    FILE *f = fopen(in_fn, "rb");
    if (!f) { perror(in_fn); return 2; }
    int64_t h[12];
    if (fread(h, 8, 12, f) != 12) { fprintf(stderr, "gtx_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], n_ex = h[1], names_len = h[2], n_ref = h[3], form = h[4], src_len = h[5], m = h[6], cols = h[7], first = h[8], max_blocks = h[9], max_bytes = h[10];
    std::vector<int32_t> tid, xs, xe, sel, start, end, cov; std::vector<uint8_t> rev, names, ref_names, src; std::vector<int64_t> ex_off, ref_off;
    std::vector<uint32_t> id[4];
    bool ok = get(f, tid, n) && get(f, rev, n) && get(f, ex_off, n + 1) && get(f, xs, n_ex) && get(f, xe, n_ex) && get(f, names, names_len);
    for (int k = 0; k < 4; ++k) ok = ok && get(f, id[k], n);
    ok = ok && get(f, ref_off, n_ref + 1) && get(f, ref_names, n_ref > 0 && ok ? ref_off[(size_t)n_ref] : 0) && get(f, src, src_len);
    ok = ok && get(f, sel, (cols & 1) ? m : 0) && get(f, start, (cols & 2) ? m : 0) && get(f, end, (cols & 4) ? m : 0) && get(f, cov, (cols & 8) ? m : 0);
    fclose(f);
    if (!ok) { fprintf(stderr, "gtx_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_gtx_params p = {(int32_t)n_ref, ref_off.data(), ref_names.empty() ? nullptr : ref_names.data(), (int32_t)form, (int32_t)src_len, src.empty() ? nullptr : src.data()};
    static const int32_t none = 0;                      // (a case without exons still has its columns: xs == NULL would mean a run's chains)
    const l2r_gtx_rows r = {n, tid.data(), rev.data(), ex_off.data(), xs.empty() ? &none : xs.data(), xe.empty() ? &none : xe.data(), names_len,
                            names.empty() ? nullptr : names.data(), id[0].data(), id[1].data(), id[2].data(), id[3].data()};
    const l2r_gtx_blocks b = {m, (cols & 1) ? sel.data() : nullptr, (cols & 2) ? start.data() : nullptr, (cols & 4) ? end.data() : nullptr, (cols & 8) ? cov.data() : nullptr};
    const GtxChains cx = {ex_off.data(), xs.data(), xe.data()};
    std::string msg;
    int rc = gtx_check_params(&p, msg);
    if (!rc) rc = gtx_check_rows(&r, p.form, msg);
    if (!rc) rc = gtx_check_blocks(&b, msg);
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    std::vector<int64_t> kind((size_t)m);
    std::vector<uint64_t> bytes((size_t)m), lines((size_t)m);
    std::vector<uint32_t> len((size_t)m);
    bool any_bad = false;
    for (int64_t q = 0; q < m; ++q) {
        kind[(size_t)q] = gtx_block_bytes(&p, &r, cx, &b, q, &bytes[(size_t)q], &lines[(size_t)q]);
        len[(size_t)q] = (uint32_t)bytes[(size_t)q];
        any_bad |= kind[(size_t)q] != GTX_OK;
    }
    put("kind", "<i8", kind.data(), 8, m); put("bytes", "<u8", bytes.data(), 8, m); put("lines", "<u8", lines.data(), 8, m);
    std::vector<uint8_t> text;
    int64_t n_lines = 0;
    if (h[11] != 0 && !any_bad) {
        uint64_t sums[2] = {0, 0}, at_byte = 0;
        double secs = 0;
        for (int64_t at = 0; at < m;) {
            int64_t take = 0, sum = 0, lines_here = 0;
            if (gtx_cut(len.data(), m, at, max_blocks, max_bytes, &take, &sum, msg) || take < 1) { fprintf(stderr, "gtx_dump: %s\n", msg.c_str()); return 2; }
            text.clear();
            const auto t0 = std::chrono::steady_clock::now();
            if (gtx_text_host(&p, &r, cx, &b, at, take, text, &lines_here, msg)) { fprintf(stderr, "gtx_dump: %s\n", msg.c_str()); return 2; }
            secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (size_t k = 0; k < text.size(); ++k, ++at_byte) { sums[0] += text[k]; sums[1] += (uint64_t)text[k] * (1u + at_byte % 251u); }
            n_lines += lines_here; at += take;
        }
        fprintf(stderr, "gtx_text_host: %lld blocks, %lld lines, %lld bytes, %.6f s\n", (long long)m, (long long)n_lines, (long long)at_byte, secs);
        put_i64("n_bytes", (int64_t)at_byte); put_i64("n_lines", n_lines); put("sums", "<u8", sums, 8, 2);
        return fclose(g_out) ? 2 : 0;
    }
    const auto t0 = std::chrono::steady_clock::now();
    rc = gtx_text_host(&p, &r, cx, &b, 0, m, text, &n_lines, msg);
    fprintf(stderr, "gtx_text_host: %lld blocks, %lld lines, %lld bytes, %.6f s\n", (long long)m, (long long)n_lines, (long long)text.size(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put_i64("text_rc", rc);
    if (rc) { put("error", "|u1", msg.data(), 1, (int64_t)msg.size()); return fclose(g_out) ? 2 : 0; }
    if (any_bad) { fprintf(stderr, "gtx_dump: gtx_text_host wrote a text over a block with an error\n"); return 2; }
    put("text", "|u1", text.data(), 1, (int64_t)text.size()); put_i64("n_lines", n_lines);
    std::vector<int64_t> cut, cut_bytes;
    std::vector<uint8_t> text_cut;
    for (int64_t at = first; at < m;) {
        int64_t take = 0, sum = 0;
        std::string cmsg;
        if (gtx_cut(len.data(), m, at, max_blocks, max_bytes, &take, &sum, cmsg)) { put("cut_error", "|u1", cmsg.data(), 1, (int64_t)cmsg.size()); return fclose(g_out) ? 2 : 0; }
        if (take < 1) { fprintf(stderr, "gtx_dump: gtx_cut took %lld blocks at %lld\n", (long long)take, (long long)at); return 2; }
        if (gtx_text_host(&p, &r, cx, &b, at, take, text_cut, nullptr, cmsg)) { fprintf(stderr, "gtx_dump: a batch failed behind a sound selection: %s\n", cmsg.c_str()); return 2; }
        cut.push_back(take); cut_bytes.push_back(sum); at += take;
    }
    put("cut", "<i8", cut.data(), 8, (int64_t)cut.size()); put("cut_bytes", "<i8", cut_bytes.data(), 8, (int64_t)cut_bytes.size());
    put("text_cut", "|u1", text_cut.data(), 1, (int64_t)text_cut.size());
    return fclose(g_out) ? 2 : 0;
}

// `gtx_dump faults`: the argument faults of l2r_gtftext_begin's reference table and of l2r_gtftext_lines (text_faults.hip.h), and
// that a bad form is reported in front of a ref_off that descends
static int faults()
{
    static const int64_t ref_off[3] = {0, 2, 4}, down[3] = {0, 3, 2};
    static const uint8_t bytes[4] = {'c', '1', 'c', '2'};
    const l2r_gtx_params sound = {2, ref_off, bytes, L2R_GTX_READ, 2, bytes};
    const auto params = [](const l2r_gtx_params *p, std::string &msg) { return gtx_check_params(p, msg); };
    text_faults::refs(sound, params);
    {   l2r_gtx_params p = sound;
        p.form = 2; p.ref_off = down;
        std::string msg; const int rc = gtx_check_params(&p, msg); text_faults::say("ref_descends_and_form_2", rc, msg);
        p.form = L2R_GTX_READ; p.ref_off = nullptr; p.src_len = -1;
        msg.clear(); const int rc2 = gtx_check_params(&p, msg); text_faults::say("ref_null_off_and_src_len_negative", rc2, msg); }
    text_faults::cuts([](const uint32_t *len, int64_t m, int64_t first, int64_t max_blocks, int64_t max_bytes, int64_t *take, int64_t *sum, std::string &msg) {
        return gtx_cut(len, m, first, max_blocks, max_bytes, take, sum, msg); });
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "faults") == 0) return faults();
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: gtx_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
