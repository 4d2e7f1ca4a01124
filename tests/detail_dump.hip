// detail_dump.hip -- the host side of l2r_detail_* (lr2rmats_amd/csrc/l2r_detailplan.hip.h) as a stand-alone host program, for
// tests/test_detail_cpu.py:
//     detail_dump <case file> <output file> [<case file> <output file> ...]
//     detail_dump faults        (one line per argument fault of l2r_detail_begin, l2r_detail_rows and l2r_detail_lines: tests/text_faults.hip.h)
// runs the argument checks, detail_line_bytes of every read, detail_cut from the case's first row to the last, and detail_text_host, the
// exact routine behind L2R_DETAIL_ROUTE=host, over all the rows and batch by batch.  No HIP function is called and no GPU is needed;
// `make -C lr2rmats_amd/csrc detail-dump` builds it with ASan + UBSan on the host code.
//
// Case file: thirteen int64 -- reads, exons, bytes of the names table, reference names, annotation transcripts, bytes of the annotation's
// names table, first row of the cuts, max_rows, max_bytes, made-up lengths, n_reads and n_exons of the results (-1: reads, exons),
// sums_only -- then tid (int32), qname (uint32), the names table, ex_off (int64, n + 1), info (uint32), ref_tx (int32), xs and xe (int32),
// the flags (uint8), ref_off (int64, n_ref + 1), the reference name bytes, the annotation's names table, tx_gid and tx_gname (uint32),
// and the made-up lengths (uint32).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` of the checks and
// `error`, or per read `kind`, `bytes` and `split` (six words each); with made-up lengths `fake_cut` and `fake_cut_bytes` (detail_cut over
// them from the first row on) or `fake_cut_error`; then, where no read has an error, `text`, `cut` (the rows each batch took),
// `cut_bytes` and `text_cut` (the batches' texts concatenated); else `text_rc` and `error` of detail_text_host.  The seconds
// detail_text_host took go to stderr (tools/bench_detail.py reads them from the build without sanitizers, `make -C lr2rmats_amd/csrc
// detail-host`).  sums_only != 0 (a text of gigabytes): only `n_bytes` and `sums` leave -- the sum of its bytes and the sum of
// byte * (1 + position mod 251).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_detailplan.hip.h"
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
    int64_t h[13];
    if (fread(h, 8, 13, f) != 13) { fprintf(stderr, "detail_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], n_ex = h[1], names_len = h[2], n_ref = h[3], n_tx = h[4], anno_len = h[5], first = h[6], max_rows = h[7], max_bytes = h[8], n_fake = h[9];
    std::vector<int32_t> tid, ref_tx, xs, xe; std::vector<uint32_t> qname, info, tx_gid, tx_gname, fake; std::vector<uint8_t> names, flags, ref_names, anno; std::vector<int64_t> ex_off, ref_off;
    bool ok = get(f, tid, n) && get(f, qname, n) && get(f, names, names_len) && get(f, ex_off, n + 1) && get(f, info, n) && get(f, ref_tx, n) && get(f, xs, n_ex) && get(f, xe, n_ex) &&
              get(f, flags, n_ex) && get(f, ref_off, n_ref + 1);
    ok = ok && get(f, ref_names, n_ref > 0 ? ref_off[(size_t)n_ref] : 0) && get(f, anno, anno_len) && get(f, tx_gid, n_tx) && get(f, tx_gname, n_tx) && get(f, fake, n_fake);
    fclose(f);
    if (!ok) { fprintf(stderr, "detail_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_detail_params p = {(int32_t)n_ref, ref_off.data(), ref_names.empty() ? nullptr : ref_names.data(), n_tx, anno_len, anno.empty() ? nullptr : anno.data(),
                                 tx_gid.data(), tx_gname.data()};
    const l2r_result res = {h[10] < 0 ? n : h[10], n_ex, h[11] < 0 ? n_ex : h[11], ex_off.data(), xs.data(), xe.data(), flags.data(), info.data(), ref_tx.data()};
    const l2r_detail_reads r = {n, tid.data(), names_len, names.empty() ? nullptr : names.data(), qname.data(), &res};
    std::string msg;
    int rc = detail_check_params(&p, msg);
    if (!rc) rc = detail_check_rows(&r, msg);
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    std::vector<int64_t> kind((size_t)n);
    std::vector<uint64_t> bytes((size_t)n);
    std::vector<uint32_t> len((size_t)n), split((size_t)n * DETAIL_SPLIT);
    bool any_bad = false;
    for (int64_t i = 0; i < n; ++i) {
        kind[(size_t)i] = detail_line_bytes(&p, &r, i, &bytes[(size_t)i], split.data() + (size_t)i * DETAIL_SPLIT);
        len[(size_t)i] = (uint32_t)bytes[(size_t)i];
        any_bad |= kind[(size_t)i] != DET_OK;
    }
    put("kind", "<i8", kind.data(), 8, n); put("bytes", "<u8", bytes.data(), 8, n); put("split", "<u4", split.data(), 4, n * DETAIL_SPLIT);
    if (n_fake > 0) {
        std::vector<int64_t> cut, cut_bytes;
        std::string cmsg;
        for (int64_t at = first;;) {
            int64_t take = 0, sum = 0;
            if (detail_cut(fake.data(), n_fake, at, max_rows, max_bytes, &take, &sum, cmsg)) { put("fake_cut_error", "|u1", cmsg.data(), 1, (int64_t)cmsg.size()); break; }
            if (take < 1) { fprintf(stderr, "detail_dump: detail_cut took %lld rows at %lld\n", (long long)take, (long long)at); return 2; }
            cut.push_back(take); cut_bytes.push_back(sum); at += take;
            if (at >= n_fake) break;
        }
        put("fake_cut", "<i8", cut.data(), 8, (int64_t)cut.size()); put("fake_cut_bytes", "<i8", cut_bytes.data(), 8, (int64_t)cut_bytes.size());
    }
    std::vector<uint8_t> text;
    if (h[12] != 0 && !any_bad) {
        uint64_t sums[2] = {0, 0}, at_byte = 0;
        double secs = 0;
        for (int64_t at = 0; at < n;) {
            int64_t take = 0, sum = 0;
            if (detail_cut(len.data(), n, at, max_rows, max_bytes, &take, &sum, msg) || take < 1) { fprintf(stderr, "detail_dump: %s\n", msg.c_str()); return 2; }
            text.clear();
            const auto t0 = std::chrono::steady_clock::now();
            if (detail_text_host(&p, &r, at, take, text, msg)) { fprintf(stderr, "detail_dump: %s\n", msg.c_str()); return 2; }
            secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (size_t k = 0; k < text.size(); ++k, ++at_byte) { sums[0] += text[k]; sums[1] += (uint64_t)text[k] * (1u + at_byte % 251u); }
            at += take;
        }
        fprintf(stderr, "detail_text_host: %lld rows, %lld bytes, %.6f s\n", (long long)n, (long long)at_byte, secs);
        put_i64("n_bytes", (int64_t)at_byte); put("sums", "<u8", sums, 8, 2);
        return fclose(g_out) ? 2 : 0;
    }
    const auto t0 = std::chrono::steady_clock::now();
    rc = detail_text_host(&p, &r, 0, n, text, msg);
    fprintf(stderr, "detail_text_host: %lld rows, %lld bytes, %.6f s\n", (long long)n, (long long)text.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put_i64("text_rc", rc);
    if (rc) { put("error", "|u1", msg.data(), 1, (int64_t)msg.size()); return fclose(g_out) ? 2 : 0; }
    if (any_bad) { fprintf(stderr, "detail_dump: detail_text_host wrote a text over a read with an error\n"); return 2; }
    put("text", "|u1", text.data(), 1, (int64_t)text.size());
    std::vector<int64_t> cut, cut_bytes;
    std::vector<uint8_t> text_cut;
    for (int64_t at = first; at < n;) {
        int64_t take = 0, sum = 0;
        std::string cmsg;
        if (detail_cut(len.data(), n, at, max_rows, max_bytes, &take, &sum, cmsg)) { put("cut_error", "|u1", cmsg.data(), 1, (int64_t)cmsg.size()); return fclose(g_out) ? 2 : 0; }
        if (take < 1) { fprintf(stderr, "detail_dump: detail_cut took %lld rows at %lld\n", (long long)take, (long long)at); return 2; }
        if (detail_text_host(&p, &r, at, take, text_cut, cmsg)) { fprintf(stderr, "detail_dump: a batch failed behind sound rows: %s\n", cmsg.c_str()); return 2; }
        cut.push_back(take); cut_bytes.push_back(sum); at += take;
    }
    put("cut", "<i8", cut.data(), 8, (int64_t)cut.size()); put("cut_bytes", "<i8", cut_bytes.data(), 8, (int64_t)cut_bytes.size());
    put("text_cut", "|u1", text_cut.data(), 1, (int64_t)text_cut.size());
    return fclose(g_out) ? 2 : 0;
}

// `detail_dump faults`: the argument faults of l2r_detail_begin, l2r_detail_rows and l2r_detail_lines (text_faults.hip.h)
static int faults()
{
    static const int64_t ref_off[3] = {0, 2, 4};
    static const uint8_t bytes[4] = {'c', '1', 'c', '2'};
    static const uint32_t ids[2] = {0, 2};
    const l2r_detail_params sound = {2, ref_off, bytes, 2, 4, bytes, ids, ids};
    const auto params = [](const l2r_detail_params *p, std::string &msg) { return detail_check_params(p, msg); };
    { std::string msg; const int rc = detail_check_params(nullptr, msg); text_faults::say("params_null", rc, msg); }
    text_faults::refs(sound, params);
    text_faults::genes(sound, params);
    text_faults::reads<l2r_detail_reads>([](const l2r_detail_reads *r, std::string &msg) { return detail_check_rows(r, msg); });
    text_faults::cuts([](const uint32_t *len, int64_t m, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *take, int64_t *sum, std::string &msg) {
        return detail_cut(len, m, first, max_rows, max_bytes, take, sum, msg); });
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "faults") == 0) return faults();
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: detail_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
