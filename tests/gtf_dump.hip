// gtf_dump.hip -- the host side of l2r_gtf_order (lr2rmats_amd/csrc/l2r_gtforder.hip.h) as a stand-alone host program, for
// tests/test_gtf_order_cpu.py:
//     gtf_dump <text file> <output file> [<text file> <output file> ...]
// runs the argument checks and then gtf_order_host, the exact routine the engine takes beyond one device call and `sort-gtf-check` runs,
// and ranks the text's heads with gtf_rank_heads as the engine does for the device.  No HIP function is called and no GPU is needed;
// `make -C lr2rmats_amd/csrc gtf-dump` builds it with ASan + UBSan on the host code.
//
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc`, then `start`, `len`,
// `line`, `counts` (lines, transcript lines, heads, names beyond the table, distinct names, the first descending line) and `head_rank`,
// or for a rejected text `error`.  The seconds gtf_order_host took go to stderr (tools/bench_gtf.py reads them from the build without
// sanitizers, `make -C lr2rmats_amd/csrc gtf-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_gtforder.hip.h"

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

static int run(const char *in_fn, const char *out_fn)
{
    FILE *f = fopen(in_fn, "rb");
    if (!f) { perror(in_fn); return 2; }
    std::vector<uint8_t> bytes;
    {   uint8_t buf[65536]; size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + k); }
    fclose(f);
    // exactly the bytes of the text: a read beyond them is the sanitizer's to report
    std::vector<uint8_t> text(bytes);
    text.shrink_to_fit();

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_gtf_text t = {(int64_t)text.size(), text.empty() ? nullptr : text.data()};
    int64_t n_rows = 0;
    std::string msg;
    int rc = gtf_check(&t, &n_rows, msg);
    GtfOrder o;
    const auto t0 = std::chrono::steady_clock::now();
    if (!rc) rc = gtf_order_host(t.text, (uint64_t)t.n_bytes, o, msg);
    fprintf(stderr, "gtf_order_host: %lld bytes, %lld lines, %lld rows, %.6f s\n", (long long)t.n_bytes, (long long)o.n_lines, (long long)o.start.size(),
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    put("start", "<u8", o.start.data(), 8, (int64_t)o.start.size());
    put("len", "<u4", o.len.data(), 4, (int64_t)o.len.size());
    put("line", "<u4", o.line.data(), 4, (int64_t)o.line.size());
    const int64_t counts[6] = {o.n_lines, o.n_tx, o.n_heads, o.n_beyond, o.n_names, o.descent_line};
    put("counts", "<i8", counts, 8, 6);
    // the heads as the device finds them (a transcript line whose first field differs from the previous transcript line's), ranked
    std::vector<uint32_t> off, len;
    {   uint64_t pf = 0, pl = 0;
        for (uint64_t p = 0; p < text.size();) {
            const uint8_t *nl = (const uint8_t *)memchr(text.data() + p, '\n', text.size() - p);
            const uint64_t q = nl ? (uint64_t)(nl - text.data()) : text.size();
            const GtfLine g = gtf_line(text.data(), p, q);
            if (g.tx && (off.empty() || g.f1_len != pl || memcmp(text.data() + g.f1, text.data() + pf, (size_t)pl) != 0)) { off.push_back((uint32_t)g.f1); len.push_back((uint32_t)g.f1_len); }
            if (g.tx) { pf = g.f1; pl = g.f1_len; }
            p = q + 1;
        } }
    std::vector<uint32_t> rank(off.size());
    GtfChrRanks ranks;
    if (gtf_rank_heads(text.data(), text.size(), off.data(), len.data(), off.size(), rank.data(), ranks)) { fprintf(stderr, "gtf_dump: a head beyond the text\n"); return 2; }
    put("head_rank", "<u4", rank.data(), 4, (int64_t)rank.size());
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: gtf_dump <text file> <output file> [<text file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
