// summary_dump.hip -- the host side of l2r_summary_* (lr2rmats_amd/csrc/l2r_summaryplan.hip.h) as a stand-alone host program, for
// tests/test_summary_cpu.py:
//     summary_dump <case file> <output file> [<case file> <output file> ...]
// runs the class function, the argument checks, the route test and summary_host, the exact routine behind L2R_SUMMARY_ROUTE=host.  No HIP
// function is called and no GPU is needed; `make -C lr2rmats_amd/csrc summary-dump` builds it with ASan + UBSan on the host code.
//
// Case file: eight int64 -- reads, exons, -s, -d, -D, the bits of -f (a float), reads and exons that an earlier add is to have left (the
// totals check; 0 0 in a sound case) -- then tid (int32) and info (uint32) per read, xs and xe (int32, `exons` each).  Read i has
// info[i] >> 8 exons, the chains lie one behind the other.
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` and `error`, or `class`
// (per read), `in_order` and `counts` (the reads of the four classes, then their unique transcripts).  The seconds summary_host took go to
// stderr (tools/bench_summary.py reads them from the build without sanitizers, `make -C lr2rmats_amd/csrc summary-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_summaryplan.hip.h"

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

static int refused(int rc, const std::string &msg)
{
    put_i64("rc", rc);
    put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
    return fclose(g_out) ? 2 : 0;
}

static int run(const char *in_fn, const char *out_fn)
{
    FILE *f = fopen(in_fn, "rb");
    if (!f) { perror(in_fn); return 2; }
    int64_t h[8];
    if (fread(h, 8, 8, f) != 8) { fprintf(stderr, "summary_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], nx = h[1];
    l2r_params prm;
    memset(&prm, 0, sizeof prm);
    prm.force_strand = (int32_t)h[2]; prm.ss_dis = (int32_t)h[3]; prm.end_dis = (int32_t)h[4];
    {   const uint32_t bits = (uint32_t)h[5];
        memcpy(&prm.single_exon_ovlp_frac, &bits, 4); }
    std::vector<int32_t> tid, xs, xe; std::vector<uint32_t> info;
    const bool ok = get(f, tid, n) && get(f, info, n) && get(f, xs, nx) && get(f, xe, nx);
    fclose(f);
    if (!ok) { fprintf(stderr, "summary_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    std::string msg;
    if (summary_check_totals(h[6], h[7], n, nx, msg)) return refused(-1, msg);
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)L2R_INFO_NEXON(info[(size_t)i]);
    {   // the arrays as an l2r_download would have left them
        std::vector<uint8_t> flag((size_t)nx + 1, 0); std::vector<int32_t> ref((size_t)n + 1, -1);
        l2r_result res{n, nx, nx, off.data(), xs.data(), xe.data(), flag.data(), info.data(), ref.data()};
        if (summary_check_result(n, tid.data(), &res, msg)) return refused(-1, msg); }
    const SummaryReads r{n, tid.data(), info.data(), off.data(), xs.data(), xe.data()};
    if (summary_check(r, msg)) return refused(-1, msg);
    put_i64("rc", 0);
    std::vector<uint8_t> cls((size_t)n);
    for (int64_t i = 0; i < n; ++i) cls[(size_t)i] = (uint8_t)summary_class(info[(size_t)i]);
    put("class", "|u1", cls.data(), 1, n);
    put_i64("in_order", summary_in_order(r) ? 1 : 0);
    int64_t counts[8];
    const auto t0 = std::chrono::steady_clock::now();
    summary_host(r, uniq_prm(&prm), counts);
    fprintf(stderr, "summary_host: %lld reads, %.6f s\n", (long long)n, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put("counts", "<i8", counts, 8, 8);
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: summary_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
