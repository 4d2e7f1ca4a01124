// uniq_dump.hip -- the host side of l2r_uniq_merge (lr2rmats_amd/csrc/l2r_uniqplan.hip.h) as a stand-alone host program, for
// tests/test_uniq_cpu.py:
//     uniq_dump <case file> <output file> [<case file> <output file> ...]
// runs the argument checks, the route test, the cluster cut (where the input is in order) and uniq_host, the exact routine behind
// L2R_UNIQ_ROUTE=host.  No HIP function is called and no GPU is needed; `make -C lr2rmats_amd/csrc uniq-dump` builds it with ASan + UBSan
// on the host code.
//
// Case file: eight int64 -- transcripts, exons, -s, -d, -D, the bits of -f (a float), words of ex_off in the file (n + 1 in a sound case),
// 0 -- then tid (int32), rev (uint8), ex_off (int64), xs and xe (int32, `exons` each).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` of the checks and
// `error`, or `in_order`, `head` / `n_clusters` / `largest` (in order only), `merged`, `uniq_of`, `u_src`, `u_start`, `u_end`, `u_cov`,
// `hits` (identical, contained, single) and `end_ext`.  The seconds uniq_host took go to stderr (tools/bench_uniq.py reads them from the
// build without sanitizers, `make -C lr2rmats_amd/csrc uniq-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_uniqplan.hip.h"

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
    int64_t h[8];
    if (fread(h, 8, 8, f) != 8) { fprintf(stderr, "uniq_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], nx = h[1], n_off = h[6];
    l2r_params prm;
    memset(&prm, 0, sizeof prm);
    prm.force_strand = (int32_t)h[2]; prm.ss_dis = (int32_t)h[3]; prm.end_dis = (int32_t)h[4];
    {   const uint32_t bits = (uint32_t)h[5];
        memcpy(&prm.single_exon_ovlp_frac, &bits, 4); }
    std::vector<int32_t> tid, xs, xe; std::vector<uint8_t> rev; std::vector<int64_t> ex_off;
    const int64_t n_cols = n < ((int64_t)1 << 31) ? n : 1;      // (a count the checks refuse: the file holds one transcript)
    const bool ok = get(f, tid, n_cols) && get(f, rev, n_cols) && get(f, ex_off, n_off) && get(f, xs, nx) && get(f, xe, nx);
    fclose(f);
    if (!ok) { fprintf(stderr, "uniq_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_uniq_trans t = {n, tid.empty() ? nullptr : tid.data(), rev.empty() ? nullptr : rev.data(), ex_off.empty() ? nullptr : ex_off.data(),
                              xs.empty() ? nullptr : xs.data(), xe.empty() ? nullptr : xe.data()};
    std::string msg;
    const int rc = uniq_check(&t, msg);
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    const bool in_order = uniq_in_order(&t);
    put_i64("in_order", in_order ? 1 : 0);
    if (in_order) {
        std::vector<uint8_t> head;
        int64_t n_c = 0, big = 0;
        uniq_clusters(&t, head, &n_c, &big);
        put("head", "|u1", head.data(), 1, n);
        put_i64("n_clusters", n_c); put_i64("largest", big);
    }
    UniqResult r;
    const auto t0 = std::chrono::steady_clock::now();
    uniq_host(&t, uniq_prm(&prm), r);
    fprintf(stderr, "uniq_host: %lld transcripts, %lld unique, %.6f s\n", (long long)n, (long long)r.u_src.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    const int64_t u = (int64_t)r.u_src.size();
    put("merged", "|u1", r.merged.data(), 1, n); put("uniq_of", "<i4", r.uniq_of.data(), 4, n);
    put("u_src", "<i4", r.u_src.data(), 4, u); put("u_start", "<i4", r.u_start.data(), 4, u); put("u_end", "<i4", r.u_end.data(), 4, u); put("u_cov", "<i4", r.u_cov.data(), 4, u);
    put("hits", "<i8", r.hits, 8, 3); put_i64("end_ext", r.end_ext);
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: uniq_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
