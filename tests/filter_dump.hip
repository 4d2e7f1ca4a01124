// filter_dump.hip -- the host side of `filter` and `fusion` (lr2rmats_amd/csrc/l2r_filterplan.hip.h) as a stand-alone host program, for
// tests/test_filter_plan_cpu.py:
//     filter_dump <case file> <output file> [<case file> <output file> ...]
// builds the table of the -r transcripts (filter_spans_build), answers a list of probes with filter_span_hit -- the function
// k_filter_score calls -- and runs one of the four argument checks.  No HIP function is called and no GPU is needed;
// `make -C lr2rmats_amd/csrc filter-dump` builds it with ASan + UBSan on the host code.
//
// Case file: eight int64 -- transcripts, probes, the check to run (0 none, 1 l2r_filter_score, 2 l2r_filter_select,
// 3 l2r_fusion_segments, 4 l2r_fusion_select), its n (records or groups), n_cigar, the words of cig_off / group_off in the file, a mask
// of the pointers handed over as NULL (bit k = the k-th pointer of the list below), 1 where the span table is handed over with NULL
// columns -- then tid, start, end (int32, `transcripts` each), the probes (tid, lo, hi: int32, three a probe), the offsets (int64).
//     check 1: ctx, recs, prm, drop, score, intron_n, flag, tid, pos, l_qseq, nm, cig_off, cig
//     check 2: ctx, prm, group_off, score, intron_n, winner
//     check 3: ctx, recs, read_start, read_end, ref_start, ref_end, qlen, flag, pos, cig_off, cig
//     check 4: ctx, prm, group_off, score, ed, tid, read_start, read_end, ref_start, ref_end, rlen_of_group, first, second
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `n_tid`, `off`, `start`,
// `pmax_end`, `hit` (one byte a probe), and with a check `rc` and `error`.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_filterplan.hip.h"

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
    if (fread(h, 8, 8, f) != 8) { fprintf(stderr, "filter_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n_tx = h[0], n_probe = h[1], check = h[2], n = h[3], n_cigar = h[4], n_off = h[5];
    const uint64_t null_mask = (uint64_t)h[6];
    std::vector<int32_t> tid, start, end, probe; std::vector<int64_t> offs;
    const bool ok = get(f, tid, n_tx) && get(f, start, n_tx) && get(f, end, n_tx) && get(f, probe, 3 * n_probe) && get(f, offs, n_off);
    fclose(f);
    if (!ok) { fprintf(stderr, "filter_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    const l2r_filter_spans rm = {n_tx, h[7] ? nullptr : tid.data(), h[7] ? nullptr : start.data(), h[7] ? nullptr : end.data()};
    FilterSpanTable t;
    filter_spans_build(h[7] ? nullptr : &rm, t);
    put_i64("n_tid", t.n_tid);
    put("off", "<i8", t.off.data(), 8, (int64_t)t.off.size());
    put("start", "<i4", t.start.data(), 4, (int64_t)t.start.size());
    put("pmax_end", "<i4", t.pmax_end.data(), 4, (int64_t)t.pmax_end.size());
    std::vector<uint8_t> hit((size_t)n_probe);
    for (int64_t k = 0; k < n_probe; ++k)
        hit[(size_t)k] = filter_span_hit(t.off.data(), t.start.data(), t.pmax_end.data(), t.n_tid, probe[(size_t)(3 * k)], probe[(size_t)(3 * k + 1)], probe[(size_t)(3 * k + 2)]);
    put("hit", "|u1", hit.data(), 1, n_probe);

    if (check) {
        // the checks read the offsets only; of every other pointer they ask whether it is NULL
        int32_t word = 0;
        int dummy = 0;
        int bit = 0;
        auto ptr = [&](const void *p) { return (null_mask >> bit++) & 1u ? nullptr : p; };
        const l2r_filter_params fprm = {0.67f, 0.75f, 0.98f, 0};
        const l2r_fusion_params uprm = {0.1f, 0.1f, 0.99f, 100000};
        std::string msg;
        int rc = 0;
        if (check == 1) {
            const void *ctx = ptr(&dummy), *recs = ptr(&dummy), *prm = ptr(&fprm), *drop = ptr(&word), *score = ptr(&word), *intron = ptr(&word);
            l2r_filter_records r = {n, n_cigar, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            r.flag = (const uint16_t *)ptr(&word); r.tid = (const int32_t *)ptr(&word); r.pos = (const int32_t *)ptr(&word);
            r.l_qseq = (const int32_t *)ptr(&word); r.nm = (const int32_t *)ptr(&word);
            r.cig_off = (const int64_t *)ptr(offs.data()); r.cig = (const uint32_t *)ptr(&word);
            rc = filter_score_check(ctx, recs ? &r : nullptr, (const l2r_filter_params *)prm, &rm, drop, score, intron, msg);
        } else if (check == 2) {
            const void *ctx = ptr(&dummy), *prm = ptr(&fprm), *goff = ptr(offs.data()), *score = ptr(&word), *intron = ptr(&word), *winner = ptr(&word);
            rc = filter_select_check(ctx, n, (const int64_t *)goff, (const int32_t *)score, (const int32_t *)intron, (const l2r_filter_params *)prm, winner, msg);
        } else if (check == 3) {
            const void *ctx = ptr(&dummy), *recs = ptr(&dummy), *o[5];
            for (int k = 0; k < 5; ++k) o[k] = ptr(&word);
            l2r_fusion_records r = {n, n_cigar, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            r.flag = (const uint16_t *)ptr(&word); r.pos = (const int32_t *)ptr(&word);
            r.cig_off = (const int64_t *)ptr(offs.data()); r.cig = (const uint32_t *)ptr(&word);
            rc = fusion_segments_check(ctx, recs ? &r : nullptr, o[0], o[1], o[2], o[3], o[4], msg);
        } else if (check == 4) {
            const void *ctx = ptr(&dummy), *prm = ptr(&uprm), *goff = ptr(offs.data());
            const int32_t *col[8];
            for (int k = 0; k < 8; ++k) col[k] = (const int32_t *)ptr(&word);
            const void *first = ptr(&word), *second = ptr(&word);
            rc = fusion_select_check(ctx, n, (const int64_t *)goff, col[0], col[1], col[2], col[3], col[4], col[5], col[6], col[7],
                                     (const l2r_fusion_params *)prm, first, second, msg);
        } else { fprintf(stderr, "filter_dump: %s: check %lld\n", in_fn, (long long)check); fclose(g_out); return 2; }
        put_i64("rc", rc);
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
    }
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: filter_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
