// bed_dump.hip -- the host side of l2r_bed_lines (lr2rmats_amd/csrc/l2r_bedplan.hip.h) as a stand-alone host program, for
// tests/test_bed12_cpu.py:
//     bed_dump <case file> <output file> [<case file> <output file> ...]
// runs the argument checks, bed_line_bound of every record, bed_cut from the case's first record to its last, and bed_lines_host, the
// exact routine behind L2R_BED_ROUTE=host.  No HIP function is called and no GPU is needed; `make -C lr2rmats_amd/csrc bed-dump` builds
// it with ASan + UBSan on the host code.
//
// Case file: eight int64 -- records, CIGAR words, reference names, colour bytes, first record of the cuts, max_records, max_bytes,
// counts_only -- then flag (uint16), tid, pos (int32), mapq (uint8), cig_off (int64, n + 1), the CIGAR words (uint32), name_off (int64,
// n + 1), the name bytes, ref_off (int64, n_ref + 1), the reference name bytes and the colour.  counts_only != 0: the file holds no CIGAR
// words and no name bytes (a record described by its counts: only the bounds and the cuts are made, which read neither).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` of the checks, `bound`,
// `cut` (the records each batch took) or `cut_error`, and `text` with `n_lines`, or `error`.  The seconds bed_lines_host took go to
// stderr (tools/bench_bed.py reads them from the build without sanitizers, `make -C lr2rmats_amd/csrc bed-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_bedplan.hip.h"

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
    if (count < 0) count = 0;                           // (a case whose offsets descend: the checks say so)
    v.assign((size_t)count, T());
    v.shrink_to_fit();
    return count == 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}

static int run(const char *in_fn, const char *out_fn)
{
    FILE *f = fopen(in_fn, "rb");
    if (!f) { perror(in_fn); return 2; }
    int64_t h[8];
    if (fread(h, 8, 8, f) != 8) { fprintf(stderr, "bed_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], n_cigar = h[1], n_ref = h[2], color_len = h[3], first = h[4], max_records = h[5], max_bytes = h[6];
    const bool counts_only = h[7] != 0;
    std::vector<uint16_t> flag; std::vector<int32_t> tid, pos; std::vector<uint8_t> mapq, names, ref_names, color; std::vector<int64_t> cig_off, name_off, ref_off;
    std::vector<uint32_t> cig;
    bool ok = get(f, flag, n) && get(f, tid, n) && get(f, pos, n) && get(f, mapq, n) && get(f, cig_off, n + 1) && get(f, cig, counts_only ? 0 : n_cigar) && get(f, name_off, n + 1);
    ok = ok && get(f, names, counts_only ? 0 : name_off[(size_t)n] - name_off[0]) && get(f, ref_off, n_ref + 1);
    ok = ok && get(f, ref_names, ref_off[(size_t)n_ref]) && get(f, color, color_len);
    fclose(f);
    if (!ok || color_len > 12) { fprintf(stderr, "bed_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    l2r_bed_params p;
    memset(&p, 0, sizeof p);
    p.n_ref = (int32_t)n_ref; p.ref_off = ref_off.data(); p.ref_names = ref_names.empty() ? nullptr : ref_names.data(); p.color_len = (int32_t)color_len;
    if (color_len) memcpy(p.color, color.data(), (size_t)color_len);
    // (the names are addressed from name_off[0]: the case holds the window's bytes only)
    const l2r_bed_records r = {n, n_cigar, flag.data(), tid.data(), pos.data(), mapq.data(), cig_off.data(), cig.empty() ? nullptr : cig.data(), name_off.data(),
                               names.empty() ? nullptr : names.data() - name_off[0]};
    std::string msg;
    int rc = bed_check_params(&p, msg);
    if (!rc) rc = bed_check_records(&r, msg, "l2r_bed_lines", !counts_only);
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    std::vector<uint64_t> bound((size_t)n);
    for (int64_t i = 0; i < n; ++i) bound[(size_t)i] = bed_line_bound(&r, &p, i);
    put("bound", "<u8", bound.data(), 8, n);
    {   std::vector<int64_t> cut;
        std::string cmsg;
        int crc = 0;
        for (int64_t at = first; at < n && !crc;) {
            int64_t take = 0;
            crc = bed_cut(&r, &p, at, max_records, max_bytes, &take, cmsg);
            if (!crc && take < 1) { fprintf(stderr, "bed_dump: bed_cut took %lld records at %lld\n", (long long)take, (long long)at); return 2; }
            if (!crc) { cut.push_back(take); at += take; }
        }
        if (crc) put("cut_error", "|u1", cmsg.data(), 1, (int64_t)cmsg.size());
        else put("cut", "<i8", cut.data(), 8, (int64_t)cut.size()); }
    if (!counts_only) {
        std::vector<uint8_t> text;
        int64_t n_lines = 0;
        const auto t0 = std::chrono::steady_clock::now();
        rc = bed_lines_host(&r, &p, text, &n_lines, msg);
        fprintf(stderr, "bed_lines_host: %lld records, %lld lines, %lld bytes, %.6f s\n", (long long)n, (long long)n_lines, (long long)text.size(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        put_i64("lines_rc", rc);
        if (rc) put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        else { put("text", "|u1", text.data(), 1, (int64_t)text.size()); put_i64("n_lines", n_lines); }
    }
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: bed_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
