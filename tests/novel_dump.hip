// novel_dump.hip -- the host side of l2r_novel_* (lr2rmats_amd/csrc/l2r_novelplan.hip.h) as a stand-alone host program, for
// tests/test_novel_cpu.py:
//     novel_dump <case file> <output file> [<case file> <output file> ...]
// runs the predicates, the argument checks, the selection, the route test, novel_host -- the exact routine behind L2R_NOVEL_ROUTE=host --
// and the BED text, whole and cut into batches of one row.  No HIP function is called and no GPU is needed;
// `make -C lr2rmats_amd/csrc novel-dump` builds it with ASan + UBSan on the host code.
//
// Case file: fourteen int64 -- reads, exons, references, annotation transcripts, na_gene, has_sj, -s, -c, -d, -D, the bits of -f (a
// float), the bytes of the reference names, and the reads and exons an earlier add is to have left (the totals check; 0 0 in a sound
// case) -- then tid (int32), info (uint32) and ref_tx (int32) per read, xs and xe (int32) and the flags (uint8) per exon, tx_gene
// (uint32) per transcript, ref_off (int64, references + 1) and the names.  Read i has info[i] >> 8 exons, the chains lie one behind the
// other.
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements: `rc` and `error`, and as
// far as the case gets: `bits` (per read: 1 offer, 2 known, 4 split-route), `in_order`, `e_src` / `e_start` / `e_end` / `e_cov` per entry,
// `tid<l>` / `a<l>` / `b<l>` / `score<l>` / `meta<l>` per kept row of list l, `items`, `counts`, `hits`, `widened`, `bed` and `bed_cut`.
// The seconds novel_host took go to stderr (tools/bench_novel.py reads them from the build without sanitizers,
// `make -C lr2rmats_amd/csrc novel-host`).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_novelplan.hip.h"

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
static void put_i32(const char *name, const std::vector<int32_t> &v) { put(name, "<i4", v.data(), 4, (int64_t)v.size()); }

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
    int64_t h[14];
    if (fread(h, 8, 14, f) != 14) { fprintf(stderr, "novel_dump: %s: no header\n", in_fn); return 2; }
    const int64_t n = h[0], nx = h[1], n_ref = h[2], n_tx = h[3];
    l2r_params prm;
    memset(&prm, 0, sizeof prm);
    prm.split_trans = (int32_t)h[6]; prm.force_strand = (int32_t)h[7]; prm.ss_dis = (int32_t)h[8]; prm.end_dis = (int32_t)h[9];
    {   const uint32_t bits = (uint32_t)h[10];
        memcpy(&prm.single_exon_ovlp_frac, &bits, 4); }
    std::vector<int32_t> tid, ref, xs, xe; std::vector<uint32_t> info, tx_gene; std::vector<uint8_t> flag, names; std::vector<int64_t> ref_off;
    const bool ok = get(f, tid, n) && get(f, info, n) && get(f, ref, n) && get(f, xs, nx) && get(f, xe, nx) && get(f, flag, nx) && get(f, tx_gene, n_tx) && get(f, ref_off, n_ref + 1) && get(f, names, h[11]);
    fclose(f);
    if (!ok) { fprintf(stderr, "novel_dump: %s: truncated case\n", in_fn); return 2; }

    g_out = fopen(out_fn, "wb");
    if (!g_out) { perror(out_fn); return 2; }
    std::string msg;
    if (novel_check_begin(&prm, (int32_t)n_ref, ref_off.data(), names.data(), n_tx, tx_gene.data(), msg)) return refused(-1, msg);
    if (novel_check_totals(h[12], h[13], n, nx, msg)) return refused(-1, msg);
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)L2R_INFO_NEXON(info[(size_t)i]);
    // (one element of padding: a case without exons has columns too)
    xs.push_back(0); xe.push_back(0); flag.push_back(0);
    l2r_result res{n, nx, nx, off.data(), xs.data(), xe.data(), flag.data(), info.data(), ref.data()};
    if (novel_check_result(n, tid.data(), &res, msg)) return refused(-1, msg);
    const NovelPrm np{(int32_t)n_ref, n_tx, (uint32_t)h[4], (int32_t)(h[5] != 0), (int32_t)(h[6] != 0)};
    std::vector<uint8_t> bits((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t w = info[(size_t)i];
        bits[(size_t)i] = (uint8_t)((novel_offer(w, np.has_sj) ? 1 : 0) | (novel_known(w) ? 2 : 0) | (novel_split(w, np.has_sj, np.split) ? 4 : 0));
    }
    put("bits", "|u1", bits.data(), 1, n);
    NovelAcc acc;
    novel_select(acc, np, tx_gene.data(), n, tid.data(), &res);
    if (acc.bad >= 0) { novel_read_fail(msg, acc.bad, acc.bad_kind); return refused(-1, msg); }
    put_i64("split", acc.split);
    if (acc.split) return refused(-3, "split-route reads");
    put_i64("rc", 0);
    put_i64("in_order", novel_in_order(acc) ? 1 : 0);
    NovelOut out;
    const auto t0 = std::chrono::steady_clock::now();
    novel_host(acc, uniq_prm(&prm), tx_gene.data(), np.na_gene, out);
    fprintf(stderr, "novel_host: %lld reads, %lld offers, %.6f s\n", (long long)n, (long long)acc.o_tid.size(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    put_i32("e_src", out.e_src); put_i32("e_start", out.e_start); put_i32("e_end", out.e_end); put_i32("e_cov", out.e_cov);
    int64_t kept[NOV_LISTS], counts[8];
    for (int l = 0; l < NOV_LISTS; ++l) {
        const NovelRows &r = out.rows[l];
        char name[24];
        snprintf(name, sizeof name, "tid%d", l); put_i32(name, r.tid);
        snprintf(name, sizeof name, "a%d", l); put_i32(name, r.a);
        snprintf(name, sizeof name, "b%d", l); put_i32(name, r.b);
        snprintf(name, sizeof name, "score%d", l); put_i32(name, r.score);
        snprintf(name, sizeof name, "meta%d", l); put(name, "|u1", r.meta.data(), 1, (int64_t)r.meta.size());
        kept[l] = (int64_t)r.tid.size();
    }
    novel_counts(kept, (int64_t)out.e_src.size(), counts);
    put("items", "<i8", out.items, 8, NOV_LISTS);
    put("counts", "<i8", counts, 8, 8);
    put_i64("hits", out.u.hits[0] + out.u.hits[1] + out.u.hits[2]);
    put_i64("widened", out.widened);
    // the text whole, and cut into batches of one row: the measured lengths, the cut, the lines
    const NovelRows &E = out.rows[NOV_EXON];
    std::vector<uint8_t> text, cut, part;
    novel_bed_host(E, ref_off.data(), names.data(), 0, kept[NOV_EXON], text);
    std::vector<uint32_t> len((size_t)kept[NOV_EXON]);
    for (size_t q = 0; q < len.size(); ++q) len[q] = novel_bed_bytes(ref_off.data(), E.tid[q], E.a[q], E.b[q], E.score[q]);
    for (int64_t first = 0; first < kept[NOV_EXON];) {
        int64_t take = 0, bytes = 0;
        if (novel_cut(len.data(), kept[NOV_EXON], first, 1, 1, &take, &bytes, msg) || take != 1) return refused(-2, msg);
        novel_bed_host(E, ref_off.data(), names.data(), first, take, part);
        if ((int64_t)part.size() != bytes) return refused(-2, "a line's bytes differ from its measure");
        cut.insert(cut.end(), part.begin(), part.end());
        first += take;
    }
    put("bed", "|u1", text.data(), 1, (int64_t)text.size());
    put("bed_cut", "|u1", cut.data(), 1, (int64_t)cut.size());
    return fclose(g_out) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: novel_dump <case file> <output file> [<case file> <output file> ...]\n"); return 2; }
    for (int k = 1; k + 1 < argc; k += 2) { const int rc = run(argv[k], argv[k + 1]); if (rc) return rc; }
    return 0;
}
