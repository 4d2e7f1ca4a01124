// tables_dump.hip -- the annotation's and the junction table's tables (lr2rmats_amd/csrc/l2r_tables.hip.h) as a stand-alone host program, for
// tests/test_tables_cpu.py:
//     tables_dump <case file> <output file> [cache dir]
// reads one annotation and / or one junction table, derives their tables through the same steps as l2r_set_annotation and
// l2r_set_junctions -- with a cache dir through the cache's load / build / store -- and writes every member of them; with reads, the two
// host cursors per read as well.  No HIP function is called and no GPU is needed; `make -C lr2rmats_amd/csrc tables-dump` builds it with
// ASan + UBSan on the host code.
//
// Case file (little endian): 12 int64 -- annotation present, n_tx, n_exon, junction table present, n_sj, n_reads, the annotation cursor
// and the junction cursor a replay starts from, 0, 0, 0, 0 -- then, if present, the annotation: tx_tid, tx_start, tx_end (int32 [n_tx]),
// tx_rev (uint8 [n_tx]), tx_ex_off (int64 [n_tx + 1]), ex_start, ex_end (int32 [n_exon]); if present, the junction table: tid, don, acc,
// uniq_c, multi_c (int32 [n_sj]); then the reads: tid, pos (int32 [n_reads]) and one byte each, "reaches the junction check".
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements.  A rejected case gives
// `rc` and `error` alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_kernels.hip.h"
#include "../lr2rmats_amd/csrc/l2r_tables.hip.h"

using namespace l2r;

static_assert(sizeof(TxHdr) == 48 && sizeof(SiteEnt) == 32, "the members below are written as 12 and 8 words");

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
template <typename T> static void put_vec(const char *name, const char *type, const std::vector<T> &v, size_t per = 1)
{
    put(name, type, v.data(), sizeof(T) / per, (int64_t)(v.size() * per));
}

template <typename T> static bool get(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// the two host cursors for every read: after a sorted upload that ends with it, and replayed over the reads in file order
static void put_cursors(const char *after, const char *replay, const char *end, const std::vector<int64_t> &key, const std::vector<int64_t> &key_raw, int64_t from,
                        const std::vector<int32_t> &tid, const std::vector<int32_t> &pos, const uint8_t *moves)
{
    const int64_t R = (int64_t)tid.size();
    std::vector<int64_t> at((size_t)R);
    for (int64_t i = 0; i < R; ++i) at[(size_t)i] = cursor_after(key, tid[(size_t)i], pos[(size_t)i]);
    std::vector<int32_t> seen((size_t)R);
    const int64_t cur = cursor_replay(key_raw, from, tid.data(), pos.data(), R, seen.data(), [&](int64_t i) { return !moves || moves[i] != 0; });
    put_vec(after, "<i8", at); put_vec(replay, "<i4", seen); put_i64(end, cur);
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: tables_dump <case file> <output file> [cache dir]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t h[12];
    if (fread(h, 8, 12, f) != 12 || h[1] < 0 || h[2] < 0 || h[4] < 0 || h[5] < 0) { fprintf(stderr, "tables_dump: bad header\n"); return 2; }
    const bool has_anno = h[0] != 0, has_sj = h[3] != 0;
    const size_t T = (size_t)h[1], X = (size_t)h[2], S = (size_t)h[4], R = (size_t)h[5];
    std::vector<int32_t> tx_tid, tx_start, tx_end, ex_start, ex_end, sj[5], r_tid, r_pos;
    std::vector<uint8_t> tx_rev, reach; std::vector<int64_t> tx_ex_off;
    bool ok = true;
    if (has_anno) ok = get(f, tx_tid, T) && get(f, tx_start, T) && get(f, tx_end, T) && get(f, tx_rev, T) && get(f, tx_ex_off, T + 1) && get(f, ex_start, X) && get(f, ex_end, X);
    if (has_sj) for (int k = 0; k < 5; ++k) ok = ok && get(f, sj[k], S);
    ok = ok && get(f, r_tid, R) && get(f, r_pos, R) && get(f, reach, R);
    if (!ok) { fprintf(stderr, "tables_dump: short case file\n"); return 2; }
    fclose(f);

    l2r_annotation a;
    memset(&a, 0, sizeof a);
    a.n_tx = (int64_t)T; a.n_exon = (int64_t)X;
    a.tx_tid = tx_tid.data(); a.tx_start = tx_start.data(); a.tx_end = tx_end.data(); a.tx_rev = tx_rev.data(); a.tx_ex_off = tx_ex_off.data();
    a.ex_start = ex_start.data(); a.ex_end = ex_end.data();
    l2r_junctions s;
    memset(&s, 0, sizeof s);
    s.n = (int64_t)S; s.tid = sj[0].data(); s.don = sj[1].data(); s.acc = sj[2].data(); s.uniq_c = sj[3].data(); s.multi_c = sj[4].data();

    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 2; }
    AnnoTables t;
    SjTables j;
    std::string msg;
    const int state = has_anno ? anno_tables(&a, argc == 4 ? argv[3] : "", t, msg) : 0;
    const int rc = state < 0 ? -1 : has_sj && S ? build_sj_tables(&s, j, msg) : 0;       // (l2r_set_junctions: an empty table is no table)
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    if (has_anno) {
        if (argc == 4) put_i64("state", state);
        put_vec("hdr", "<i4", t.hdr, 12); put_vec("key", "<i8", t.key); put_vec("key_raw", "<i8", t.key_raw); put_vec("ex", "<i4", t.ex, 2);
        put_vec("st_ent", "<u4", t.st_ent, 8); put_vec("en_ent", "<u4", t.en_ent, 8);       // (SiteEnt: k1, k2, tx_base are signed)
        put_vec("st_dir", "<u4", t.st_dir); put_vec("st_rdir", "<u4", t.st_rdir); put_vec("en_dir", "<u4", t.en_dir);
        put_vec("tid_base", "<i4", t.tid_base); put_vec("kb_base", "<i4", t.kb_base); put_vec("key_dir", "<u4", t.key_dir);
        put_i64("n_wide", t.n_wide); put_i64("n_compact", t.n_compact); put_i64("n_tid_dir", t.n_tid_dir); put_i64("n_tid_key", t.n_tid_key);
        if (R) put_cursors("anno_after", "anno_replay", "anno_replay_end", t.key, t.key_raw, h[6], r_tid, r_pos, nullptr);
    }
    if (has_sj) {
        put_vec("sj_key", "<i8", j.key); put_vec("sj_key_raw", "<i8", j.key_raw);
        put_vec("sj_cbase", "<i4", j.cbase); put_vec("sj_cdir", "<u4", j.cdir); put_vec("sj_dbase", "<i4", j.dbase); put_vec("sj_ddir", "<u4", j.ddir);
        put_vec("sj_row", "<i4", j.row, 4); put_i64("sj_ntid", j.n_tid);
        if (R) put_cursors("sj_after", "sj_replay", "sj_replay_end", j.key, j.key_raw, h[7], r_tid, r_pos, reach.data());
    }
    return fclose(g_out) ? 2 : 0;
}
