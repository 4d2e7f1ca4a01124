// plan_dump.hip -- the upload's plan (lr2rmats_amd/csrc/l2r_plan.hip.h) as a stand-alone host program, for tests/test_upload_plan_cpu.py:
//     plan_dump <case file> <output file>
// reads one case, builds the plan through the same steps as l2r_upload_reads, and writes every member of it.  No HIP function is
// called and no GPU is needed; `make -C lr2rmats_amd/csrc plan-dump` builds it with ASan + UBSan on the host code.
//
// Case file (little endian): 12 int64 -- n_reads, n_cigar, summaries present, min_intron, max_delet, want_slab, want_index,
// stream_sorted, last_key, exb (-1: n_cigar + n_reads, what the engine takes where the CIGARs are short), 0, 0 -- then tid[n_reads] and
// pos[n_reads] (int32), cig_off[n_reads + 1] (int64), cig[n_cigar] (uint32) and, if present, the summaries (3 uint32 per read).
// Output file: per member a 24-byte name, an 8-byte numpy type, the element count (int64) and the elements.  A case the plan
// rejects gives `rc` and `error` alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../lr2rmats_amd/csrc/l2r_kernels.hip.h"
#include "../lr2rmats_amd/csrc/l2r_window.hip.h"
#include "../lr2rmats_amd/csrc/l2r_slab.hip.h"
#include "../lr2rmats_amd/csrc/l2r_chunk.hip.h"
#include "../lr2rmats_amd/csrc/l2r_tchunk.hip.h"
#include "../lr2rmats_amd/csrc/l2r_plan.hip.h"

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
template <typename T> static void put_vec(const char *name, const char *type, const std::vector<T> &v, size_t per = 1)
{
    put(name, type, v.data(), sizeof(T) / per, (int64_t)(v.size() * per));
}

template <typename T> static bool get(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: plan_dump <case file> <output file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t h[12];
    if (fread(h, 8, 12, f) != 12 || h[0] < 0 || h[1] < 0) { fprintf(stderr, "plan_dump: bad header\n"); return 2; }
    const size_t N = (size_t)h[0], C = (size_t)h[1];
    std::vector<int32_t> tid, pos; std::vector<int64_t> cig_off; std::vector<uint32_t> cig, summ;
    if (!get(f, tid, N) || !get(f, pos, N) || !get(f, cig_off, N + 1) || !get(f, cig, C) || !get(f, summ, h[2] ? 3 * N : 0)) { fprintf(stderr, "plan_dump: short case file\n"); return 2; }
    fclose(f);

    l2r_reads r;
    memset(&r, 0, sizeof r);
    r.n_reads = (int64_t)N; r.n_cigar = (int64_t)C;
    r.tid = tid.data(); r.pos = pos.data(); r.cig_off = cig_off.data(); r.cig = cig.data();
    r.cig_summary = h[2] ? summ.data() : nullptr;
    PlanOpts o;
    o.min_intron = (int32_t)h[3]; o.max_delet = (int32_t)h[4]; o.want_slab = h[5] != 0; o.want_index = h[6] != 0;
    o.stream_sorted = h[7] != 0; o.last_key = h[8];

    g_out = fopen(argv[2], "wb");
    if (!g_out) { perror(argv[2]); return 2; }
    UploadPlan pl;
    std::string msg;
    const int rc = plan_check_reads(r, pl, msg);
    put_i64("rc", rc);
    if (rc) {
        put("error", "|u1", msg.data(), 1, (int64_t)msg.size());
        return fclose(g_out) ? 2 : 0;
    }
    plan_tiles(r, o, pl);
    const size_t exb = h[9] < 0 ? C + N : (size_t)h[9];
    plan_slab(r, exb, pl);

    put_i64("sorted_here", pl.sorted_here); put_i64("sorted", pl.sorted); put_i64("last_key", pl.last_key);
    put_i64("wide_cigar", pl.wide_cigar); put_i64("many_exon_reads", pl.many_exon_reads);
    put("est", "<f8", &pl.est, 8, 1);
    put_i64("slab_tiles", pl.slab_tiles); put_i64("slab_long", pl.slab_long); put_i64("slab_layout", pl.slab_layout); put_i64("make_index", pl.make_index);
    put_i64("reads_per_tile", pl.reads_per_tile);
    put_vec("tile_first", "<u4", pl.tile_first);
    put_i64("n_tiles", pl.n_tiles); put_i64("n_tiles256", pl.n_tiles256);
    put_i64("slab_ok", pl.slab_ok);
    if (pl.slab_ok) {
        put_vec("sbase", "<u4", pl.sbase);
        put_i64("slab_total", (int64_t)pl.slab_total); put_i64("dense_rows", (int64_t)pl.dense_rows);
        put_vec("rec", "<i4", pl.rec, 8);                   // (TileRec: eight words; tid0, lo and the last base in pad[0] are signed)
        put_vec("off32", "<u4", pl.off32);
        put_i64("have_index", pl.have_index);
        put_vec("nn", "<u2", pl.nn);
        put_vec("tile_stat", "<i4", pl.tile_stat, 4);
        put_vec("sup_stat", "<i4", plan_sup_stat(pl, pl.tile_stat), 4);
    }
    return fclose(g_out) ? 2 : 0;
}
