// l2r_plan.hip.h -- the plan of an upload: everything l2r_upload_reads (l2r_engine.hip) decides about a read set on the host, from the
// caller's arrays alone.  How the records are cut into tiles is decided here and nowhere else, so every precondition of the kernels
// that concerns a tile starts here: TILE_POS_CAP, SLAB_TILE_SPAN, SLAB_ROWS, SLOT_LOC_LIMIT, "never exact" for reads of 255 exons or more.
// Host arithmetic only: no HIP call, no kernel launch, no context, no environment.  The engine stages what the plan holds; a
// stand-alone program (tests/plan_dump.hip) writes it out for tests/test_upload_plan_cpu.py, which compares it with a restatement.
// Included behind the kernel headers (their constants, TileRec, TileStat).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lr2rmats_hip.h"

namespace l2r {

// The facts of the context a plan depends on
struct PlanOpts {
    int32_t min_intron = 3, max_delet = 50;     // l2r_params: the exon sample counts the operations that cut under them
    bool want_slab = true;                      // a slab layout is wanted (the pipeline asked for is not the classic one)
    bool want_index = true;                     // a tile index is wanted where the CIGARs are short (the tile path, and more than ONE run will follow)
    bool stream_sorted = true;                  // the uploads of this input so far were in coordinate order (l2r_ctx::Stream)
    int64_t last_key = INT64_MIN;               // ... and the key of their last record
};

struct UploadPlan {
    // ---- plan_check_reads
    bool sorted_here = true;                    // this upload's records are in coordinate order among themselves
    // ---- plan_tiles
    bool sorted = true;                         // ... and so is everything uploaded so far with them
    int64_t last_key = INT64_MIN;               // key of the last record (unchanged by an empty upload)
    bool wide_cigar = false, many_exon_reads = false;
    double est = 1.0;                           // exons per read, from the sample
    bool slab_tiles = false, slab_long = false, slab_layout = false, make_index = false;
    int reads_per_tile = TILE_THREADS;
    std::vector<uint32_t> tile_first;           // first read of every tile, and the closing entries
    int64_t n_tiles = 0, n_tiles256 = 0;
    // ---- plan_slab: the slab part
    bool slab_ok = false;
    std::vector<uint32_t> sbase;                // n_tiles + 1
    uint64_t slab_total = 0, dense_rows = 0;    // elements of the slabs, rows of the dense area
    std::vector<TileRec> rec;
    std::vector<uint32_t> off32;
    // ---- plan_slab: the summary-index part
    bool have_index = false;                    // k_tile_index runs
    std::vector<uint16_t> nn;                   // with summaries: the records' N operations
    std::vector<TileStat> tile_stat;            // n_tiles; from the summaries where there are any, else as k_tile_index finds them empty
};

static int plan_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

// (tid, pos) of a record as one key: sortedness across uploads.  (Not the engine's host_key, which leaves room for tid -1.)
static inline int64_t plan_read_key(int32_t tid, int32_t pos) { return ((int64_t)tid << 32) | (uint32_t)pos; }

// ---- the records are what the kernels may assume, and are they in coordinate order
static int plan_check_reads(const l2r_reads &r, UploadPlan &pl, std::string &msg)
{
    const int64_t N = r.n_reads;
    if (N && (r.cig_off[0] != 0 || r.cig_off[N] != r.n_cigar)) return plan_fail(msg, "[l2r_upload_reads] cig_off does not span n_cigar");
    bool sorted = true;
    for (int64_t i = 0; i < N; ++i) {
        if (r.tid[i] < 0) return plan_fail(msg, "[l2r_upload_reads] record %lld has no reference (unmapped); the reference aborts on it (bam2gtf.c:100)", (long long)i);
        if (r.cig_off[i + 1] < r.cig_off[i]) return plan_fail(msg, "[l2r_upload_reads] cig_off not monotone at %lld", (long long)i);
        if (i && (r.tid[i] < r.tid[i - 1] || (r.tid[i] == r.tid[i - 1] && r.pos[i] < r.pos[i - 1]))) sorted = false;
    }
    pl.sorted_here = sorted;
    return 0;
}

// ---- an upload that continues others (l2r_ctx::Stream): sorted only if everything so far was, and it begins where they ended
static void plan_continuation(const l2r_reads &r, const PlanOpts &o, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    pl.sorted = o.stream_sorted;
    if (N && o.stream_sorted) {
        const int64_t first = plan_read_key(r.tid[0], r.pos[0]);
        if (!pl.sorted_here || first < o.last_key) pl.sorted = false;            // from here on the cursors depend on the history
    }
    pl.last_key = N ? plan_read_key(r.tid[N - 1], r.pos[N - 1]) : o.last_key;
}

// ---- the exon sample
static void plan_exon_sample(const l2r_reads &r, const PlanOpts &o, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    pl.wide_cigar = N > 0 && (double)r.n_cigar / (double)N > 32.0;
    // tile size: keep the expected exons of a tile inside the LDS staging area.
    // Estimate exons/read from a sample of the CIGARs (ops that can start an exon).
    pl.many_exon_reads = false;
    pl.est = 1.0;
    if (N) {
        const int64_t sample = N < 4096 ? N : 4096;
        const int64_t step = N / sample;
        double cuts = 0;
        int64_t many = 0;                                  // sampled reads with more exons than a slab has rows
        for (int64_t s = 0; s < sample; ++s) {
            const int64_t i = s * step;
            int64_t mine = 0;
            for (int64_t k = r.cig_off[i]; k < r.cig_off[i + 1]; ++k) {
                const uint32_t op = r.cig[k] & 15u; const int len = (int)(r.cig[k] >> 4);
                mine += (op == 3u && len >= o.min_intron) || (op == 2u && len > o.max_delet);
            }
            cuts += (double)mine; many += mine + 1 > (int64_t)SLAB_ROWS;
        }
        // (k_walk_slab_long hands a read beyond SLAB_ROWS exons to the generic kernel, the classic kernels keep it on the mask path: an
        //  input where such reads are more than a rarity stays with them)
        pl.many_exon_reads = many * 200 > sample;
        pl.est = cuts / (double)sample + 1.0;
    }
}

// ---- which layouts the upload gets
static void plan_layouts(const PlanOpts &o, UploadPlan &pl)
{
    // What this upload's layout allows, decided once: the slab pipeline takes coordinate-sorted records; with long CIGARs
    // (k_walk_slab_long) only where reads beyond SLAB_ROWS exons are a rarity.  Its tiles are cut by span and get the slab layout.
    const bool slab_wanted = o.want_slab && pl.sorted;
    pl.slab_tiles = slab_wanted && !pl.wide_cigar;                               // short CIGARs (k_walk_slab)
    pl.slab_long = slab_wanted && pl.wide_cigar && !pl.many_exon_reads;          // long CIGARs (k_walk_slab_long)
    pl.slab_layout = pl.slab_tiles || pl.slab_long;                              // -> slab_ok
    // ... and the tile index (k_tile_index) that the one-kernel tile path needs: not for an upload that ONE run follows (l2r_classify)
    pl.make_index = o.want_index && !pl.wide_cigar;
}

// ---- reads per tile
static void plan_reads_per_tile(const l2r_reads &r, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    int rpt = TILE_THREADS;
    // (long CIGARs on the slab pipeline: the probe kernels stage SLAB_POS_CAP positions per tile)
    if (N) while (rpt > 32 && pl.est * rpt * 1.25 > (double)(pl.slab_long ? SLAB_POS_CAP : LDS_EXON_CAP)) rpt >>= 1;
    // ... and keep the genomic span of a tile inside the staged bucket directory (DIR_CAP buckets of 512 bp):
    // sparse input (few reads per locus) makes 256 consecutive reads span many genes, and a tile that does not
    // fit goes to the generic kernel read by read (~30x the cost).  Sample windows of the sorted input, take for
    // every candidate size the share of windows that would not fit, and pick the cheapest size.
    // (The slab pipeline's tiles are cut by span one by one, below: a sparse stretch makes ITS tiles small, not every tile of the
    //  upload -- an annotation with a few isoform-rich loci and long sparse stretches got 128-read tiles throughout, twice the tiles.)
    if (pl.sorted && N >= 2 * TILE_THREADS && !pl.slab_layout) {
        const int64_t n_win = std::min<int64_t>(N / TILE_THREADS, 384);
        const int64_t wstep = (N / TILE_THREADS) / n_win;
        const int64_t limit = (int64_t)(DIR_CAP - 8) << SITE_SHIFT;
        int64_t bad[4] = {0, 0, 0, 0};                 // sizes 256, 128, 64, 32
        for (int64_t w = 0; w < n_win; ++w) {
            const int64_t i0 = w * wstep * TILE_THREADS;
            int64_t hi = 0;
            int size_idx = 3, next_mark = 32;
            for (int64_t q = 0; q < TILE_THREADS && i0 + q < N; ++q) {
                const int64_t i = i0 + q;
                if (r.tid[i] != r.tid[i0]) break;
                int64_t end = r.pos[i];
                for (int64_t k = r.cig_off[i]; k < r.cig_off[i + 1]; ++k) if ((0x18du >> (r.cig[k] & 15u)) & 1u) end += r.cig[k] >> 4;
                hi = std::max(hi, end - r.pos[i0]);
                if (q + 1 == next_mark) {              // the first 32 / 64 / 128 / 256 reads of the window
                    if (hi > limit) { for (int z = 0; z <= size_idx; ++z) bad[z]++; break; }   // this size and every larger one
                    --size_idx; next_mark <<= 1;
                }
            }
        }
        double best = 1e300; int best_rpt = rpt;
        for (int z = 0; z < 4; ++z) {
            const int cand = TILE_THREADS >> z;
            if (cand > rpt) continue;
            const double f = (double)bad[z] / (double)n_win;
            const double cost = (1.0 - f) * (z == 0 ? 1.0 : z == 1 ? 1.6 : z == 2 ? 2.6 : 4.5) + 30.0 * f;
            if (cost < best - 1e-9) { best = cost; best_rpt = cand; }
        }
        rpt = best_rpt;
    }
    pl.reads_per_tile = rpt;
}

// ---- the tile cut
static void plan_tile_cut(const l2r_reads &r, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    const int rpt = pl.reads_per_tile;
    const bool sorted = pl.sorted;
    // Tiles: runs of up to rpt consecutive reads; for sorted input a tile also ends where the chromosome changes, so
    // that every read of a tile can use the tile's dictionary slices (unsorted input: plain runs, the reads that are
    // not on the chromosome of their tile's first read take the generic kernel).
    std::vector<uint32_t> &tile_first = pl.tile_first;
    tile_first.clear();
    tile_first.reserve((size_t)(N / rpt + 64));
    // (slab pipeline: a tile's exons are staged by position in LDS on their way out, l2r_slab.hip.h SLAB_POS_CAP: a tile also ends
    //  where the exon bounds of its reads -- from the CIGAR lengths -- would exceed that, so no read of it is left outside)
    uint64_t pos_sum = 0;
    for (int64_t i = 0, start = 0; i <= N; ++i) {
        if (i == N) { if (i > start) tile_first.push_back((uint32_t)start); break; }
        const uint64_t need = pl.slab_tiles ? (uint64_t)slab_rows_of((uint32_t)std::min<int64_t>(r.cig_off[i + 1] - r.cig_off[i], 0x7ffffff0)) : 0u;
        // (tiles of sorted records also end where the reads would begin 2^17 bases apart: a slab tile's exons are kept relative to its
        //  first base, and any tile's dictionary slices cover 196 kb -- sparse stretches give small tiles instead of tiles for the
        //  generic kernel; the classic pipeline, whose tiles own 24 KB of hand-over buffer each, keeps at least 8 reads per tile)
        if (i - start == rpt || (sorted && r.tid[i] != r.tid[start]) || (i > start && pos_sum + need > (uint64_t)TILE_POS_CAP) ||
            (sorted && i > start && (int64_t)r.pos[i] - (int64_t)r.pos[start] >= (int64_t)SLAB_TILE_SPAN && (pl.slab_layout || i - start >= 8))) { tile_first.push_back((uint32_t)start); start = i; pos_sum = 0; }
        pos_sum += need;
    }
    pl.n_tiles = (int64_t)tile_first.size();
    tile_first.push_back((uint32_t)N);
    if (tile_first.size() < 2) tile_first.push_back((uint32_t)N);        // (an empty launch still runs one workgroup)
    pl.n_tiles256 = (N + TILE_THREADS - 1) / TILE_THREADS;
}

// ---- the slab layout
// exb: exons the upload's result arrays have room for -- with long CIGARs the engine has counted the operations that can cut on the device
static void plan_slab_layout(const l2r_reads &r, size_t exb, UploadPlan &pl)
{
    // the slab layout (l2r_slab.hip.h): per tile as many rows of 256 elements as its longest read can have exons (bound from
    // the CIGAR lengths); reads beyond SLAB_ROWS rows are outliers and get a run of the dense area
    const size_t T = (size_t)pl.n_tiles;
    const std::vector<uint32_t> &tile_first = pl.tile_first;
    std::vector<uint32_t> &sbase = pl.sbase;
    sbase.assign(T + 1, 0u);
    uint64_t total = 0, ovf = 0;
    for (size_t t = 0; t < T; ++t) {
        uint32_t m = 1;
        if (pl.wide_cigar) {
            // long CIGARs (k_walk_slab_long): the CIGAR length says nothing about the exons -- every tile has SLAB_ROWS rows, and
            // the dense area has room for every exon of the shard (exb: reads + the operations that can cut)
            m = (uint32_t)SLAB_ROWS;
        } else
        for (uint32_t i = tile_first[t]; i < tile_first[t + 1]; ++i) {
            const uint64_t cc = (uint64_t)(r.cig_off[i + 1] - r.cig_off[i]);
            const uint64_t rw = (cc + 3u) >> 1;
            // (room in the dense area for EVERY read: besides the long CIGARs a read with an exon of 64 kb or more ends up
            //  there, which only the walk finds out)
            ovf += cc + 1;
            if (rw <= (uint64_t)SLAB_ROWS) m = std::max<uint32_t>(m, (uint32_t)rw);
        }
        sbase[t] = (uint32_t)total; total += (uint64_t)m * SLAB_STRIDE;
        if (total >= 0x7ffffff0ULL || ovf >= 0x7ffffff0ULL) break;
    }
    if (pl.wide_cigar) ovf = (uint64_t)exb;
    pl.slab_total = total; pl.dense_rows = ovf;
    pl.slab_ok = total < 0x7ffffff0ULL && ovf < 0x7ffffff0ULL;
    if (pl.slab_ok) sbase[T] = (uint32_t)total;                     // (rows of tile t = (sbase[t + 1] - sbase[t]) / 256)
}

// ---- the tiles' records and the 32-bit CIGAR offsets
static void plan_tile_recs(const l2r_reads &r, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    const size_t T = (size_t)pl.n_tiles;
    // the tiles' records for k_walk_slab (TileRec: reads, slab, chromosome and first base of the tile in one place) and the
    // records' CIGAR offsets in 32 bits (the walk reads 4 bytes per record instead of 8 at a stride of 8)
    pl.rec.assign(T ? T : 1, TileRec{});
    for (size_t t = 0; t < T; ++t) {
        TileRec &q = pl.rec[t];
        q.r0 = pl.tile_first[t]; q.n_act = pl.tile_first[t + 1] - pl.tile_first[t]; q.sbase = pl.sbase[t]; q.rows = (pl.sbase[t + 1] - pl.sbase[t]) >> 8;
        q.tid0 = q.n_act ? r.tid[q.r0] : 0; q.lo = (q.n_act ? r.pos[q.r0] : 0) + 1; q.pad[0] = q.pad[1] = 0u;
    }
    pl.off32.resize((size_t)N + 1);
    for (int64_t i = 0; i <= N; ++i) pl.off32[(size_t)i] = (uint32_t)r.cig_off[i];
}

// ---- the tile index from the reader's summaries
static void plan_summary_index(const l2r_reads &r, UploadPlan &pl)
{
    const int64_t N = r.n_reads;
    const size_t T = (size_t)pl.n_tiles;
    // every tile's last base (the largest read end: CIGAR lengths only, no parameter has a say) into its record: the one-kernel
    // tile path makes the tiles' windows from it in front of the walk (l2r_tile.hip.h)
    // ... and an index of its CIGAR operations from which a run knows the tile's exon count unless a threshold is borderline in it
    pl.tile_stat.assign(T, TileStat{0, INT32_MAX, 0, INT32_MAX});
    pl.have_index = T && pl.make_index;
    pl.nn.clear();
    if (!pl.have_index || !r.cig_summary) return;
    // the reader's per-record summaries: the tiles' statistics and last bases on the host (no parameter has a say in them), the
    // records' N operations as one 16-bit column for the kernel -- which then touches no CIGAR
    pl.nn.resize((size_t)N);
    for (size_t t = 0; t < T; ++t) {
        TileStat st{0, INT32_MAX, 0, INT32_MAX};
        int64_t hi = INT32_MIN; uint32_t tot_x = 0u; bool many = false;
        for (uint32_t i = pl.tile_first[t]; i < pl.tile_first[t + 1]; ++i) {
            const uint32_t *q = r.cig_summary + 3 * (size_t)i;
            const uint32_t n_n = q[1] & 0xffffu, mn = q[1] >> 16, md = q[2] & 0xffffu, ms = q[2] >> 16;
            pl.nn[i] = (uint16_t)n_n;
            st.n_ops_n += (int32_t)n_n; st.min_n = std::min(st.min_n, (int32_t)mn); st.min_seg = std::min(st.min_seg, (int32_t)ms);
            st.max_d = std::max(st.max_d, md == 0xffffu ? INT32_MAX : (int32_t)md);      // (65535: that long or longer)
            hi = std::max<int64_t>(hi, (int64_t)r.pos[i] + (int64_t)q[0]);
            tot_x += n_n + 1u; many = many || n_n + 1u >= 255u;
        }
        // (a read of 255 exons or more, places a slot record cannot say: never an exact tile -- as k_tile_index<false> rules)
        if (many || tot_x >= SLOT_LOC_LIMIT) st.min_seg = INT32_MIN;
        pl.tile_stat[t] = st;
        pl.rec[t].pad[0] = (uint32_t)std::min<int64_t>(std::max<int64_t>(hi, INT32_MIN), INT32_MAX);
    }
}

// ---- the index once more per super-block (l2r_slab.hip.h SlabArgs::sup_stat); stat: the tiles' statistics, from the plan or from k_tile_index
static std::vector<TileStat> plan_sup_stat(const UploadPlan &pl, const std::vector<TileStat> &stat)
{
    const size_t T = (size_t)pl.n_tiles;
    std::vector<TileStat> sup((T >> LB_SUP_SHIFT) + 1, TileStat{0, INT32_MAX, 0, INT32_MAX});
    for (size_t t = 0; t < T; ++t) {
        TileStat &q = sup[t >> LB_SUP_SHIFT]; const TileStat &st = stat[t];
        q.n_ops_n += st.n_ops_n + (int32_t)pl.rec[t].n_act; q.min_n = std::min(q.min_n, st.min_n); q.max_d = std::max(q.max_d, st.max_d); q.min_seg = std::min(q.min_seg, st.min_seg);
    }
    return sup;
}

// The plan in two parts, each a list of the steps above.  The records are checked (plan_check_reads) before either.
// ... the tiles: what the staging of the records and the sizes of the work buffers need
static void plan_tiles(const l2r_reads &r, const PlanOpts &o, UploadPlan &pl)
{
    plan_continuation(r, o, pl);
    plan_exon_sample(r, o, pl);
    plan_layouts(o, pl);
    plan_reads_per_tile(r, pl);
    plan_tile_cut(r, pl);
}
// ... the slab part and the summary-index part, where the upload gets the slab layout (exb: see plan_slab_layout)
static void plan_slab(const l2r_reads &r, size_t exb, UploadPlan &pl)
{
    pl.slab_ok = false;
    if (!pl.slab_layout) return;
    plan_slab_layout(r, exb, pl);
    if (!pl.slab_ok) return;
    plan_tile_recs(r, pl);
    plan_summary_index(r, pl);
}

}   // namespace l2r
