// l2r_engine.hip -- C-ABI implementation (include/lr2rmats_hip.h) over the gfx950
// kernels of l2r_kernels.hip.h.  One context = one GPU = one HIP stream.
// There is deliberately no CPU path in this file: every entry point that does
// work needs a HIP device and fails with a message otherwise.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/lr2rmats_hip.h"
#include "l2r_kernels.hip.h"
#include "l2r_window.hip.h"
#include "l2r_slab.hip.h"
#include "l2r_chunk.hip.h"
#include "l2r_tchunk.hip.h"
#include "l2r_filter.hip.h"
#include "l2r_fusion.hip.h"
#include "l2r_sj.hip.h"
#include "l2r_sort.hip.h"
#include "l2r_names.hip.h"
#include "l2r_gtf.hip.h"
#include "l2r_bed.hip.h"
#include "l2r_uniq.hip.h"
#include "l2r_gtftext.hip.h"
#include "l2r_readlist.hip.h"
#include "l2r_detail.hip.h"
#include "l2r_summary.hip.h"
#include "l2r_novel.hip.h"
#include "l2r_plan.hip.h"
#include "l2r_tables.hip.h"
#include "l2r_nameorder.hip.h"
#include "l2r_gtforder.hip.h"
#include "l2r_bedplan.hip.h"
#include "l2r_gtftextplan.hip.h"
#include "l2r_readlistplan.hip.h"
#include "l2r_detailplan.hip.h"

using namespace l2r;

static thread_local char g_err[1024] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY_AS(who, expr)                                                                           \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(-2, "[%s] %s: %s", who, #expr, hipGetErrorString(e_));        \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(__func__, expr)        // (HIP_TRY_AS: in a helper, under the entry point's name)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;     // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n)
    {
        if (n <= cap && p) return 0;
        // (contents are never carried over: every user refills the buffer.)  The old buffer is released first -- at 288 GB
        // shards both would not always fit -- so a failed grow leaves an EMPTY buffer (p = null, cap = 0), never a stale one.
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const size_t want = n ? n : 1;
        T *q = nullptr;
        const hipError_t e = hipMalloc((void **)&q, want * sizeof(T));
        if (e != hipSuccess) return fail(-2, "hipMalloc(%zu bytes): %s", want * sizeof(T), hipGetErrorString(e));
        p = q; cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Two events around a piece of device work whose time is wanted (hipEventElapsedTime(a, b)), destroyed with the scope
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// The stage timer of a table command (`filter` / `fusion`, `bam2sj` / `sjtab`, `sort`, `sort -n`, `sort-gtf`): its launches go through
// launch().  on (L2R_FUSION_TIMING=1, L2R_SJ_TIMING=1, L2R_SORT_TIMING=1): a launch is bracketed by the two events and waited for, its
// device milliseconds are ADDED to *ms -- the caller zeroes its words.  wait: a launch is waited for in any case (the sort paths under
// L2R_CHECK).  A command arms its timer with begin() before its first launch.
struct StageTimer {
    bool on = false, wait = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    StageTimer() = default;
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() { for (int k = 0; k < 2; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]); }
    int begin(bool on_, bool wait_)
    {
        on = on_; wait = wait_;
        for (int k = 0; k < 2 && on; ++k) if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k]));
        return 0;
    }
    template <typename F> int launch(l2r_ctx *c, double *ms, F f);      // (behind l2r_ctx)
};

// The three kernel pipelines: classic (l2r_kernels.hip.h, two walks), slab (l2r_slab.hip.h, one walk, two kernels), tile (l2r_tile.hip.h,
// one kernel per tile).  The upload says which of them its layout allows, choose_pipeline which one a launch takes.
enum class Pipeline { classic, slab, tile };

// `bam2sj` (l2r_sj.hip.h): what lives between l2r_sj_begin and l2r_sj_download.  Every buffer belongs to the context and is used again
// by the next batch; the two row buffers take turns as source and target of the radix passes and of the reduction.
struct SjRowBuf {
    DevBuf<int32_t> col[6];                 // col[5], the overhang: only in a table begun with l2r_sj_begin_tab
    size_t cap = 0;
    SjCols cols() const { return SjCols{col[0].p, col[1].p, col[2].p, col[3].p, col[4].p, col[5].p}; }
};
struct SjState {
    bool open = false, finished = false;
    bool over = false;                      // l2r_sj_begin_tab: six columns, the OVER instances of fill / scatter / reduce
    SjPrm prm{3, 1};
    int32_t n_seq = 0;
    DevBuf<int64_t> seq_off; DevBuf<uint8_t> bases;
    SjRowBuf rows[2]; int cur = 0;
    int64_t n_rows = 0;                     // rows[cur] holds that many
    int64_t compact_rows = (int64_t)1 << 24, compact_at = (int64_t)1 << 24;     // L2R_SJ_COMPACT_ROWS: rows beyond which an add sorts and reduces what is there
    DevBuf<uint16_t> flag; DevBuf<int32_t> tid, pos; DevBuf<uint8_t> uniq; DevBuf<int64_t> cig_off; DevBuf<uint32_t> cig, cnt;   // one batch
    DevBuf<uint32_t> hist12, tile_hist, head, word;     // word[0]: a scan's total, word[1]: k_sj_motif's bad row, word[2]: k_sj_introns' row count, word[3]: rows the intron-size rule dropped
    DevBuf<uint8_t> strand[2], motif[2], anno[2]; int bcur = 0;      // per-row bytes; the filter moves them to the other set
    DevBuf<int32_t> near_acc;               // l2r_sj_filter_rows2: per row the distance to the nearest other acceptor
    double stats[32] = {0};
    StageTimer clk;
};
// the annotation of l2r_sj_annotate on the device, and its introns: a table of their own (five columns), sorted and made unique by sj_compact
struct SjIntrons {
    DevBuf<int32_t> tx_tid, ex_start, ex_end; DevBuf<int64_t> tx_ex_off;
    SjState st;
};

// `sort`, `filter -S` (l2r_sort.hip.h): the buffers of l2r_sort_order.  They belong to the context, grow on demand and are used again by
// the next call; the two key / index columns take turns as source and target of the radix passes.
struct SortState {
    DevBuf<uint16_t> flag; DevBuf<int32_t> tid, pos;
    DevBuf<uint64_t> key[2]; DevBuf<uint32_t> idx[2];
    DevBuf<uint32_t> hist, tile_hist, word;             // hist: 8 x 256 and, behind them, the descent flag; word[0]: a scan's total
    StageTimer clk;
    double stats[7] = {0};                              // l2r_sort_stats
};

// `sort -n`, `filter -N`, `fusion -N` (l2r_names.hip.h): the buffers of l2r_name_order beside those of SortState, which hold the hashes
// and the index column of the passes.  They belong to the context, grow on demand and are used again by the next call.
struct NameState {
    DevBuf<uint64_t> blob, hkey;                        // the name bytes as aligned words; the hashes in record order
    DevBuf<int64_t> off;
    DevBuf<uint32_t> head, head_pos, first_idx, sizes, order;
    DevBuf<uint32_t> word;                              // word[0]: groups (the first scan's total), [1]: mismatching pairs, [2]: a record moved, [3]: the second scan's total
    StageTimer clk;
    double stats[11] = {0};                             // l2r_name_stats
};

// `sort-gtf` (l2r_gtf.hip.h): the buffers of l2r_gtf_order beside those of SortState, which hold the keys and the index columns of its
// two radix stages, and the rows of the last call on the host (l2r_gtf_rows_out).  They belong to the context, grow on demand and are
// used again by the next call.
struct GtfState {
    DevBuf<uint4> text;                                 // the text, 16-byte aligned, GTF_TEXT_ROOM zeroed bytes behind it
    DevBuf<uint32_t> tile_cnt, start;                   // newlines per tile (scanned in place); line starts
    DevBuf<uint32_t> kept, tx, l_name_off, l_name_len, l_s, l_e;      // per line
    DevBuf<uint32_t> r_start, r_len, r_line, r_tx;      // per kept line
    DevBuf<uint32_t> t_name_off, t_name_len, t_s, t_e, head;          // per transcript line
    DevBuf<uint32_t> h_off, h_len, rank;                // per head
    DevBuf<uint32_t> c, s, e, order1, order;            // per kept line: the triple, stage 1's order, the order
    DevBuf<uint32_t> word;                              // GTFW_*
    std::vector<uint64_t> res_start; std::vector<uint32_t> res_len, res_line;        // the rows of the last call, in the order
    StageTimer clk;
    double stats[17] = {0};                             // l2r_gtf_stats
};

// The reference-name table of a text command (l2r_bed_begin, l2r_gtftext_begin): a copy on the host, which the command's parameters are
// re-pointed at and its host route reads, and one on the device
struct RefNames {
    std::vector<int64_t> h_off; std::vector<uint8_t> h_names;
    DevBuf<int64_t> off; DevBuf<uint8_t> names;
    void set(int32_t n_ref, const int64_t *ref_off, const uint8_t *ref_names)
    {
        const size_t R = (size_t)n_ref, NB = R ? (size_t)ref_off[R] : 0;
        h_off.assign(R + 1, 0);
        for (size_t k = 0; k <= R && R; ++k) h_off[k] = ref_off[k];
        h_names.assign(NB + 1, 0);
        if (NB) memcpy(h_names.data(), ref_names, NB);
    }
    int upload(l2r_ctx *c);                             // (behind l2r_ctx) queued on the context stream
};

// The annotation's gene tables of a per-read text command (l2r_detail_begin, l2r_gtftext_anno), in the manner of RefNames; one element of
// padding behind each, so that no vector is empty.  Each command keeps its own: the two may be given different tables.
struct GeneTables {
    std::vector<uint8_t> h_names; std::vector<uint32_t> h_gid, h_gname;
    DevBuf<uint8_t> names; DevBuf<uint32_t> gid, gname;
    void set(int64_t n_tx, int64_t names_len, const uint8_t *anno_names, const uint32_t *tx_gid, const uint32_t *tx_gname)
    {
        const size_t T = (size_t)n_tx, A = (size_t)names_len;
        h_names.assign(A + 1, 0);
        if (A) memcpy(h_names.data(), anno_names, A);
        h_gid.assign(T + 1, 0); h_gname.assign(T + 1, 0);
        if (T) { memcpy(h_gid.data(), tx_gid, T * 4); memcpy(h_gname.data(), tx_gname, T * 4); }
    }
    int upload(l2r_ctx *c);                             // (behind l2r_ctx) queued on the context stream
};

// The reads of a shard and their results as l2r_detail_rows and l2r_gtftext_reads keep them (take_reads): on the device or, the host route
// alone, on the host.  run_res: they came with res == NULL, the results are those of the context's last l2r_run in HBM (result_cols).
struct ReadRows {
    bool run_res = false;
    int64_t n = 0, names_len = 0; double exons_per_read = 0;
    DevBuf<int32_t> tid, xs, xe, ref_tx; DevBuf<uint8_t> names, f; DevBuf<uint32_t> qname, tid_name, ex_off, info;
    const uint32_t *tid_name_p = nullptr;               // qname's buffer where no tid_name came
    struct Host {                                       // the host route's copies; tid_name is empty where none came (tid_name_or_qname)
        std::vector<int32_t> tid, xs, xe, ref_tx; std::vector<uint8_t> names, f; std::vector<uint32_t> qname, tid_name, info; std::vector<int64_t> ex_off;
        l2r_result res{};                               // points into the vectors
        const uint32_t *tid_name_or_qname() const { return tid_name.empty() ? qname.data() : tid_name.data(); }
    } h;
    std::vector<uint32_t> off32;                        // ex_off narrowed for the upload; it lives until the stream has been waited for
};

// The text a command has produced (l2r_bed_lines, l2r_gtftext_lines), in HBM or on the host where the host route made it, until text_out
// fetches it.  TEXT_SLACK bytes lie behind the text in HBM; under L2R_CHECK they hold a pattern that the write kernel must leave alone.
constexpr size_t TEXT_SLACK = 64;
constexpr uint8_t TEXT_GUARD_BYTE = 0xa5;
struct TextOut {
    DevBuf<uint4> text;                                 // 16-byte aligned (text_stream_out of l2r_text.hip.h relies on it)
    std::vector<uint8_t> host_text;
    bool have = false, on_host = false;
    int64_t n_bytes = 0;
    uint8_t guard[TEXT_SLACK];                          // fetch_guard's copy
    void reset() { have = false; on_host = false; n_bytes = 0; host_text.clear(); }
    int reserve(size_t B) { return text.ensure((B + TEXT_SLACK + 15) / 16); }
    uint8_t *bytes() const { return reinterpret_cast<uint8_t *>(text.p); }
    void take_host() { have = true; on_host = true; n_bytes = (int64_t)host_text.size(); }
    void take_device(size_t B) { have = true; n_bytes = (int64_t)B; }
    // (behind l2r_ctx) the guard behind B bytes of text: filled in front of the write kernel, fetched behind it -- queued on the context
    // stream -- and compared once the stream has been waited for.  Without L2R_CHECK none of them touches the device.
    hipError_t arm_guard(const l2r_ctx *c, size_t B);
    hipError_t fetch_guard(const l2r_ctx *c, size_t B);
    bool guard_intact(const l2r_ctx *c) const;
};

// `bam2bed` (l2r_bed.hip.h): the reference names and the colour of l2r_bed_begin, the columns of one batch, what k_bed_measure leaves per
// record, and the text of the last l2r_bed_lines (in HBM, or on the host where the host route made it) until l2r_bed_text_out fetches it.
// The buffers belong to the context, grow on demand and are used again by the next batch.
struct BedState {
    bool begun = false;
    l2r_bed_params prm{};                               // ref_off / ref_names point into ref's vectors
    RefNames ref;
    DevBuf<uint16_t> flag; DevBuf<int32_t> tid, pos; DevBuf<uint8_t> mapq, names; DevBuf<int64_t> cig_off, name_off; DevBuf<uint32_t> cig;      // one batch
    DevBuf<uint32_t> off, n_blocks, span, size_len;     // per record; off: the line lengths, scanned in place (n + 1 words)
    DevBuf<uint32_t> word;                              // BEDW_*
    TextOut out;
    StageTimer clk;
    double stats[11] = {0};                             // l2r_bed_stats
};

// `unique-gtf` (l2r_uniq.hip.h): the columns of the last l2r_uniq_merge, what its kernels leave, and its results -- in HBM, or in `host` where
// uniq_host made them -- until l2r_uniq_out fetches them.  The buffers belong to the context and grow on demand.
struct UniqState {
    DevBuf<int32_t> tid, xs, xe; DevBuf<uint8_t> rev; DevBuf<int64_t> ex_off;      // the input
    DevBuf<UniqRec> rec; DevBuf<uint64_t> tile_max;
    DevBuf<uint32_t> head, first, len, word;            // head: flags, scanned in place (n + 1); len: list lengths, scanned in place; word: UQW_*
    DevBuf<int32_t> l_src, l_start, l_end, l_cov;       // the clusters' lists
    DevBuf<int32_t> uniq_of, u_src, u_start, u_end, u_cov; DevBuf<uint8_t> merged;
    bool have = false, on_host = false;
    int64_t n = 0, n_unique = 0;
    UniqResult host;
    StageTimer clk;
    double stats[UQS_N] = {0};                          // l2r_uniq_stats
};

// A device column that is appended to: reserve() keeps the n elements it holds (a copy on the context stream into a larger buffer, which
// is waited for before the old one is released) and, where the larger buffer cannot be had, leaves the column as it was.
template <typename T>
struct AccBuf {
    T *p = nullptr;
    size_t cap = 0, n = 0;
    AccBuf() = default;
    AccBuf(const AccBuf &) = delete;
    AccBuf &operator=(const AccBuf &) = delete;
    ~AccBuf() { if (p) (void)hipFree(p); }
    void clear() { n = 0; }
    int reserve(hipStream_t stream, size_t want)
    {
        if (want <= cap) return 0;
        T *q = nullptr;
        size_t room = want > 2 * cap ? want : 2 * cap;
        hipError_t e = hipMalloc((void **)&q, room * sizeof(T));
        if (e != hipSuccess && room > want) { room = want; e = hipMalloc((void **)&q, room * sizeof(T)); }
        if (e != hipSuccess) return fail(-2, "hipMalloc(%zu bytes): %s", room * sizeof(T), hipGetErrorString(e));
        if (n) e = hipMemcpyAsync(q, p, n * sizeof(T), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(q); return fail(-2, "growing a column of %zu elements: %s", n, hipGetErrorString(e)); }
        if (p) (void)hipFree(p);
        p = q; cap = room;
        return 0;
    }
};

// The read classes and unique counts of `update-gtf -y` (l2r_summary.hip.h): the merge parameters of l2r_summary_begin, the reads of every
// l2r_summary_add since -- in HBM, or on the host where the route of the begin is the host's -- and what the kernels of l2r_summary_finish
// leave.  `u` holds the permuted columns and the work of the merge kernels: a UniqState of this unit's own, so that a l2r_uniq_merge on
// the same context keeps its results.
struct SummaryState {
    bool begun = false, on_host = false;
    UniqPrm p{0, 0, 0, 0.0f};
    int64_t n = 0, x = 0, adds = 0;                     // reads, exons, calls so far
    AccBuf<int32_t> tid, xs, xe; AccBuf<uint32_t> info;
    struct Host { std::vector<int32_t> tid, xs, xe; std::vector<uint32_t> info; } h;
    DevBuf<uint8_t> cls; DevBuf<uint32_t> src_off, tile_cnt, dst_off, src, word;      // src_off, dst_off: n + 1, scanned in place; tile_cnt: 4 tiles + 1; word: SUMW_*
    DevBuf<unsigned long long> bad;                     // the smallest read outside the domain << 4 | its kind
    UniqState u;
    double stats[SMS_N] = {0};                          // l2r_summary_stats
};

// The novel list of `update-gtf` (l2r_novel.hip.h): the parameters of l2r_novel_begin, what the selection of every l2r_novel_add since
// has appended -- in HBM, or in `h` where the route of the begin is the host's -- the work of an add and of l2r_novel_finish, and its
// results until the next begin: the entries and kept rows in HBM (the two gene lists on the host, where add_gene's last test is made), or
// all of them in `out` where novel_host made them.  `u` holds the work of the merge kernels, as in SummaryState.
struct NovelState {
    bool begun = false, on_host = false, finished = false, rows_on_host = false;
    UniqPrm p{0, 0, 0, 0.0f};
    NovelPrm np{0, 0, 0u, 0, 0};
    RefNames ref;
    std::vector<uint32_t> h_tx_gene; DevBuf<uint32_t> tx_gene;
    int64_t n = 0, x = 0, adds = 0, split = 0;          // reads, their exons, calls, split-route reads so far
    AccBuf<int32_t> o_tid, o_ref, o_read, xs, xe, k_tid; AccBuf<uint8_t> o_rev, f; AccBuf<uint32_t> o_nex, k_gene;
    NovelAcc h;
    DevBuf<int32_t> a_tid, a_ref, a_xs, a_xe; DevBuf<uint32_t> a_off, a_info, cnt_x, tile_cnt, aword; DevBuf<uint8_t> a_f, bits;     // one add; cnt_x: n + 1, tile_cnt: 2 tiles + 1, aword: NOVW_*
    std::vector<uint32_t> off32;
    DevBuf<unsigned long long> bad;                     // the smallest read outside the domain << 4 | its kind
    UniqState u;
    DevBuf<uint32_t> o_off, cnt, hi, ia, ib, icov, order1, order, head, first, grp, sum, fword; DevBuf<uint8_t> imeta;     // the finish; fword: NOVF_*
    DevBuf<int32_t> e_src, r_tid, r_a, r_b, r_score; DevBuf<uint8_t> r_meta;
    int64_t n_entries = 0, row0[NOV_LISTS + 1] = {0}, kept[NOV_LISTS] = {0};
    NovelOut out;
    DevBuf<uint32_t> len, off, tword; std::vector<uint32_t> h_len; TextOut text;    // the BED text
    double tstats[12] = {0};                            // text_batch's slots
    bool has_gtf = false, gtf_ready = false; int last_which = L2R_NOVEL_BED;       // the updated GTF: the source string and gene tables came with the begin; l2r_novel_names has set the GTF-text unit up
    std::vector<uint8_t> h_src; GeneTables genes; int64_t anno_len = 0;
    DevBuf<uint32_t> e_qname, e_tidname;
    double stats[NVS_N] = {0};                          // l2r_novel_stats
};

// The GTF block of `bam2gtf` / `unique-gtf` (l2r_gtftext.hip.h): the reference names, source string and form of l2r_gtftext_begin, the
// transcripts of l2r_gtftext_rows, the selection of l2r_gtftext_blocks with what k_gtx_measure left per block, and the text of the last
// l2r_gtftext_lines (in HBM, or on the host where the host route made it) until l2r_gtftext_out fetches it.  The route is read at
// l2r_gtftext_rows and holds until the next; only the host route keeps copies of the columns (h).  The buffers belong to the context,
// grow on demand and are used again.
struct GtxState {
    bool begun = false, have_rows = false, have_blocks = false, on_host = false;
    bool run_chains = false;                            // rows came with xs == NULL: the exon chains of the context's last l2r_run
    l2r_gtx_params prm{};                               // ref_off / ref_names point into ref's vectors, src into h_src
    RefNames ref;
    std::vector<uint8_t> h_src; DevBuf<uint8_t> src;
    int64_t n = 0, m = 0, names_len = 0;
    double exons_per_row = 0;                           // of the run's chains (the host does not see them)
    std::vector<uint32_t> h_nex;                        // uploaded rows: exons per transcript (the form of k_gtx_measure)
    DevBuf<int32_t> tid, xs, xe, sel, start, end, cov; DevBuf<uint8_t> rev, names; DevBuf<int64_t> ex_off; DevBuf<uint32_t> id[4];
    const uint32_t *id_p[4] = {nullptr, nullptr, nullptr, nullptr};     // aliasing columns share one buffer
    bool has_sel = false, has_start = false, has_end = false, has_cov = false;
    struct Host {                                       // the host route's copies
        std::vector<int32_t> tid, xs, xe, sel, start, end, cov; std::vector<uint8_t> rev, names; std::vector<int64_t> ex_off; std::vector<uint32_t> id[4];
    } h;
    std::vector<uint32_t> h_len;                        // the measured bytes of every block of the selection
    DevBuf<uint32_t> len, fix, off, word;               // per block; off: one batch's lengths, scanned in place; word: GTXC_* and the scan's total
    DevBuf<unsigned long long> word64;                  // k_gtx_measure: the smallest bad block << 4 | kind, the lines
    TextOut out;
    StageTimer clk;
    double stats[14] = {0};                             // l2r_gtftext_stats
    // The read lists of `update-gtf -a / -k / -v / -u` (l2r_readlist.hip.h): the annotation's gene tables of l2r_gtftext_anno, the reads of
    // l2r_gtftext_reads and the selection of the last l2r_gtftext_list.  While `active`, the blocks of len / fix / h_len are those of
    // the list and l2r_gtftext_lines composes them with k_rl_write (or rl_text_host); l2r_gtftext_rows ends that.
    struct Lists {
        bool have_anno = false, have_reads = false, active = false;
        bool has_sj = false, split = false;
        l2r_gtx_anno anno{};                            // points into genes' vectors
        GeneTables genes;
        ReadRows reads;
        int64_t n_pieces = 0;
        int list = 0;
        RlSel h_sel;                                    // the host route's selection
        DevBuf<uint32_t> cnt, hfix, word;               // cnt: blocks per read, scanned in place (n + 1); hfix: per block; word[0]: the blocks, [1]: the piece blocks
        DevBuf<int32_t> b_read, b_first, b_count, b_piece;      // the selection
    } rl;
};

// The detail table of `update-gtf -A` (l2r_detail.hip.h): the reference names and the annotation's gene tables of l2r_detail_begin, the
// reads of l2r_detail_rows with what k_detail_measure left per read, and the text of the last l2r_detail_lines (in HBM, or on the host
// where the host route made it) until l2r_detail_out fetches it.  The route is read at l2r_detail_rows and holds until the next; only the
// host route keeps copies of the columns (rows.h).  The buffers belong to the context, grow on demand and are used again.
struct DetailState {
    bool begun = false, have_rows = false, on_host = false;
    l2r_detail_params prm{};                            // ref_off / ref_names point into ref's vectors, the gene tables into genes'
    RefNames ref;
    GeneTables genes;
    ReadRows rows;
    std::vector<uint32_t> h_len;                        // the measured bytes of every read
    DevBuf<uint32_t> len, split, off, word;             // len, split: per read; off: one batch's lengths, scanned in place; word: DETC_* and the scan's total
    DevBuf<unsigned long long> word64;                  // k_detail_measure: the smallest bad read << 4 | kind
    TextOut out;
    StageTimer clk;
    double stats[12] = {0};                             // l2r_detail_stats
};

// What l2r_sync has learned from the counters of a completed run of the tile path (fetch_run_facts): a later run of the same inputs,
// parameters and outputs sizes its list-driven launches by the counts and skips those whose list was empty.  One record, forgotten as a
// whole wherever one of those changes (forget_list_state).  LC_*: the list counter a field is a copy of (l2r_kernels.hip.h).
struct RunFacts {
    bool known = false;                 // a completed run has been looked at: what follows is what it left
    uint32_t n_wide = 0;                // LC_WIDE: entries of wide_list -- the grid of k_tile's WIDE instance
    uint32_t n_chunk = 0;               // LC_CHUNK: entries of chunk_list -- k_tile_chunk's grid
    uint32_t n_rest = 0;                // LC_REST: entries of rest_list -- the grid of k_tile's general instance beside the EXACT one
    uint32_t n_late = 0;                // LC_LATE: tiles a one-window kernel handed to the chunked kernel late -- the grid of k_tile_chunk's second launch
    uint32_t n_fb = 0;                  // LC_FB: tiles k_tile left in slab form for k_probe_slab
    uint32_t n_wide_rest = 0;           // LC_WIDE_REST: wide tiles that kept the slab form, for k_probe_slab_wide
    unsigned long long chunk_rest = 0;  // tiles left to k_probe_slab_chunked: with k_tile_chunk what its two launches declined (LC_DECLINED, LC_DECLINED_LATE), else every entry (LC_LATE + LC_CHUNK)
    bool redo_empty = false;            // TOT_REDO was 0: nothing for the generic kernel, and -- every read had its junction check in k_tile -- nothing for k_validate_sj
};

struct l2r_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // one-kernel tile path: the instances of k_tile that take the isoform-rich tiles (WIDE, CHUNK) need nothing of the plain instance --
    // their tiles' first slots are known since k_describe_scan -- and run BESIDE it on streams of their own (forked behind
    // k_describe_scan, joined in front of the list kernels): a few thousand long-lived workgroups fill in where the plain instance's
    // short ones leave CUs, instead of costing a launch each with a tail of its own.  L2R_SIDE=0: one behind the other on `stream`.
    // k_tile's general instance over the rest list runs beside the EXACT instance too, on side[0] in front of the WIDE instance -- but only
    // in runs WITHOUT an inexact tile (split_wait_free): then no tile of any instance waits for a count.  With inexact tiles the general
    // instance is their only publisher, and EXACT workgroups that wait for them keep their CU slots: it goes on the main stream IN FRONT
    // of the EXACT instance (launch_tile).  No stream of its own: with a third side stream two of the four streams shared a hardware queue.
    hipStream_t side[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};

    // ---- switches and device facts, read once at l2r_create
    int fast_grid = 0;                      // L2R_FAST_GRID: tests force many tiles per workgroup of k_classify_fast
    int n_cu = 256, wg_per_cu = 4;          // persistent grid of k_classify_fast (L2R_WG_PER_CU overrides)
    int ablate = 0;                         // diagnostics, L2R_ABLATE
    int64_t seg_max = SEG_MAX;              // tiles up to which the segmented scans are used (l2r_kernels.hip.h); L2R_SEG_MAX
    Pipeline want_pipe = Pipeline::tile;    // L2R_PIPELINE (see Pipeline); the default takes the tile path where the input allows it, else slab
    bool pipeline_forced = false;           // L2R_PIPELINE is set: the pipeline it names also for single-run uploads (tests, A/B runs)
    bool wide_direct = true;                // L2R_WIDE_DIRECT=0: the exact 64-bit-mask tiles keep the slab form and k_probe_slab_wide (k_tile's WIDE instance, l2r_tile.hip.h)
    bool chunk_direct = true;               // L2R_CHUNK_DIRECT=0: the exact tiles of the chunked kernel keep the slab form and k_probe_slab_chunked (k_tile_chunk, l2r_tchunk.hip.h)
    bool tile_split = true;                 // L2R_TILE_SPLIT=0: no EXACT instance of k_tile -- the general instance takes every tile (A/B runs, tests)
    bool side_on = true;                    // L2R_SIDE=0: no side streams
    bool env_tile_anyway = false, env_launch_all = false;   // L2R_TILE_ANYWAY / L2R_LAUNCH_ALL (diagnostics)
    bool check_stages = false;              // L2R_CHECK
    bool env_stamps = false;                // L2R_STAMPS (diagnostics): the next upload makes the `stamps` buffer
    int64_t tile_resident = 0;              // workgroups of k_tile the device holds at a time
    bool tile_starved = false;              // the device cannot hold the workgroups k_tile's look-back needs -- or (l2r_sync) a tile has waited in vain for the counts in front of it: the slab pipeline from then on
    int64_t n_lb_fallback = 0;              // runs that were done again on the slab pipeline for that reason (l2r_debug_counters)

    // ---- caller's settings
    l2r_params prm;
    std::string anno_cache_dir;             // L2R_ANNO_CACHE / l2r_set_annotation_cache: where the annotation tables are kept between runs
    int anno_cache_state = 0;               // last l2r_set_annotation: 0 no cache, 1 built + stored, 2 read from the cache
    unsigned want = L2R_WANT_RESULTS | L2R_WANT_ACCEPTED;      // l2r_set_outputs
    bool one_shot_upload = false;           // ONE run will follow the upload (l2r_classify, l2r_hint_single_run): see l2r_classify

    // ---- per upload (l2r_upload_reads)
    // ... what the upload's plan (UploadPlan, l2r_plan.hip.h) found: written by the upload alone
    bool sorted = true;
    int reads_per_tile = TILE_THREADS;
    int64_t n_tiles = 0, n_tiles256 = 0;
    bool wide_cigar = false;                // long CIGARs: the HBM walks fetch 16 words per lane and round
    bool many_exon_reads = false;           // the upload's sample: more than 0.5 % of the reads have more exons than a slab has rows
    bool slab_ok = false;                   // the upload can run the slab pipeline: coordinate-sorted records, short CIGARs, its slab layout fits
    bool have_index = false;                // the upload has its tile index (slot records, op statistics): the tile path is possible
    float index_ms = 0.0f;                  // GPU time of the upload's k_tile_index (l2r_upload_index_ms)
    DevBuf<SlotRec> slot_rec;               // the upload's slot records (k_tile_index)
    DevBuf<TileStat> tile_stat; std::vector<TileStat> h_tile_stat;      // the upload's index of the tiles' CIGAR operations (k_tile_index)
    DevBuf<TileStat> sup_stat;              // ... summed up per super-block of 1024 tiles
    DevBuf<uint16_t> sum_nn;                // the records' N operations (l2r_reads::cig_summary) for k_tile_index<true>
    DevBuf<uint32_t> tile_sbase, s_pre, s_loc, s_pl, cig_off32, tile_rec, tile_total, tile_xbase, tile_span;    // (tile_span: 16-byte TileSpan records, l2r_slab.hip.h)
    DevBuf<int32_t> dense_start, dense_end; // slab pipeline: the outliers' dense area
    DevBuf<uint32_t> slab_row;              //                the exon rows between its kernels (one word per exon)
    DevBuf<TileWin> tw;
    DevBuf<TileWin64> tw64; DevBuf<uint32_t> wide_list, chunk_list, list_cnt, tile_flags;     // tiles with 33 .. 63 window members (l2r_wide.hip.h); list_cnt: two blocks of LC_WORDS
    DevBuf<unsigned long long> ovf_cursor;
    DevBuf<unsigned long long> lb_tile, lb_blk, lb_sup;     // one-kernel tile path: the tiles' exon counts on their way to the later tiles' first slots
    DevBuf<uint32_t> fb_list;               //                       the tiles it leaves to k_probe_slab
    DevBuf<uint32_t> rest_list;             //                       the tiles k_describe_scan<true> has not marked for the EXACT instance

    // ---- per run: what the last launch did, and what completed runs have taught (forgotten with inputs, parameters or outputs: forget_list_state)
    Pipeline pipe = Pipeline::classic;      // what the last launch took (choose_pipeline)
    bool prev_run_tile = false;             // the last launch of this upload took the tile path (else the list counters are whatever a slab run left: cleared before the next tile run)
    uint32_t lc_flip = 0;                   // which of the two blocks of list counters the next run of the tile path uses (lc_this_run / lc_next_run / lc_last_run; lc_reset, end_of_run)
    uint32_t lb_flip = 0;                   // which of the two lb_sup arrays it uses (l2r_slab.hip.h SlabArgs::lb_sup)
    RunFacts facts;                         // the list counters and the redo count of a completed run of the tile path
    int64_t inexact_tiles = -1;             // tiles that are not exact under the parameters now set (-1: not counted yet; choose_pipeline counts)
    // annotation
    int64_t n_tx = 0, n_anno_exon = 0;
    DevBuf<TxHdr> hdr;
    DevBuf<int2> anno_ex;
    DevBuf<int64_t> anno_key;
    DevBuf<SiteEnt> sk_st, sk_en;                   // site dictionaries (l2r_kernels.hip.h): START / END entries
    DevBuf<uint32_t> sd_st, sd_en, sr_st;           // bucket directories, reach-back directory of START
    DevBuf<int32_t> tid_base; int32_t n_tid_dir = 0;
    DevBuf<uint32_t> key_dir; DevBuf<int32_t> kb_base; int32_t n_tid_key = 0;   // cursor directory
    DevBuf<int32_t> j0;
    int64_t n_compact = 0, n_wide = 0;
    std::vector<int64_t> h_anno_key_raw;    // per transcript (tid,end) key, NOT prefix-maxed (unsorted-input cursor)
    std::vector<int64_t> h_anno_key_pm;     // ... and its running maximum (what anno_key holds on the device)
    // junctions
    int64_t n_sj = 0;
    DevBuf<int32_t> sj_tid, sj_don, sj_acc, sj_uniq, sj_multi;
    DevBuf<int64_t> sj_key;
    DevBuf<int32_t> sj_cbase, sj_dbase; DevBuf<uint32_t> sj_cdir, sj_ddir; DevBuf<int4> sj_row; int32_t sj_ntid = 0;      // SjDir (l2r_kernels.hip.h)
    std::vector<int64_t> h_sj_key_raw;      // per row (tid,acc) key
    std::vector<int64_t> h_sj_key_pm;       // ... and its running maximum
    // reads
    int64_t n_reads = 0, n_cigar = 0, first_read = 0;
    DevBuf<int32_t> r_tid, r_pos;
    DevBuf<uint8_t> r_rev;
    DevBuf<int64_t> cig_off;
    DevBuf<uint32_t> cig;
    std::vector<int32_t> h_tid, h_pos;      // kept for unsorted input, and with a junction table (cursor carry, below)
    // One input may arrive as SEVERAL uploads (a single-GPU run too large for one shard: l2r_upload_reads with
    // first_read_index == the number of records uploaded so far).  The two sequential cursors of check_trans()
    // (src/update_gtf.c:938 last_anno_i, last_sj_i) are then carried from upload to upload, so that unsorted input
    // sees the same history as one sequential pass.
    struct Stream {
        bool valid = false, sorted = true;
        int64_t next = 0;                   // first_read_index a continuation must have
        int64_t last_key = INT64_MIN;       // (tid, pos) of the last record so far (sortedness across uploads)
        int64_t anno_cur = 0, sj_cur = 0;   // cursor values after everything uploaded (and, for sj_cur, classified) so far
        int64_t anno_cur_start = 0, sj_cur_start = 0;   // ... and at the start of the current upload
        bool sj_pending = false;            // the current upload used the device's prefix cursor: sj_cur is brought up to date at the next upload
    } seq;
    DevBuf<int32_t> win_start, sj_cursor;   // only for unsorted input
    bool have_win = false;
    // work + results
    DevBuf<uint32_t> local, tile_base, ex_off, info, tile_acc, tile_acc_ex, tile_acc_at, tile_acc_ex_at, tile_chunk, tile_rchunk, totals;  // totals: TOT_WORDS words, by name TOT_* (l2r_kernels.hip.h)
    DevBuf<uint32_t> redo;                  // reads the fast kernel hands to the generic one
    DevBuf<uint8_t> order;                  // per tile: reads by falling exon count (pass A)
    DevBuf<TileDesc> desc;
    DevBuf<int2> walked;               // long-CIGAR inputs: exons walked by pass A (n_cigar + n_reads slots)
    DevBuf<uint32_t> tile_first;       // first read of every tile (+ one closing entry)
    DevBuf<TxHdr> win_hdr;             // WIN_TX window headers per tile (pass A)
    DevBuf<int32_t> ex_start, ex_end, ref_tx;
    DevBuf<uint8_t> ex_flag;
    int64_t ex_cap = 0;
    DevBuf<AccRec> acc_rec;
    DevBuf<uint32_t> acc_ex_off;
    DevBuf<int32_t> acc_start, acc_end;
    DevBuf<uint8_t> acc_flag;
    bool ran = false;
    DevBuf<unsigned long long> stamps;      // diagnostics, L2R_STAMPS=1
    uint32_t h_totals[3] = {0, 0, 0};
    bool totals_valid = false;
    SjState sj;                             // `bam2sj`, `sjtab`
    SjIntrons sj_intr;                      // `sjtab`: l2r_sj_annotate
    double fusion_stats[5] = {0, 0, 0, 0, 0};        // `filter`, `fusion`: l2r_fusion_stats
    StageTimer fusion_clk;
    SortState sort;                         // `sort`, `filter -S`
    NameState name;                         // `sort -n`, `filter -N`, `fusion -N`
    GtfState gtf;                           // `sort-gtf`
    BedState bed;                           // `bam2bed`
    UniqState uniq;                         // `unique-gtf`
    GtxState gtx;                           // `bam2gtf`, `unique-gtf`: the GTF text
    DetailState detail;                     // `update-gtf -A`: the detail table
    SummaryState summary;                   // `update-gtf -y`: read classes and unique counts
    NovelState novel;                       // `update-gtf`: the novel list, its kept items, the BED text
};

// A launch (or a group of launches) on the context stream
template <typename F> int StageTimer::launch(l2r_ctx *c, double *ms, F f)
{
    if (on) HIP_TRY(hipEventRecord(ev[0], c->stream));
    f();
    HIP_TRY(hipGetLastError());
    if (on) {
        float t = 0.0f;
        HIP_TRY(hipEventRecord(ev[1], c->stream));
        HIP_TRY(hipEventSynchronize(ev[1]));
        HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
        *ms += t;
    }
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// What completed runs have shown about the tile path's lists and the inexact tiles: forgotten wherever inputs, parameters or outputs change
static void forget_list_state(l2r_ctx *c)
{
    c->facts = RunFacts{};
    c->inexact_tiles = -1;
}

// A completed run left nothing to the list-driven kernels behind k_tile (k_probe_slab, the WIDE instance / k_probe_slab_wide, k_tile_chunk /
// k_probe_slab_chunked): what ends up on their lists depends on nothing else, so none of them is launched until something changes
static bool lists_empty(const RunFacts &f) { return f.n_fb == 0u && f.n_wide == 0u && f.n_chunk == 0u && f.n_late == 0u; }
// ... or left most tiles in slab form (an isoform-rich annotation): k_tile would only walk for them, which k_walk_slab does faster -- later
// runs take the slab pipeline.  (The tiles k_tile's WIDE instance / k_tile_chunk take are no burden of the tile path.)
static bool lists_heavy(const l2r_ctx *c)
{
    const RunFacts &f = c->facts;
    return 2ull * ((unsigned long long)f.n_fb + (c->wide_direct ? f.n_wide_rest : f.n_wide) + f.chunk_rest) > (unsigned long long)c->n_tiles;
}
// Does a kernel over a list of n entries (as a completed run left it) run: unless that run has shown the list empty (L2R_LAUNCH_ALL: always)
static bool list_runs(const l2r_ctx *c, unsigned long long n) { return !c->facts.known || n != 0ull || c->env_launch_all; }
// ... and its grid when it has a workgroup per entry: the list's length once a run has shown it, until then one for every tile (most leave at once)
static unsigned list_grid(const l2r_ctx *c, uint32_t n) { return c->facts.known ? std::max(n, 1u) : (unsigned)std::max<int64_t>(c->n_tiles, 1); }

// The tile path's two blocks of list counters take turns run by run (SlabArgs::list_cnt_next): lc_flip names the block of the next run to
// be launched.  Three addresses: the block a run being launched counts in, the one it clears for the run behind it, and -- between
// runs, when end_of_run has flipped -- the block of the run that has just ended (of two blocks, the one that is not the next run's).
static uint32_t *lc_this_run(const l2r_ctx *c) { return c->list_cnt.p + LC_WORDS * (c->lc_flip & 1u); }
static uint32_t *lc_next_run(const l2r_ctx *c) { return c->list_cnt.p + LC_WORDS * ((c->lc_flip & 1u) ^ 1u); }
static uint32_t *lc_last_run(const l2r_ctx *c) { return lc_next_run(c); }
// Both blocks cleared and the turn back at block 0: at an upload, and in front of the first tile run behind a slab run (whose kernels
// leave their own counts in block 0)
static hipError_t lc_reset(l2r_ctx *c) { c->lc_flip = 0; return hipMemsetAsync(c->list_cnt.p, 0, 2 * LC_WORDS * sizeof(uint32_t), c->stream); }
// A run has been launched: the list counters and lb_sup (SlabArgs::lb_sup) change turns behind a run of the tile path
static void end_of_run(l2r_ctx *c, bool tile) { if (tile) { c->lb_flip ^= 1u; c->lc_flip ^= 1u; } c->prev_run_tile = tile; }

static DevParams dev_params(const l2r_ctx *c)
{
    DevParams p;
    p.min_exon = c->prm.min_exon; p.min_intron = c->prm.min_intron; p.max_delet = c->prm.max_delet;
    p.ss_dis = c->prm.ss_dis; p.full_level = c->prm.full_level; p.use_multi = c->prm.use_multi;
    p.min_sj_cnt = c->prm.min_sj_cnt; p.split_trans = c->prm.split_trans; p.frac = c->prm.single_exon_ovlp_frac;
    p.n_tx = (int32_t)c->n_tx; p.n_sj = (int32_t)c->n_sj; p.reads_per_tile = c->reads_per_tile;
    p.ablate = c->ablate; p.want = (int32_t)c->want;
    // (bits 9 / 10 leave the junction check to k_validate_sj: with a table no read is accepted yet when k_tile is done, so it must not place
    //  the tile's accepted chunk itself -- bit 1: every chunk is k_gather_accepted's)
    if (c->n_sj > 0 && (c->ablate & (512 | 1024))) p.ablate |= 2;
    return p;
}

// p.full_level (1 .. 5; anything else is 0: src/update_gtf.c:629-696, no evidence is gathered, full = lfull && rfull = 0) as a
// compile-time constant for the kernels' level parameter, and a run-time flag as a compile-time bool: f(constant)
template <typename F> static void with_level(int level, F &&f)
{
    switch (level) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    default: f(std::integral_constant<int, 0>()); break;
    }
}
template <typename F> static void with_flag(bool on, F &&f)
{
    if (on) f(std::true_type());
    else f(std::false_type());
}

// One instance of k_tile (l2r_tile.hip.h): the general one, WIDE over wide_list, EXACT over the tiles k_describe_scan<true> marked.
// (A template: in front of the C linkage block, with the others.)
template <bool WIDE, bool EXACT>
static void launch_k_tile(const l2r_ctx *c, const DevParams &p, const SlabArgs &sa, unsigned grid, hipStream_t st)
{
    // (k_tile decides acceptance itself, junction table or not; the WIDE instance's tiles leave their accepted chunks to k_gather_accepted)
    with_level(p.full_level, [&](auto L) { with_flag(p.ss_dis > 0, [&](auto D) { with_flag(!WIDE && (c->want & L2R_WANT_ACCEPTED), [&](auto A) {
        if constexpr (!(WIDE && A))
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tile<L, A, D, WIDE, EXACT>), dim3(grid), dim3(TILE_THREADS), 0, st, sa, (const TileRec *)c->tile_rec.p, (const TileWin *)c->tw.p,
                               (const TileStat *)c->tile_stat.p, (const SlotRec *)c->slot_rec.p, c->tile_xbase.p);
    }); }); });
}

// n elements of a host array / a host vector into a device buffer that grows to hold them: an asynchronous copy on the context stream
template <typename T> static int to_dev(l2r_ctx *c, DevBuf<T> &b, const T *src, size_t n)
{
    if (b.ensure(n ? n : 1)) return -2;
    if (n) HIP_TRY(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return 0;
}
template <typename T> static int put_dev(l2r_ctx *c, DevBuf<T> &b, const std::vector<T> &v) { return to_dev(c, b, v.data(), v.size()); }

// The tail of an entry point of a table command.  rc: what uploads and launches came to; where that is 0 the downloads are queued.  The
// stream is waited for in any case (the host columns are the caller's, device buffers may be the caller's locals), and the first error is
// the result.
struct Download { void *dst; const void *src; size_t bytes; };
static int download_all(l2r_ctx *c, int rc, std::initializer_list<Download> list, const char *who)
{
    hipError_t e = hipSuccess;
    if (!rc) for (const Download &d : list) if (e == hipSuccess && d.bytes) e = hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, c->stream);
    const hipError_t sync = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = sync;
    if (!rc && e != hipSuccess) rc = fail(-2, "[%s] %s", who, hipGetErrorString(e));
    return rc;
}

static bool env_on(const char *name) { const char *e = getenv(name); return e && atoi(e) != 0; }
// L2R_BED_ROUTE, L2R_UNIQ_ROUTE, L2R_GTX_ROUTE, L2R_DETAIL_ROUTE = host: the exact host routine instead of the kernels (tests, comparators)
static bool route_is_host(const char *env) { const char *e = getenv(env); return e && strcmp(e, "host") == 0; }

// The form of a measure kernel (k_fusion_seg, k_bed_measure, k_gtx_measure, k_detail_measure): one wave per item where the items are long, above 32 words
// on average -- the bound of l2r_upload_reads' wide_cigar (upload_plan, l2r_plan.hip.h).  env (L2R_FUSION_WAVE, L2R_BED_WAVE,
// L2R_GTX_WAVE, L2R_DETAIL_WAVE) = 0|1 says otherwise: tests, tools/bench_*.py
static bool wave_form(double per_item, const char *env)
{
    if (const char *e = getenv(env)) return atoi(e) != 0;
    return per_item > 32.0;
}

// what is behind the l2r_*_stats of the table commands: the `have` words of src, then zeros
static int stats_out(const double *src, int have, double *out, int n, const char *who)
{
    if (!src || !out || n < 0) return fail(-1, "[%s] bad argument", who);
    for (int k = 0; k < n; ++k) out[k] = k < have ? src[k] : 0.0;
    return 0;
}

int RefNames::upload(l2r_ctx *c)
{
    if (int rc = put_dev(c, off, h_off)) return rc;
    return put_dev(c, names, h_names);
}

int GeneTables::upload(l2r_ctx *c) { int rc; return (rc = put_dev(c, names, h_names)) || (rc = put_dev(c, gid, h_gid)) || (rc = put_dev(c, gname, h_gname)) ? rc : 0; }

hipError_t TextOut::arm_guard(const l2r_ctx *c, size_t B) { return c->check_stages ? hipMemsetAsync(bytes() + B, TEXT_GUARD_BYTE, TEXT_SLACK, c->stream) : hipSuccess; }
hipError_t TextOut::fetch_guard(const l2r_ctx *c, size_t B) { return c->check_stages ? hipMemcpyAsync(guard, bytes() + B, TEXT_SLACK, hipMemcpyDeviceToHost, c->stream) : hipSuccess; }
bool TextOut::guard_intact(const l2r_ctx *c) const
{
    if (c->check_stages) for (size_t k = 0; k < TEXT_SLACK; ++k) if (guard[k] != TEXT_GUARD_BYTE) return false;
    return true;
}

// What is behind l2r_bed_text_out, l2r_gtftext_out and l2r_detail_out: the text into the caller's `cap` bytes.  arg_code: of an argument or order error.
static int text_out(l2r_ctx *c, const TextOut &t, uint8_t *text, int64_t cap, const char *who, const char *lines, int arg_code)
{
    if (!t.have) return fail(arg_code, "[%s] no text: the last %s failed, or none was made", who, lines);
    if (cap < t.n_bytes) return fail(arg_code, "[%s] room for %lld bytes, the last %s left %lld", who, (long long)cap, lines, (long long)t.n_bytes);
    if (t.n_bytes == 0) return 0;
    if (!text) return fail(arg_code, "[%s] null text", who);
    if (t.on_host) { memcpy(text, t.host_text.data(), (size_t)t.n_bytes); return 0; }
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(-2, "[%s] hipSetDevice: %s", who, hipGetErrorString(e));
    return download_all(c, 0, {{text, t.text.p, (size_t)t.n_bytes}}, who);
}

extern "C" {

int l2r_abi_version(void) { return L2R_ABI_VERSION; }
const char *l2r_last_error(void) { return g_err; }

int l2r_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

l2r_ctx *l2r_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { fail(-1, "[l2r_create] no HIP device available (%s); this library has no CPU path", hipGetErrorString(e)); return nullptr; }
    if (device < 0 || device >= n) { fail(-1, "[l2r_create] device %d out of range (have %d)", device, n); return nullptr; }
    if ((e = hipSetDevice(device)) != hipSuccess) { fail(-2, "[l2r_create] hipSetDevice: %s", hipGetErrorString(e)); return nullptr; }
    l2r_ctx *c = new l2r_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        fail(-2, "[l2r_create] hipStreamCreate: %s", hipGetErrorString(e)); delete c; return nullptr;
    }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // (lowest, highest)
    // (the side streams carry the long-lived workgroups: highest priority, so that they are on their way early and the plain instance's short ones
    //  fill in -- measured on cfg3_gencode: lowest 0.665, default 0.660, highest 0.658 ms: the dispatcher hardly cares)
    for (int k = 0; k < 2; ++k)
        if (((e = hipStreamCreateWithPriority(&c->side[k], hipStreamNonBlocking, prio_hi)) != hipSuccess &&
             ((void)hipGetLastError(), e = hipStreamCreateWithFlags(&c->side[k], hipStreamNonBlocking)) != hipSuccess) ||      // (a runtime without stream priorities: a plain stream does)
            (e = hipEventCreateWithFlags(&c->ev_join[k], hipEventDisableTiming)) != hipSuccess) {
            fail(-2, "[l2r_create] side stream: %s", hipGetErrorString(e)); l2r_destroy(c); return nullptr;
        }
    if ((e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess) { fail(-2, "[l2r_create] hipEventCreate: %s", hipGetErrorString(e)); l2r_destroy(c); return nullptr; }
    // src/update_gtf.c:24-35 defaults
    c->prm = l2r_params{3, 3, 50, 0, 0x7fffffff, 5, 0, 0, 1, 0, 0.80f};
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
        const char *e = getenv("L2R_WG_PER_CU");
        if (e && atoi(e) > 0) c->wg_per_cu = atoi(e);
        e = getenv("L2R_FAST_GRID");
        if (e && atoi(e) > 0) c->fast_grid = atoi(e);
        e = getenv("L2R_ABLATE");
        c->ablate = e ? atoi(e) : 0;
        c->check_stages = getenv("L2R_CHECK") != nullptr;
        e = getenv("L2R_SEG_MAX");                       // diagnostics / tests: tiles beyond which the scans take k_scan_u32 in a launch of its own
        if (e && atoll(e) >= 0) c->seg_max = atoll(e);
        e = getenv("L2R_ANNO_CACHE");
        if (e && *e) c->anno_cache_dir = e;
        e = getenv("L2R_WIDE_DIRECT");
        if (e) c->wide_direct = atoi(e) != 0;
        c->env_tile_anyway = getenv("L2R_TILE_ANYWAY") != nullptr; c->env_launch_all = getenv("L2R_LAUNCH_ALL") != nullptr;
        e = getenv("L2R_CHUNK_DIRECT");
        if (e) c->chunk_direct = atoi(e) != 0;
        e = getenv("L2R_TILE_SPLIT");
        if (e) c->tile_split = atoi(e) != 0;
        e = getenv("L2R_SIDE");
        if (e) c->side_on = atoi(e) != 0;
        c->env_stamps = getenv("L2R_STAMPS") != nullptr;
        e = getenv("L2R_PIPELINE");
        if (e) { c->want_pipe = !strcmp(e, "classic") ? Pipeline::classic : !strcmp(e, "slab") ? Pipeline::slab : Pipeline::tile; c->pipeline_forced = true; }
        {   // k_tile's look-back: a tile may wait for one whose workgroup comes up to 8 * TILE_GROUP - 1 block indices later (fused_tile), so
            // that many workgroups + 1 have to be resident together -- guaranteed nowhere; checked here (small or partitioned devices, CU
            // masks): a device that cannot hold them takes the slab pipeline from the start
            int per_cu = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_tile<3, false, false, false>, TILE_THREADS, 0) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
            c->tile_resident = (int64_t)per_cu * c->n_cu;
            if ((int64_t)per_cu * c->n_cu < 8 * (int64_t)TILE_GROUP + 1 || getenv("L2R_TILE_STARVED")) c->tile_starved = true;
        }
    }
    return c;
}

void l2r_destroy(l2r_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);                      // (the device buffers go with `delete c`)
    for (int k = 0; k < 2; ++k) { if (c->side[k]) (void)hipStreamDestroy(c->side[k]); if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void *l2r_stream(l2r_ctx *c) { return c ? (void *)c->stream : nullptr; }
float l2r_upload_index_ms(l2r_ctx *c) { return c ? c->index_ms : 0.0f; }
int l2r_hint_single_run(l2r_ctx *c, int on) { if (!c) return fail(-1, "[l2r_hint_single_run] null context"); c->one_shot_upload = on != 0; return 0; }

int l2r_set_outputs(l2r_ctx *c, unsigned want)
{
    if (!c) return fail(-1, "[l2r_set_outputs] null context");
    if (!(want & (L2R_WANT_RESULTS | L2R_WANT_ACCEPTED)) || (want & ~(unsigned)(L2R_WANT_RESULTS | L2R_WANT_ACCEPTED)))
        return fail(-1, "[l2r_set_outputs] want = %u: expected L2R_WANT_RESULTS and/or L2R_WANT_ACCEPTED", want);
    // The per-read result arrays are always produced on the device (the junction check and the redo list read them);
    // what the flag saves is the compaction of the accepted list (kernel work, 16 + 9n bytes per accepted read).
    c->want = want;
    c->ran = false; forget_list_state(c);
    return 0;
}

int l2r_set_params(l2r_ctx *c, const l2r_params *prm)
{
    if (!c || !prm) return fail(-1, "[l2r_set_params] null argument");
    c->prm = *prm;
    c->ran = false; forget_list_state(c);
    return 0;
}

int l2r_set_annotation_cache(l2r_ctx *c, const char *dir)
{
    if (!c) return fail(-1, "[l2r_set_annotation_cache] null context");
    c->anno_cache_dir = dir ? dir : "";
    return 0;
}

int l2r_annotation_cache_state(l2r_ctx *c) { return c ? c->anno_cache_state : -1; }

int l2r_set_annotation(l2r_ctx *c, const l2r_annotation *a)
{
    if (!c || !a) return fail(-1, "[l2r_set_annotation] null argument");
    if (a->n_tx < 0 || a->n_tx > 0x7ffffff0LL || a->n_exon < 0 || a->n_exon > 0x7ffffff0LL) return fail(-1, "[l2r_set_annotation] size out of range");
    HIP_TRY(hipSetDevice(c->device));
    AnnoTables t;
    std::string msg;
    c->anno_cache_state = 0;
    const int state = anno_tables(a, c->anno_cache_dir, t, msg);
    if (state < 0) return fail(-1, "%s", msg.c_str());
    c->anno_cache_state = state;
    int rc = 0;
    if ((rc = put_dev(c, c->sk_st, t.st_ent)) || (rc = put_dev(c, c->sd_st, t.st_dir)) || (rc = put_dev(c, c->sr_st, t.st_rdir)) ||
        (rc = put_dev(c, c->sk_en, t.en_ent)) || (rc = put_dev(c, c->sd_en, t.en_dir)) || (rc = put_dev(c, c->tid_base, t.tid_base)) ||
        (rc = put_dev(c, c->key_dir, t.key_dir)) || (rc = put_dev(c, c->kb_base, t.kb_base)) || (rc = put_dev(c, c->hdr, t.hdr)) ||
        (rc = put_dev(c, c->anno_key, t.key)) || (rc = put_dev(c, c->anno_ex, t.ex))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));              // (t is a local)
    c->h_anno_key_raw.swap(t.key_raw);
    c->h_anno_key_pm.swap(t.key);
    c->seq = l2r_ctx::Stream();
    c->n_compact = t.n_compact; c->n_wide = t.n_wide; c->n_tid_dir = t.n_tid_dir; c->n_tid_key = t.n_tid_key;
    c->n_tx = a->n_tx; c->n_anno_exon = a->n_exon;
    c->have_win = false; c->ran = false; forget_list_state(c);
    return 0;
}

int l2r_set_junctions(l2r_ctx *c, const l2r_junctions *s)
{
    if (!c) return fail(-1, "[l2r_set_junctions] null context");
    HIP_TRY(hipSetDevice(c->device));
    c->ran = false; forget_list_state(c);
    if (!s || s->n == 0) { c->n_sj = 0; c->h_sj_key_raw.clear(); c->h_sj_key_pm.clear(); c->seq = l2r_ctx::Stream(); return 0; }
    SjTables t;
    std::string msg;
    if (build_sj_tables(s, t, msg)) return fail(-1, "%s", msg.c_str());
    const size_t n = (size_t)s->n;
    int rc = 0;
    if ((rc = put_dev(c, c->sj_row, t.row)) || (rc = put_dev(c, c->sj_cbase, t.cbase)) || (rc = put_dev(c, c->sj_cdir, t.cdir)) ||
        (rc = put_dev(c, c->sj_dbase, t.dbase)) || (rc = put_dev(c, c->sj_ddir, t.ddir)) ||
        (rc = to_dev(c, c->sj_tid, s->tid, n)) || (rc = to_dev(c, c->sj_don, s->don, n)) || (rc = to_dev(c, c->sj_acc, s->acc, n)) ||
        (rc = to_dev(c, c->sj_uniq, s->uniq_c, n)) || (rc = to_dev(c, c->sj_multi, s->multi_c, n)) || (rc = put_dev(c, c->sj_key, t.key))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));              // (t is a local)
    c->sj_ntid = t.n_tid;
    c->n_sj = s->n;
    c->h_sj_key_raw.swap(t.key_raw);
    c->h_sj_key_pm.swap(t.key);
    c->seq = l2r_ctx::Stream();
    return 0;
}

static int prepare_unsorted_windows(l2r_ctx *c);
static int finish_stream_sj_cursor(l2r_ctx *c);

// is this upload the continuation of the previous one?  (see l2r_ctx::Stream; its sorted / last_key follow from the plan)
static int stream_begin_upload(l2r_ctx *c, const l2r_reads *r)
{
    l2r_ctx::Stream &st = c->seq;
    const bool cont = st.valid && r->first_read_index > 0 && r->first_read_index == st.next;
    if (cont) { int rc = finish_stream_sj_cursor(c); if (rc) return rc; }      // (needs the previous upload's results: before they are overwritten)
    else st = l2r_ctx::Stream();
    st.anno_cur_start = st.anno_cur; st.sj_cur_start = st.sj_cur;
    st.next = r->first_read_index + r->n_reads; st.valid = true;
    st.sj_pending = false;
    return 0;
}

// the five record columns and the tiles' first reads
static int stage_reads(l2r_ctx *c, const l2r_reads *r, const UploadPlan &pl)
{
    const int64_t N = r->n_reads;
    if (c->tile_first.ensure(pl.tile_first.size())) return -2;
    HIP_TRY(hipMemcpyAsync(c->tile_first.p, pl.tile_first.data(), pl.tile_first.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (c->r_tid.ensure((size_t)N) || c->r_pos.ensure((size_t)N) || c->r_rev.ensure((size_t)N) ||
        c->cig_off.ensure((size_t)N + 1) || c->cig.ensure((size_t)r->n_cigar + 8)) return -2;     // + 8: the kernels read whole 16-byte vectors (pass A: two per lane)
    if (N) {
        HIP_TRY(hipMemcpyAsync(c->r_tid.p, r->tid, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->r_pos.p, r->pos, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->r_rev.p, r->rev, (size_t)N, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->cig_off.p, r->cig_off, (size_t)(N + 1) * 8, hipMemcpyHostToDevice, c->stream));
        if (r->n_cigar) HIP_TRY(hipMemcpyAsync(c->cig.p, r->cig, (size_t)r->n_cigar * 4, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// work buffers.  n_exon(read) <= ops(read) + 1, so n_cigar + n_reads bounds the exon arrays; for long CIGARs (hundreds of
// M/I/D ops per exon) that bound is 10-50 times too generous, so the ops that can end an exon at all (N, D) are
// counted on the device (one pass over the words that were just uploaded; sizing only, nothing of it is kept).
static int count_exon_bound(l2r_ctx *c, const l2r_reads *r, bool wide_cigar, size_t *exb)
{
    *exb = (size_t)r->n_cigar + (size_t)r->n_reads;
    if (!wide_cigar) return 0;
    if (c->totals.ensure(TOT_WORDS)) return -2;
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->totals.p);
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, c->stream));
    hipLaunchKernelGGL(k_count_cut_ops, dim3(4096), dim3(TILE_THREADS), 0, c->stream, (const uint32_t *)c->cig.p, (int64_t)r->n_cigar, d_cnt);
    unsigned long long cuts = 0;
    HIP_TRY(hipMemcpyAsync(&cuts, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *exb = (size_t)cuts + (size_t)r->n_reads;
    return 0;
}

static int reserve_work(l2r_ctx *c, size_t n_reads, size_t exb)
{
    const size_t N = n_reads, T = (size_t)c->n_tiles;
    if (c->j0.ensure(N) || c->local.ensure(N + 1) || c->ex_off.ensure(N) || c->info.ensure(N) || c->ref_tx.ensure(N) ||
        c->redo.ensure(N) || c->order.ensure(N + TILE_THREADS) || c->desc.ensure(T) || c->win_hdr.ensure(T * WIN_TX) ||
        c->tile_base.ensure(T + 1) || c->tile_acc.ensure(T + 1) || c->tile_acc_ex.ensure(T + 1) ||
        c->tile_acc_at.ensure(T + 2) || c->tile_acc_ex_at.ensure(T + 2) ||
        c->totals.ensure(TOT_WORDS) || c->tile_chunk.ensure(T + 1) || c->tile_rchunk.ensure(T + 1) || c->ex_start.ensure(exb) || c->ex_end.ensure(exb) || c->ex_flag.ensure(exb) ||
        c->acc_rec.ensure(N) || c->acc_ex_off.ensure(N) ||
        c->acc_start.ensure(exb) || c->acc_end.ensure(exb) || c->acc_flag.ensure(exb) || (c->wide_cigar && c->walked.ensure((T + 1) * LDS_EXON_CAP))) return -2;
    c->ex_cap = (int64_t)exb;
    return 0;
}

// the slab pipeline's buffers, and what the plan has laid out for them
static int stage_slab(l2r_ctx *c, size_t n_reads, const UploadPlan &pl)
{
    const size_t N = n_reads, T = (size_t)pl.n_tiles;
    if (c->tw64.ensure(T + 1) || c->wide_list.ensure(2 * (T + 1)) || c->chunk_list.ensure(2 * (T + 1)) || c->list_cnt.ensure(2 * LC_WORDS) || c->tile_flags.ensure(T + 8) ||
        c->lb_tile.ensure(T + 64) || c->lb_blk.ensure(T / LB_BLK + 64) || c->lb_sup.ensure(2 * ((T >> LB_SUP_SHIFT) + 64)) || c->fb_list.ensure(T + 1) || c->rest_list.ensure(T + 1) || c->tile_stat.ensure(T + 1) || c->sup_stat.ensure((T >> LB_SUP_SHIFT) + 2) ||
        (!c->wide_cigar && c->slot_rec.ensure((T + 1) * TILE_THREADS))) return -2;
    HIP_TRY(hipMemsetAsync(c->lb_sup.p, 0, 2 * ((T >> LB_SUP_SHIFT) + 64) * 8, c->stream)); c->lb_flip = 0;      // (two arrays taking turns; from then on each is cleared by the run in front of its own)      // (an isoform-rich annotation makes EVERY tile wide: 2.4 KB each)
    HIP_TRY(lc_reset(c)); c->prev_run_tile = false;
    if (c->tile_sbase.ensure(T + 1) || c->ovf_cursor.ensure(1) || c->tw.ensure(T + 1) || c->tile_total.ensure(T + 2) || c->tile_xbase.ensure(T + 2) || c->tile_span.ensure(12 * (T + 1)) ||
        c->s_pre.ensure(N + 1) || c->s_loc.ensure(N + 1) ||
        c->slab_row.ensure((size_t)pl.slab_total + 4) ||
        c->dense_start.ensure((size_t)pl.dense_rows + 1) || c->dense_end.ensure((size_t)pl.dense_rows + 1)) return -2;
    HIP_TRY(hipMemsetAsync(c->ovf_cursor.p, 0, 8, c->stream));
    HIP_TRY(hipMemcpyAsync(c->tile_sbase.p, pl.sbase.data(), (T + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (c->tile_rec.ensure(8 * (T + 1)) || c->cig_off32.ensure(N + 2) || c->s_pl.ensure(N + 1)) return -2;
    HIP_TRY(hipMemcpyAsync(c->tile_rec.p, pl.rec.data(), pl.rec.size() * sizeof(TileRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->cig_off32.p, pl.off32.data(), pl.off32.size() * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// the upload's tile index (k_tile_index): the slot records, and the tiles' statistics -- which come from the plan where the reader's
// summaries made them, and from the kernel's walk of the CIGARs where not.  Leaves them in h_tile_stat either way.
static int make_tile_index(l2r_ctx *c, const l2r_reads *r, const UploadPlan &pl)
{
    const size_t N = (size_t)r->n_reads, T = (size_t)pl.n_tiles;
    const bool summaries = r->cig_summary != nullptr;
    c->h_tile_stat = pl.tile_stat;
    c->index_ms = 0.0f; c->have_index = pl.have_index;
    if (!pl.have_index) return 0;
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a)); HIP_TRY(hipEventCreate(&ev.b));
    if (summaries) {
        if (c->sum_nn.ensure(N + 1)) return -2;
        HIP_TRY(hipMemcpyAsync(c->sum_nn.p, pl.nn.data(), N * 2, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->tile_stat.p, c->h_tile_stat.data(), T * sizeof(TileStat), hipMemcpyHostToDevice, c->stream));
    }
    const unsigned gi = (unsigned)std::min<size_t>(T, 8192);
    HIP_TRY(hipEventRecord(ev.a, c->stream));
    with_flag(summaries, [&](auto S) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tile_index<S>), dim3(gi), dim3(TILE_THREADS), 0, c->stream, (TileRec *)c->tile_rec.p, c->tile_stat.p, c->slot_rec.p, (uint32_t)T,
                           (const uint32_t *)c->cig_off32.p, (const int32_t *)c->r_pos.p, (const uint8_t *)c->r_rev.p, (const uint32_t *)c->cig.p, S ? (const uint16_t *)c->sum_nn.p : (const uint16_t *)nullptr);
    });
    HIP_TRY(hipEventRecord(ev.b, c->stream));
    if (!summaries) {
        HIP_TRY(hipMemcpyAsync(c->h_tile_stat.data(), c->tile_stat.p, T * sizeof(TileStat), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));       // (sup_stat is made from them)
    }
    HIP_TRY(hipEventSynchronize(ev.b));
    HIP_TRY(hipEventElapsedTime(&c->index_ms, ev.a, ev.b));
    return 0;
}

int l2r_upload_reads(l2r_ctx *c, const l2r_reads *r)
{
    if (!c || !r) return fail(-1, "[l2r_upload_reads] null argument");
    if (r->n_reads < 0 || r->n_cigar < 0) return fail(-1, "[l2r_upload_reads] negative size");
    // exon offsets are 32 bit on the device: n_exon(read) <= n_cigar(read) + 1
    if ((uint64_t)r->n_cigar + (uint64_t)r->n_reads >= 0xfffffff0ULL)
        return fail(-1, "[l2r_upload_reads] shard too large for 32-bit exon offsets (%lld ops + %lld reads); split it", (long long)r->n_cigar, (long long)r->n_reads);
    HIP_TRY(hipSetDevice(c->device));
    const int64_t N = r->n_reads;
    // The plan and the super-block sums are the source of asynchronous copies: they live until the function returns, and whichever way
    // it returns the stream has drained by then
    UploadPlan pl;
    std::vector<TileStat> sup;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{c->stream};
    std::string msg;
    if (int rc = plan_check_reads(*r, pl, msg)) return fail(rc, "%s", msg.c_str());

    if (int rc = stream_begin_upload(c, r)) return rc;

    PlanOpts po;
    po.min_intron = c->prm.min_intron; po.max_delet = c->prm.max_delet;
    po.want_slab = c->want_pipe != Pipeline::classic;
    po.want_index = c->want_pipe == Pipeline::tile && !(c->one_shot_upload && !c->env_tile_anyway && !c->pipeline_forced);
    po.stream_sorted = c->seq.sorted; po.last_key = c->seq.last_key;
    plan_tiles(*r, po, pl);
    c->seq.sorted = pl.sorted; c->seq.last_key = pl.last_key;
    const bool sorted = pl.sorted;
    c->sorted = sorted; c->have_win = false;
    if (!sorted || c->n_sj > 0) { c->h_tid.assign(r->tid, r->tid + N); c->h_pos.assign(r->pos, r->pos + N); }
    else { c->h_tid.clear(); c->h_pos.clear(); }
    c->wide_cigar = pl.wide_cigar; c->many_exon_reads = pl.many_exon_reads;
    c->reads_per_tile = pl.reads_per_tile; c->n_tiles = pl.n_tiles; c->n_tiles256 = pl.n_tiles256;

    if (int rc = stage_reads(c, r, pl)) return rc;
    size_t exb = 0;
    if (int rc = count_exon_bound(c, r, pl.wide_cigar, &exb)) return rc;
    if (int rc = reserve_work(c, (size_t)N, exb)) return rc;

    plan_slab(*r, exb, pl);
    c->slab_ok = pl.slab_ok; c->pipe = Pipeline::classic;
    if (pl.slab_ok) {
        if (int rc = stage_slab(c, (size_t)N, pl)) return rc;
        if (int rc = make_tile_index(c, r, pl)) return rc;
        sup = plan_sup_stat(pl, c->h_tile_stat);
        HIP_TRY(hipMemcpyAsync(c->sup_stat.p, sup.data(), sup.size() * sizeof(TileStat), hipMemcpyHostToDevice, c->stream));
    }
    if (c->env_stamps && !c->stamps.p) {
        if (c->stamps.ensure(1024 * 8 + 16)) return -2;
        HIP_TRY(hipMemsetAsync(c->stamps.p, 0, (1024 * 8 + 16) * 8, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));

    c->n_reads = N; c->n_cigar = r->n_cigar; c->first_read = r->first_read_index;
    c->ran = false; c->totals_valid = false; forget_list_state(c);
    if (sorted) {
        // the annotation cursor after a sorted prefix is the prefix function of its last record
        if (N) c->seq.anno_cur = std::max(c->seq.anno_cur, cursor_after(c->h_anno_key_pm, r->tid[N - 1], r->pos[N - 1]));
        c->seq.sj_pending = c->n_sj > 0;
    } else {
        int rc = prepare_unsorted_windows(c);            // replays the cursor now, so that the next upload can continue it
        if (rc) return rc;
    }
    return 0;
}

// Brings Stream::sj_cur up to date after an upload whose junction cursor ran on the device (sorted so far): the
// reference's last_sj_i only moves for reads that reach check_short_sj (src/update_gtf.c:947,613-614), so it is the
// prefix function of the LAST such read -- known only once that upload has been classified.
static int finish_stream_sj_cursor(l2r_ctx *c)
{
    l2r_ctx::Stream &st = c->seq;
    if (!st.sj_pending || !c->ran || c->n_sj == 0 || c->n_reads == 0) { st.sj_pending = false; return 0; }
    const int64_t N = c->n_reads;
    std::vector<uint32_t> info((size_t)N);
    HIP_TRY(hipMemcpyAsync(info.data(), c->info.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = N - 1; i >= 0; --i) {
        if ((info[(size_t)i] & (I_FULL | I_KNOWN | I_KSITE)) != (I_FULL | I_KSITE)) continue;
        st.sj_cur = std::max(st.sj_cur, cursor_after(c->h_sj_key_pm, c->h_tid[(size_t)i], c->h_pos[(size_t)i]));
        break;
    }
    st.sj_pending = false;
    return 0;
}

// Unsorted input: the annotation cursor is history dependent (update_gtf.c:801-802).  Replay it on the
// host (O(N + T)); the per-read work still runs on the GPU.
static int prepare_unsorted_windows(l2r_ctx *c)
{
    if (c->sorted || c->have_win) return 0;
    const int64_t N = c->n_reads;
    std::vector<int32_t> w((size_t)N);
    // (from anno_cur_start: 0 unless this upload continues an earlier one)
    c->seq.anno_cur = cursor_replay(c->h_anno_key_raw, c->seq.anno_cur_start, c->h_tid.data(), c->h_pos.data(), N, w.data(), [](int64_t) { return true; });
    if (c->win_start.ensure((size_t)N)) return -2;
    if (N) HIP_TRY(hipMemcpyAsync(c->win_start.p, w.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_win = true;
    return 0;
}

// Unsorted input with a junction table: the junction cursor only moves for reads that reach the check
// (update_gtf.c:947), so it needs the classification first.
static int prepare_unsorted_sj_cursor(l2r_ctx *c)
{
    const int64_t N = c->n_reads;
    std::vector<uint32_t> info((size_t)N);
    if (N) HIP_TRY(hipMemcpyAsync(info.data(), c->info.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> cur_v((size_t)N);
    // (from sj_cur_start: 0 unless this upload continues an earlier one)
    c->seq.sj_cur = cursor_replay(c->h_sj_key_raw, c->seq.sj_cur_start, c->h_tid.data(), c->h_pos.data(), N, cur_v.data(),
                                  [&](int64_t i) { return (info[(size_t)i] & (I_FULL | I_KNOWN | I_KSITE)) == (I_FULL | I_KSITE); });
    if (c->sj_cursor.ensure((size_t)N)) return -2;
    if (N) HIP_TRY(hipMemcpyAsync(c->sj_cursor.p, cur_v.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

enum { ST_PASS_A = 0, ST_SCAN1, ST_FAST, ST_GENERIC, ST_SJ, ST_SCAN2, ST_GATHER, ST_N };

// Which pipeline the next launch takes: what the upload allows (slab_ok, have_index), the parameters, and what earlier runs of the
// same upload and parameters have shown (inexact tiles, lists_heavy, a starved look-back)
static Pipeline choose_pipeline(l2r_ctx *c, const DevParams &p)
{
    // the slab pipeline wants the straight-line walk: thresholds that fit a CIGAR word (else: the classic kernels)
    if (!(c->slab_ok && p.min_intron >= 0 && p.min_intron < (1 << 28) && p.max_delet >= -1 && p.max_delet < (1 << 28) - 1 &&
          (!c->wide_cigar || p.min_exon >= 1)))           // (k_walk_slab_long has no -e < 1 form: the classic kernels take that)
        return Pipeline::classic;
    // the one-kernel tile path: short CIGARs whose exon counts the CIGAR lengths bound (-e >= 1)
    if (c->want_pipe != Pipeline::tile || c->wide_cigar || p.min_exon < 1 || !(c->have_index || c->n_tiles == 0) || c->tile_starved)
        return Pipeline::slab;
    // A tile whose exon count the first kernel cannot derive from the upload's index (a threshold is borderline in it) publishes it
    // from k_tile, and every later tile's write-out waits for it: fine for a few, a convoy for many (measured: 3 x the kernel when
    // every tile does) -- such a run takes the two-kernel path.
    if (c->inexact_tiles < 0) {     // (depends on the upload and the parameters alone: counted once, forgotten with them -- forget_list_state)
        int64_t inexact = 0;
        for (const TileStat &st : c->h_tile_stat) inexact += tile_exact(st, p.min_exon, p.min_intron, p.max_delet) ? 0 : 1;
        c->inexact_tiles = inexact;
    }
    if (c->inexact_tiles * 50 > c->n_tiles + 800 && !c->env_tile_anyway) return Pipeline::slab;
    // (measured: cfg3_iso40 -- every tile wide or chunked -- 1.34 ms on this path against 1.26 on the slab pipeline)
    if (c->facts.known && lists_heavy(c) && !c->env_tile_anyway) return Pipeline::slab;
    return Pipeline::tile;
}

// The stage boundaries of a launch: per-stage events (l2r_run_timed); L2R_CHECK=1 (diagnostics): wait for the device at every one, so
// that a kernel fault is reported with the stage it happened in instead of at the next synchronisation of the caller
static const char *const stage_name[ST_N + 1] = {"(start)", "pass A / order", "scan / walk", "classification", "generic", "junction check", "accepted scan", "accepted gather"};
#define MARK(i) do { if (ev) HIP_TRY(hipEventRecord(ev[i], c->stream)); \
        if (c->check_stages) { const hipError_t e_ = hipStreamSynchronize(c->stream); \
            if (e_ != hipSuccess) return fail(-2, "[launch_all] device error behind stage \"%s\": %s", stage_name[i], hipGetErrorString(e_)); } } while (0)

static FastArgs fast_args(const l2r_ctx *c, const DevParams &p, const SiteTabs &tabs, const int32_t *j0)
{
    FastArgs fa;
    fa.n_reads = c->n_reads; fa.r_tid = c->r_tid.p; fa.r_pos = c->r_pos.p; fa.r_rev = c->r_rev.p; fa.cig_off = c->cig_off.p; fa.cig = c->cig.p;
    fa.walked = c->walked.p; fa.local = c->local.p; fa.order = c->order.p; fa.tile_base = c->tile_base.p; fa.j0 = j0; fa.desc = c->desc.p; fa.win_hdr = c->win_hdr.p;
    fa.hdr = c->hdr.p; fa.st = tabs.st; fa.en = tabs.en;
    fa.ex_off = c->ex_off.p; fa.ex_start = c->ex_start.p; fa.ex_end = c->ex_end.p; fa.ex_flag = c->ex_flag.p; fa.info = c->info.p; fa.ref_tx = c->ref_tx.p;
    fa.tile_acc = c->tile_acc.p; fa.tile_acc_ex = c->tile_acc_ex.p; fa.redo_count = c->totals.p + TOT_REDO; fa.redo = c->redo.p;
    fa.tile_chunk = c->tile_chunk.p; fa.tile_rchunk = c->tile_rchunk.p; fa.chunk_cursor = (unsigned long long *)(c->totals.p + TOT_CHUNK_CURSOR);
    fa.acc_start = c->acc_start.p; fa.acc_end = c->acc_end.p; fa.acc_flag = c->acc_flag.p; fa.acc_rec = (AccRec *)c->acc_rec.p; fa.acc_ex_off = c->acc_ex_off.p; fa.first_read = c->first_read;
    fa.stamps = c->stamps.p; fa.p = p;
    return fa;
}

// The split of k_tile (l2r_tile.hip.h) and who may wait for whom.  Only an INEXACT tile publishes its exon count late, from the general
// instance; every other count is known since k_describe_scan.  So:
//   no inexact tile in this run (split_wait_free): nobody waits for anybody -- the split is on from the first run, the general instance
//       runs beside the EXACT one;
//   inexact tiles: a general tile may wait for one that stands ANYWHERE on the rest list (the list is not in tile order), and EXACT tiles
//       wait for general ones.  Progress then needs every listed tile resident at once and the general instance dispatched before the
//       EXACT one: the split is on only once a completed run has shown the list to fit half of what the device holds (and 4 per CU),
//       with the general instance on the main stream in front.  Until the length is known the run only MAKES the list (SPLIT_LIST): the
//       general instance takes every tile in tile order, whose look-back the dispatch order carries as it always has.
//   a list beyond 4 entries per CU (an isoform-rich annotation): the split is off, the general instance's walk over the list buys nothing.
static bool split_wait_free(const l2r_ctx *c) { return c->inexact_tiles == 0 && !(c->ablate & 256); }      // (inexact_tiles: choose_pipeline has counted them)
static uint32_t split_mode(const l2r_ctx *c)
{
    if (!c->tile_split || !c->rest_list.p) return SPLIT_OFF;
    const uint32_t fits = (uint32_t)std::min<int64_t>((int64_t)c->n_cu * 4, c->tile_resident / 2);
    if (c->facts.known) return c->facts.n_rest <= fits ? SPLIT_ON : SPLIT_OFF;
    return split_wait_free(c) ? SPLIT_ON : SPLIT_LIST;
}

// The slab and the tile pipeline's arguments (l2r_slab.hip.h).  Every launch does all of it: nothing is kept from an earlier run of the same upload.
static SlabArgs slab_args(const l2r_ctx *c, const FastArgs &fa, const CursorDir &cd, bool tile)
{
    SlabArgs sa;
    sa.g.f = fa; sa.g.cd = cd; sa.g.tid_base = c->tid_base.p; sa.g.n_tid_dir = c->n_tid_dir; sa.g.tile_total = c->tile_total.p;
    sa.tile_sbase = c->tile_sbase.p; sa.slab_row = c->slab_row.p;
    sa.dense_start = c->dense_start.p; sa.dense_end = c->dense_end.p; sa.ovf_cursor = c->ovf_cursor.p;
    sa.pl = c->s_pl.p; sa.pre_x = c->s_pre.p; sa.loc_x = c->s_loc.p; sa.cig_off32 = c->cig_off32.p; sa.tw = c->tw.p; sa.span = (TileSpan *)c->tile_span.p;
    sa.n_tiles = (uint32_t)c->n_tiles;
    sa.tw64 = (c->ablate & 4) ? nullptr : c->tw64.p;
    sa.chunk_on = (c->ablate & 32) ? 0u : 1u;          // (L2R_ABLATE bit 2: no 64-member windows, bit 5: no chunked windows)
    sa.wide_list = c->wide_list.p; sa.chunk_list = c->chunk_list.p; sa.list_cnt = c->list_cnt.p; sa.list_cnt_next = nullptr; sa.tile_flags = c->tile_flags.p;
    if (tile) { sa.list_cnt = lc_this_run(c); sa.list_cnt_next = lc_next_run(c); }
    {   const size_t sup_words = (size_t)(c->n_tiles >> LB_SUP_SHIFT) + 64;
        sa.lb_sup = c->lb_sup.p ? c->lb_sup.p + (c->lb_flip ? sup_words : 0) : nullptr;
        sa.lb_sup_next = c->lb_sup.p ? c->lb_sup.p + (c->lb_flip ? 0 : sup_words) : nullptr;
        sa.n_sup = (uint32_t)(c->n_tiles >> LB_SUP_SHIFT) + 1u; }
    sa.lb_tile = c->lb_tile.p; sa.lb_blk = c->lb_blk.p; sa.lb_err = c->totals.p + TOT_LB_ERR; sa.fb_list = c->fb_list.p; sa.exon_total = c->totals.p + TOT_EXONS; sa.tile_stat = c->tile_stat.p; sa.sup_stat = c->sup_stat.p;
    sa.sj = SjDir{CursorDir{c->sj_key.p, c->sj_cdir.p, c->sj_cbase.p, c->sj_ntid, (int32_t)c->n_sj}, c->sj_ddir.p, c->sj_dbase.p, c->sj_ntid, c->sj_row.p};
    sa.has_wide_keys = c->n_wide > 0 ? 1u : 0u;
    sa.wide_direct_on = (tile && c->wide_direct && c->tw64.p && !(c->ablate & 4)) ? 1u : 0u;
    sa.chunk_direct_on = (tile && c->chunk_direct && sa.chunk_on) ? 1u : 0u;
    sa.rest_list = c->rest_list.p;
    sa.split_on = tile ? split_mode(c) : SPLIT_OFF;
    return sa;
}

// k_probe_slab: every tile (slab pipeline), or the tiles k_tile left in slab form (`list`: fb_list, tile path).  `acc`: the tiles leave
// their accepted chunks themselves (with the accepted list wanted and no junction table to decide later)
static void launch_probe(const l2r_ctx *c, const DevParams &p, const SlabArgs &sa, bool list, bool acc, unsigned grid)
{
    with_level(p.full_level, [&](auto L) { with_flag(p.ss_dis > 0, [&](auto D) { with_flag(list, [&](auto LIST) { with_flag(acc && !list, [&](auto A) {
        // (the tiles k_tile left in slab form leave no accepted chunks themselves: they stay k_gather_accepted's -- so the
        //  instances with both are never made, half of those with a list)
        if constexpr (!(A && LIST))
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_probe_slab<L, A, D, LIST>), dim3(grid), dim3(TILE_THREADS), 0, c->stream, sa, (const TileSpan *)c->tile_span.p,
                               (const TileWin *)c->tw.p, (const uint32_t *)c->tile_xbase.p, (const uint32_t *)c->fb_list.p);
    }); }); }); });
}

// k_tile_chunk (l2r_tchunk.hip.h): a workgroup per entry of chunk_list (late = 0), or of the tiles a one-window kernel handed on late (1)
static void launch_tile_chunk(const l2r_ctx *c, const DevParams &p, const SlabArgs &sa, unsigned grid, uint32_t late, hipStream_t s)
{
    with_level(p.full_level, [&](auto L) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tile_chunk<L>), dim3(grid), dim3(TILE_THREADS), 0, s, sa, (const TileRec *)c->tile_rec.p, (const TileWin *)c->tw.p,
                           (const TileStat *)c->tile_stat.p, (const SlotRec *)c->slot_rec.p, c->tile_xbase.p, late);
    });
}

// ---- classic: pass A (exons walked into the tiles' staging, the reads ordered), a scan of the tiles' exon counts, k_classify_fast
static int launch_classic(l2r_ctx *c, hipEvent_t *ev, const DevParams &p, const FastArgs &fa, const CursorDir &cd, const SiteTabs &tabs)
{
    hipStream_t s = c->stream;
    const unsigned gt = (unsigned)(c->n_tiles ? c->n_tiles : 1);
    // sorted input: the cursor value of every read is computed on the device; unsorted input: it was replayed on the host
    with_flag(c->wide_cigar, [&](auto W) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pass_a<W>), dim3(gt), dim3(TILE_THREADS), W ? pass_a_dynamic_lds(c->reads_per_tile) : 0, s, c->n_reads, c->r_tid.p, c->r_pos.p,
                           c->cig_off.p, c->cig.p, cd, tabs, p, (c->sorted ? (const int32_t *)nullptr : (const int32_t *)c->win_start.p), c->j0.p, c->local.p, c->order.p,
                           c->tile_base.p, c->desc.p, c->totals.p + TOT_REDO, (const TxHdr *)c->hdr.p, c->win_hdr.p, (const uint32_t *)c->tile_first.p, c->walked.p);
    });
    MARK(ST_SCAN1);
    {
        ScanJobs jobs = {}; jobs.job[0] = ScanJob{c->tile_base.p, c->n_tiles, c->totals.p + TOT_EXONS}; jobs.job[1] = jobs.job[0];
        hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, s, jobs);
    }
    MARK(ST_FAST);
    // persistent grid: a few workgroups per CU walk over the tiles (l2r_kernels.hip.h)
    unsigned gp = (unsigned)std::min<int64_t>(c->n_tiles ? c->n_tiles : 1, (int64_t)c->n_cu * c->wg_per_cu);
    if (c->fast_grid > 0) gp = (unsigned)std::min<int64_t>(gp, c->fast_grid);           // L2R_FAST_GRID: tests force many tiles per workgroup
    with_level(p.full_level, [&](auto L) { with_flag(c->wide_cigar, [&](auto W) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_classify_fast<L, W>), dim3(gp), dim3(TILE_THREADS), 0, s, fa, c->n_tiles, (const TileDesc *)c->desc.p,
                           (const uint32_t *)c->tile_base.p, (const int64_t *)c->cig_off.p, (const uint8_t *)c->order.p, (const uint32_t *)c->tile_first.p);
    }); });
    return 0;
}

// ---- slab: two light kernels at full occupancy -- the walk (exons into the tiles' slabs, read-order places, descriptors), a scan of
//      the tiles' exon counts -- then the probes, which write the read-order results (l2r_slab.hip.h)
static int launch_slab(l2r_ctx *c, hipEvent_t *ev, const DevParams &p, const SlabArgs &sa)
{
    hipStream_t s = c->stream;
    const unsigned gx = 8u * (unsigned)std::max<int64_t>((c->n_tiles + 7) / 8, 1);      // (l2r_slab.hip.h xcd_tile; an empty upload still launches)
    if (c->wide_cigar)
        hipLaunchKernelGGL(k_walk_slab_long, dim3(gx), dim3(TILE_THREADS), pass_a_dynamic_lds(c->reads_per_tile), s, sa, (const TileRec *)c->tile_rec.p);
    else
        with_flag(p.min_exon < 1, [&](auto E) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_slab<E>), dim3(gx), dim3(TILE_THREADS), 0, s, sa, (const TileRec *)c->tile_rec.p); });
    MARK(ST_SCAN1);
    {   // the tiles' exon counts -> their first slots in the read-order result arrays (tile_xbase; the sum = the exon count): the
        // first workgroups of the launch, a segment each; the tiles' descriptors and windows, sixteen lanes per tile, and the lists
        // of the 64-bit-mask and the chunked kernel: the workgroups behind them (l2r_slab.hip.h)
        const DescribeScan job{c->tile_total.p, c->tile_xbase.p, c->totals.p + TOT_EXONS, c->n_tiles};
        unsigned n_scan = (unsigned)std::max<int64_t>((c->n_tiles + DESCRIBE_SEG - 1) / DESCRIBE_SEG, 1);
        if (c->n_tiles > c->seg_max) {
            // (very large shards: one workgroup scans, in a launch of its own)
            HIP_TRY(hipMemcpyAsync(c->tile_xbase.p, c->tile_total.p, (size_t)c->n_tiles * 4, hipMemcpyDeviceToDevice, s));
            ScanJobs jobs = {}; jobs.job[0] = ScanJob{c->tile_xbase.p, c->n_tiles, c->totals.p + TOT_EXONS}; jobs.job[1] = jobs.job[0];
            hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, s, jobs);
            n_scan = 0;
        }
        const unsigned gd = n_scan + (unsigned)std::max<int64_t>((c->n_tiles + DESCRIBE_TILES - 1) / DESCRIBE_TILES, 1);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_describe_scan<false>), dim3(gd), dim3(TILE_THREADS), 0, s, sa, job, (uint32_t)n_scan, (const TileRec *)nullptr);
    }
    MARK(ST_FAST);
    launch_probe(c, p, sa, false, (c->want & L2R_WANT_ACCEPTED) && c->n_sj == 0, gx);
    return 0;
}

// ---- tile: ONE kernel per tile (l2r_tile.hip.h) -- the descriptors first (spans from the upload), then walk + probes + write-out in one
//      workgroup; the instances that take the isoform-rich tiles beside it, k_probe_slab behind it for the few tiles that kept the slab
//      form (none on most inputs)
static int launch_tile(l2r_ctx *c, hipEvent_t *ev, const DevParams &p, const SlabArgs &sa, bool skip_lists)
{
    hipStream_t s = c->stream;
    const RunFacts &f = c->facts;
    const DescribeScan job{c->tile_total.p, c->tile_xbase.p, c->totals.p + TOT_EXONS, c->n_tiles};
    const unsigned gd = (unsigned)std::max<int64_t>((c->n_tiles + DESCRIBE_TILES - 1) / DESCRIBE_TILES, 1);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_describe_scan<true>), dim3(gd), dim3(TILE_THREADS), 0, s, sa, job, 0u, (const TileRec *)c->tile_rec.p);
    MARK(ST_SCAN1);
    // ---- the plan: which instances run, and where
    // the split of k_tile: the EXACT instance over every tile number (it leaves at once where k_describe_scan has not marked the tile),
    // the general instance over the rest list
    const bool split = sa.split_on == SPLIT_ON;
    const bool rest_launch = split && list_runs(c, f.n_rest);
    // the exact 64-bit-mask tiles straight from their CIGARs: k_tile's WIDE instance, a workgroup per entry of wide_list; the exact
    // tiles of the chunked kernel: k_tile_chunk, a workgroup per entry of chunk_list
    const bool wide_launch = !skip_lists && sa.wide_direct_on && list_runs(c, f.n_wide);
    const bool chunk_launch = !skip_lists && sa.chunk_direct_on && list_runs(c, f.n_chunk);
    // beside the plain instance, on streams of their own (see l2r_ctx::side); with per-stage events or L2R_CHECK one behind the other.
    // The general instance over the rest list goes beside it only in a run where nobody waits for a count; else on the main stream in
    // front of everything that may wait for its tiles, the side instances included -- they fork behind it (split_mode)
    const bool beside = c->side_on && !ev && !c->check_stages;
    const bool rest_side = rest_launch && beside && split_wait_free(c);
    const bool wide_side = wide_launch && beside, chunk_side = chunk_launch && beside;
    const bool side0 = rest_side || wide_side, side1 = chunk_side;       // side[0]: the general instance, the WIDE instance behind it; side[1]: k_tile_chunk
    const unsigned gf = fused_grid(c->n_tiles), gr = list_grid(c, f.n_rest), gwd = list_grid(c, f.n_wide), gcd = list_grid(c, f.n_chunk);
    // ---- fork
    if (rest_launch && !rest_side) launch_k_tile<false, false>(c, p, sa, gr, s);
    if (side0 || side1) HIP_TRY(hipEventRecord(c->ev_fork, s));
    // ---- launches: side[0] (its join is recorded behind whichever launch came last on it), side[1], the main stream
    if (side0) HIP_TRY(hipStreamWaitEvent(c->side[0], c->ev_fork, 0));
    if (rest_side) launch_k_tile<false, false>(c, p, sa, gr, c->side[0]);
    if (wide_launch) launch_k_tile<true, false>(c, p, sa, gwd, wide_side ? c->side[0] : s);
    if (side0) HIP_TRY(hipEventRecord(c->ev_join[0], c->side[0]));
    if (side1) {
        HIP_TRY(hipStreamWaitEvent(c->side[1], c->ev_fork, 0));
        launch_tile_chunk(c, p, sa, gcd, 0u, c->side[1]);
        HIP_TRY(hipEventRecord(c->ev_join[1], c->side[1]));
    }
    if (split) launch_k_tile<false, true>(c, p, sa, gf, s);
    else launch_k_tile<false, false>(c, p, sa, gf, s);
    MARK(ST_FAST);
    if (chunk_launch && !chunk_side) launch_tile_chunk(c, p, sa, gcd, 0u, s);
    // ---- joins
    if (side0) HIP_TRY(hipStreamWaitEvent(s, c->ev_join[0], 0));
    if (side1) HIP_TRY(hipStreamWaitEvent(s, c->ev_join[1], 0));
    // k_probe_slab over the tiles k_tile left in slab form
    const unsigned gl = (unsigned)std::min<int64_t>(c->n_tiles ? c->n_tiles : 1, (int64_t)c->n_cu * 2);
    if (!skip_lists && list_runs(c, f.n_fb)) launch_probe(c, p, sa, true, false, gl);
    return 0;
}

// ---- slab and tile: the list-driven kernels behind the probes (none has anything to do on most inputs: the grid finds an empty list and leaves)
static void launch_lists(l2r_ctx *c, const DevParams &p, const SlabArgs &sa, bool tile, bool skip_lists)
{
    if (skip_lists) return;
    hipStream_t s = c->stream;
    const RunFacts &f = c->facts;       // (what a completed run of the tile path has shown; the slab pipeline launches all three)
    if (!tile || list_runs(c, f.n_wide_rest)) {
        // the tiles with 33 .. 63 window members
        const WideArgs wa{c->tw64.p};
        const unsigned gw = (unsigned)std::min<int64_t>(c->n_tiles ? c->n_tiles : 1, (int64_t)c->n_cu * 5);
        with_level(p.full_level, [&](auto L) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_probe_slab_wide<L>), dim3(gw), dim3(TILE_THREADS), 0, s, sa, wa, (const uint32_t *)c->tile_first.p, (const int32_t *)c->r_pos.p,
                               (const uint32_t *)c->tile_sbase.p, (const TileWin *)c->tw.p, (const uint32_t *)c->tile_xbase.p, (const TileStat *)(tile ? c->tile_stat.p : nullptr));
        });
    }
    if (sa.chunk_direct_on && list_runs(c, f.n_late)) {
        // the tiles a one-window kernel handed on late (a key in several entries): k_tile_chunk once more, over that list
        // (every entry needs its workgroup: k_probe_slab_chunked skips what this launch takes)
        launch_tile_chunk(c, p, sa, list_grid(c, f.n_late), 1u, s);
    }
    if (sa.chunk_on && (!tile || list_runs(c, f.chunk_rest))) {
        // the tiles without a window record, or with a dictionary key in several entries
        const unsigned gc = (unsigned)std::min<int64_t>(c->n_tiles ? c->n_tiles : 1, (int64_t)c->n_cu * 4);
        with_level(p.full_level, [&](auto L) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_probe_slab_chunked<L>), dim3(gc), dim3(TILE_THREADS), 0, s, sa, (const uint32_t *)c->tile_first.p, (const int32_t *)c->r_pos.p,
                               (const uint32_t *)c->tile_sbase.p, (const TileWin *)c->tw.p, (const uint32_t *)c->tile_xbase.p);
        });
    }
    // (accepted list: k_describe_scan marks every tile CHUNK_DEFERRED, k_probe_slab<., true> takes that back for the tiles whose
    //  chunk it has written itself; k_count_accepted / k_gather_accepted place the rest)
}

// ---- every pipeline: the generic kernel (reads the others handed on), the junction check, the accepted list's count / scan / gather
static int launch_tail(l2r_ctx *c, hipEvent_t *ev, const DevParams &p, const CursorDir &cd, const int32_t *j0)
{
    hipStream_t s = c->stream;
    const bool tile = c->pipe == Pipeline::tile;
    const unsigned gt = (unsigned)(c->n_tiles ? c->n_tiles : 1), g256 = (unsigned)(c->n_tiles256 ? c->n_tiles256 : 1);
    MARK(ST_GENERIC);
    // (one-kernel tile path: a completed run of the same inputs and parameters has left nothing on the redo list -- no read is left for
    //  the generic kernel, and the list counters need no launch for their clearing, they take turns -- and nothing to the list-driven
    //  kernels or no junction table: no read is left for the junction check either, k_tile has checked every read whose verdict it made)
    // (L2R_ABLATE bits 9 / 10 take the junction check out of k_tile: with a table every candidate is then k_validate_sj's, in every run)
    const bool sj_left = c->n_sj > 0 && (c->ablate & (512 | 1024)) != 0;
    const bool nothing_left = tile && c->facts.known && c->facts.redo_empty && (lists_empty(c->facts) || c->n_sj == 0) && !c->env_launch_all && !sj_left;
    end_of_run(c, tile);
    if (!nothing_left) {
        const unsigned gg = (unsigned)std::min<int64_t>(c->n_tiles ? c->n_tiles * 4 : 1, 4096);      // one wave per listed read, grid-stride
        hipLaunchKernelGGL(k_classify_generic, dim3(gg), dim3(TILE_THREADS), 0, s, c->totals.p + TOT_REDO, c->redo.p, c->r_tid.p, c->r_rev.p,
                           (c->pipe != Pipeline::classic ? (const int32_t *)nullptr : j0),
                           c->hdr.p, c->anno_ex.p, p, c->ex_off.p, c->ex_start.p, c->ex_end.p, c->ex_flag.p, c->info.p, c->ref_tx.p,
                           c->tile_acc.p, c->tile_acc_ex.p, (const uint32_t *)c->tile_first.p, (int)c->n_tiles, cd);
    }
    MARK(ST_SJ);
    // (one-kernel tile path: k_tile has checked every read whose verdict it made; with nothing on the redo list and nothing left to the
    //  list-driven kernels -- seen by a completed run of the same inputs and parameters -- no read is left for this launch)
    if (c->n_sj > 0 && !nothing_left) {
        if (!c->sorted) { int rc = prepare_unsorted_sj_cursor(c); if (rc) return rc; }
        hipLaunchKernelGGL(k_validate_sj, dim3(g256), dim3(TILE_THREADS), 0, s, c->n_reads, c->r_tid.p, c->ex_off.p, c->ex_start.p, c->ex_end.p, c->ex_flag.p,
                           c->sj_key.p, (c->sorted ? (const int32_t *)nullptr : c->sj_cursor.p), c->sj_tid.p, c->sj_don.p, c->sj_acc.p,
                           c->sj_uniq.p, c->sj_multi.p, p, c->info.p,
                           SjDir{CursorDir{c->sj_key.p, c->sj_cdir.p, c->sj_cbase.p, c->sj_ntid, (int32_t)c->n_sj}, c->sj_ddir.p, c->sj_dbase.p, c->sj_ntid, c->sj_row.p});
    }
    if ((c->n_sj > 0 || c->pipe != Pipeline::classic) && (c->want & L2R_WANT_ACCEPTED)) {
        // acceptance is decided by the junction check (and the slab pipeline counts nothing itself): count per tile
        hipLaunchKernelGGL(k_count_accepted, dim3((gt + 3u) / 4u), dim3(TILE_THREADS), 0, s, (const uint32_t *)c->tile_first.p, c->info.p, (const uint32_t *)c->tile_chunk.p, c->tile_acc.p, c->tile_acc_ex.p, (uint32_t)c->n_tiles);
    }
    MARK(ST_SCAN2);
    if (c->want & L2R_WANT_ACCEPTED) {
        // the deferred tiles' counts -> their places behind the fused chunks (tile_acc_at / tile_acc_ex_at; the sums = totals[TOT_ACCEPTED], [TOT_ACCEPTED_EXONS])
        if (c->n_tiles <= c->seg_max) {
            const unsigned n_seg = (unsigned)std::max<int64_t>((c->n_tiles + SEG_COUNT - 1) / SEG_COUNT, 1);
            hipLaunchKernelGGL(k_scan_segments, dim3(2u * n_seg), dim3(TILE_THREADS), 0, s, SegScan{c->tile_acc.p, c->tile_acc_at.p, c->totals.p + TOT_ACCEPTED, c->n_tiles},
                               SegScan{c->tile_acc_ex.p, c->tile_acc_ex_at.p, c->totals.p + TOT_ACCEPTED_EXONS, c->n_tiles}, (uint32_t)n_seg);
        } else {
            HIP_TRY(hipMemcpyAsync(c->tile_acc_at.p, c->tile_acc.p, (size_t)c->n_tiles * 4, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(c->tile_acc_ex_at.p, c->tile_acc_ex.p, (size_t)c->n_tiles * 4, hipMemcpyDeviceToDevice, s));
            ScanJobs jobs = {}; jobs.job[0] = ScanJob{c->tile_acc_at.p, c->n_tiles, c->totals.p + TOT_ACCEPTED}; jobs.job[1] = ScanJob{c->tile_acc_ex_at.p, c->n_tiles, c->totals.p + TOT_ACCEPTED_EXONS};
            hipLaunchKernelGGL(k_scan_u32, dim3(2), dim3(1024), 0, s, jobs);
        }
    }
    MARK(ST_GATHER);
    if (c->want & L2R_WANT_ACCEPTED)
        hipLaunchKernelGGL(k_gather_accepted, dim3((gt + GATHER_TILES - 1) / GATHER_TILES), dim3(TILE_THREADS), 0, s, (const uint32_t *)c->tile_first.p, c->first_read, c->info.p, c->ref_tx.p, c->ex_off.p,
                           c->ex_start.p, c->ex_end.p, c->ex_flag.p, c->tile_acc_at.p, c->tile_acc_ex_at.p, c->tile_chunk.p, c->tile_rchunk.p, c->totals.p + TOT_CHUNK_CURSOR,
                           c->acc_rec.p, c->acc_ex_off.p, c->acc_start.p, c->acc_end.p, c->acc_flag.p, (uint32_t)c->n_tiles);
    MARK(ST_N);
    return 0;
}

// One run: the front of the pipeline choose_pipeline picks, the list-driven kernels of the slab and the tile pipeline, the common tail
static int launch_all(l2r_ctx *c, hipEvent_t *ev /* ST_N + 1 events or null */)
{
    const DevParams p = dev_params(c);
    MARK(ST_PASS_A);
    c->pipe = choose_pipeline(c, p);
    const int32_t *j0 = c->sorted ? (const int32_t *)c->j0.p : (const int32_t *)c->win_start.p;
    const CursorDir cd{c->anno_key.p, c->key_dir.p, c->kb_base.p, c->n_tid_key, (int32_t)c->n_tx};
    const SiteTabs tabs{{c->sk_st.p, c->sd_st.p, c->sr_st.p}, {c->sk_en.p, c->sd_en.p, nullptr}, c->tid_base.p, c->n_tid_dir};
    const FastArgs fa = fast_args(c, p, tabs, j0);
    int rc = 0;
    if (c->pipe == Pipeline::classic) rc = launch_classic(c, ev, p, fa, cd, tabs);
    else {
        const bool tile = c->pipe == Pipeline::tile;
        // (the list counters are whatever a slab run left: cleared in front of the first tile run behind one)
        if (tile && !c->prev_run_tile) HIP_TRY(lc_reset(c));
        const SlabArgs sa = slab_args(c, fa, cd, tile);
        // (the three list-driven kernels behind k_tile: not launched once a completed run of the same inputs and parameters has shown
        //  their lists empty -- what ends up on them does not depend on anything else)
        const bool skip_lists = tile && c->facts.known && lists_empty(c->facts) && !c->env_launch_all;
        rc = tile ? launch_tile(c, ev, p, sa, skip_lists) : launch_slab(c, ev, p, sa);
        if (!rc) launch_lists(c, p, sa, tile, skip_lists);
    }
    if (!rc) rc = launch_tail(c, ev, p, cd, j0);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return 0;
}
#undef MARK

/* diagnostics: L2R_STAMPS=1 makes k_classify_fast accumulate per-phase cycles; this prints and clears them */
int l2r_debug_stamps(l2r_ctx *c, unsigned long long *out, int n)
{
    if (!c || !out) return fail(-1, "[l2r_debug_stamps] null argument");
    if (!c->stamps.p) { for (int i = 0; i < n; ++i) out[i] = 0; return 0; }
    std::vector<unsigned long long> h(1024 * 8 + 16);
    HIP_TRY(hipMemcpyAsync(h.data(), c->stamps.p, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(c->stamps.p, 0, h.size() * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) out[i] = 0;
    for (size_t k = 0; k < 1024 * 8; ++k) if ((int)(k & 7) < n) out[k & 7] += h[k];
    for (int i = 8; i < n && i < 16; ++i) out[i] = h[1024 * 8 + (i - 8)];      /* redo reasons: not fast, not in LDS, wide, other tid, not sane, window/compact */
    return 0;
}

/* diagnostics (L2R_STAMPS=1, one-kernel tile path): per tile four words -- the 100 MHz clock at its start << 3 | its XCD, the clock at the
   publication of its exon count, at the begin and at the end of its wait for the counts of the tiles in front */
int l2r_debug_tile_times(l2r_ctx *c, uint32_t *out, int64_t n_tiles)
{
    if (!c || !out) return fail(-1, "[l2r_debug_tile_times] null argument");
    if (c->pipe != Pipeline::tile || !c->ran || n_tiles > c->n_tiles) return fail(-1, "[l2r_debug_tile_times] no run of the one-kernel tile path to report");
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t *src[4] = {c->tile_total.p, c->tile_acc.p, c->tile_acc_ex.p, c->tile_flags.p};
    std::vector<uint32_t> h((size_t)n_tiles);
    for (int k = 0; k < 4; ++k) {
        HIP_TRY(hipMemcpyAsync(h.data(), src[k], (size_t)n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int64_t i = 0; i < n_tiles; ++i) out[4 * i + k] = h[(size_t)i];
    }
    return 0;
}

/* diagnostics: [0] reads the last run sent to the generic kernel, [1] dictionary entries flagged wide,
   [2] compact transcripts, [3] tiles, [4..11] tiles by the reason they are not fast, [12] tiles of k_probe_slab_wide */
int l2r_debug_counters(l2r_ctx *c, long long *out, int n)
{
    if (!c || !out || n < 4) return fail(-1, "[l2r_debug_counters] bad argument");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t redo = 0;
    if (c->totals.p) { HIP_TRY(hipMemcpyAsync(&redo, c->totals.p + TOT_REDO, 4, hipMemcpyDeviceToHost, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); }
    out[0] = redo; out[1] = c->n_wide; out[2] = c->n_compact; out[3] = c->n_tiles;
    if (n >= 12) for (int k = 0; k < 8; ++k) out[4 + k] = 0;
    if (n >= 13) out[12] = 0;
    for (int k = 16; k < std::min(n, 29); ++k) out[k] = 0;         // (the descriptor words below: 0 where no run left descriptors)
    if (n >= 14) out[13] = c->n_lb_fallback;              // runs done again on the slab pipeline because k_tile's look-back starved
    if (n >= 16) {                                        // one-kernel tile path, last run: entries of chunk_list k_tile_chunk declined, tiles handed to the chunked kernel late
        out[14] = 0; out[15] = 0;
        if (c->pipe == Pipeline::tile && c->ran && c->list_cnt.p) {
            uint32_t lc[LC_WORDS];
            HIP_TRY(hipMemcpyAsync(lc, lc_last_run(c), sizeof lc, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            out[14] = lc[LC_DECLINED]; out[15] = lc[LC_LATE];
            if (n >= 29) out[28] = lc[LC_REST];             // entries of the rest list: the tiles k_tile's general instance ran over beside the EXACT one (0: split off)
        }
    }
    if (n >= 12 && c->pipe != Pipeline::classic && c->ran && c->tw.p && c->n_tiles > 0) {     // slab pipeline: the descriptors k_walk_slab made (flags as the probe kernels left them)
        std::vector<TileWin> w((size_t)c->n_tiles);
        HIP_TRY(hipMemcpyAsync(w.data(), c->tw.p, w.size() * sizeof(TileWin), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (const TileWin &t : w) {
            if (n >= 27) {                                  // largest dictionary slices of any tile, tiles k_tile_chunk took (k_describe_scan<true>)
                out[24] = std::max<long long>(out[24], t.d.st_nk); out[25] = std::max<long long>(out[25], t.d.en_nk);
                if (t.d.flags & TD_CDIRECT) out[26]++;
                if (n >= 29 && c->pipe == Pipeline::tile && (t.d.flags & TD_XDIRECT)) out[27]++;      // tiles k_tile's EXACT instance took
            }
            if (n >= 24) {                                  // tiles of the chunked kernel by the END entries of their dictionary slices (<= 256, 512, 768, 1024, more), START entries beyond 128 / 256, all of them
                const uint32_t why = (t.d.flags >> 8) & 7u;
                if ((t.d.flags & TD_CHUNK) || (!(t.d.flags & (TD_FAST | TD_WIDE)) && (why == 4u || why == 3u))) {
                    out[16 + (t.d.en_nk <= 256u ? 0 : t.d.en_nk <= 512u ? 1 : t.d.en_nk <= 768u ? 2 : t.d.en_nk <= 1024u ? 3 : 4)]++;
                    if (t.d.st_nk > 128u) out[21]++;
                    if (t.d.st_nk > 256u) out[22]++;
                    out[23]++;
                }
            }
            out[4 + ((t.d.flags >> 8) & 7u)]++;
            if (n >= 13 && (t.d.flags & TD_WIDE) && !(t.d.flags & TD_CHUNK)) out[12]++;     // out[12]: tiles k_probe_slab_wide classified (33 .. 63 window members)
        }
    } else if (n >= 12 && c->pipe == Pipeline::classic && c->desc.p && c->n_tiles > 0) {     // out[4 + k]: tiles that are not fast for reason k (k_pass_a), k = 0: fast
        std::vector<TileDesc> d((size_t)c->n_tiles);
        HIP_TRY(hipMemcpyAsync(d.data(), c->desc.p, d.size() * sizeof(TileDesc), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (const TileDesc &t : d) {
            out[4 + ((t.flags >> 8) & 7u)]++;
            if (n >= 27) { out[24] = std::max<long long>(out[24], t.st_nk); out[25] = std::max<long long>(out[25], t.en_nk); }
        }
    }
    return 0;
}

/* Which kernel(s) stand behind stage_ms[stage] of l2r_timing for the inputs and parameters now set (the pipeline is
   chosen per launch: slab for coordinate-sorted records with short CIGARs, classic otherwise). */
const char *l2r_stage_kernel(l2r_ctx *c, int stage)
{
    if (!c || stage < 0 || stage >= L2R_N_STAGES) return "";
    // (the first word is the kernel's name as a profile lists it; both scans are launches of k_scan_u32)
    static const char *const classic[L2R_N_STAGES] = {"k_pass_a", "k_scan_u32 (tile sums)", "k_classify_fast", "k_classify_generic",
                                                      "k_validate_sj", "k_scan_accepted (k_scan_u32 of the accepted counts)", "k_gather_accepted", ""};
    if (stage >= 3 || c->pipe == Pipeline::classic) return classic[stage];
    if (c->pipe == Pipeline::tile) return stage == 0 ? "k_describe_scan (tile descriptors + tile lists; first kernel of the run)" : stage == 1 ? "k_tile (walk + probes + write-out, one workgroup per tile)" : "k_probe_slab (tiles k_tile left in slab form) (+ k_tile_chunk + k_probe_slab_wide + k_probe_slab_chunked)";
    return stage == 0 ? (c->wide_cigar ? "k_walk_slab_long" : "k_walk_slab") : stage == 1 ? "k_describe_scan (tile descriptors + scan of the exon counts + tile lists)" : "k_probe_slab (+ k_probe_slab_wide + k_probe_slab_chunked)";
}

int l2r_run(l2r_ctx *c)
{
    if (!c) return fail(-1, "[l2r_run] null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = prepare_unsorted_windows(c);
    if (rc) return rc;
    if ((rc = launch_all(c, nullptr))) return rc;
    c->ran = true; c->totals_valid = false;
    return 0;
}

// What a completed run of the tile path left on the lists of the kernels behind k_tile, and on the redo list: c->facts
static int fetch_run_facts(l2r_ctx *c)
{
    uint32_t lc[LC_WORDS];
    HIP_TRY(hipMemcpyAsync(lc, lc_last_run(c), sizeof lc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t redo_n = 1u;
    HIP_TRY(hipMemcpyAsync(&redo_n, c->totals.p + TOT_REDO, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    RunFacts &f = c->facts;
    f.n_wide = lc[LC_WIDE]; f.n_chunk = lc[LC_CHUNK]; f.n_rest = lc[LC_REST]; f.n_late = lc[LC_LATE];
    f.n_fb = lc[LC_FB]; f.n_wide_rest = lc[LC_WIDE_REST];
    const bool tchunk = c->chunk_direct && !(c->ablate & 32);
    f.chunk_rest = tchunk ? (unsigned long long)lc[LC_DECLINED] + lc[LC_DECLINED_LATE] : (unsigned long long)lc[LC_LATE] + lc[LC_CHUNK];
    f.redo_empty = redo_n == 0u;
    f.known = true;
    return 0;
}

int l2r_sync(l2r_ctx *c)
{
    if (!c) return fail(-1, "[l2r_sync] null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->ran && c->pipe == Pipeline::tile && c->totals.p) {
        // a tile of k_tile waited in vain for the exon counts in front of it (its poll limit ended every wait: the run is complete but its
        // result slots are not to be trusted): the SAME resident upload once more on the slab pipeline, which has no such wait -- and no
        // later run of this context takes the tile path again (the cause is the device's occupancy, not this input)
        uint32_t lb = 0u;
        HIP_TRY(hipMemcpyAsync(&lb, c->totals.p + TOT_LB_ERR, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (lb != 0u) {
            c->tile_starved = true; c->n_lb_fallback++;
            forget_list_state(c); c->totals_valid = false;
            int rc = launch_all(c, nullptr);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            snprintf(g_err, sizeof g_err, "[l2r_sync] note: k_tile's look-back starved; the run was done again on the slab pipeline (this context keeps to it)");
        }
    }
    if (c->ran && c->pipe == Pipeline::tile && !c->facts.known && c->list_cnt.p) return fetch_run_facts(c);
    return 0;
}

static int fetch_totals(l2r_ctx *c)
{
    if (!c->ran) return fail(-1, "no completed run on this context");
    if (c->totals_valid) return 0;
    uint32_t dev[TOT_WORDS];
    HIP_TRY(hipMemcpyAsync(dev, c->totals.p, sizeof dev, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // accepted exons = the chunks the classification kernel placed itself (cursor) + the ones k_gather_accepted placed
    if (c->pipe == Pipeline::tile && dev[TOT_LB_ERR] != 0u) return fail(-2, "[l2r] k_tile: a tile waited in vain for the exon counts of the tiles in front of it and l2r_sync was not called behind the run (it does the run again on the slab pipeline)");
    c->h_totals[0] = dev[TOT_EXONS]; c->h_totals[1] = dev[TOT_ACCEPTED] + dev[TOT_CHUNK_CURSOR + 1]; c->h_totals[2] = dev[TOT_ACCEPTED_EXONS] + dev[TOT_CHUNK_CURSOR];
    if (!(c->want & L2R_WANT_ACCEPTED)) c->h_totals[1] = c->h_totals[2] = 0;
    c->totals_valid = true;
    return 0;
}

int l2r_run_timed(l2r_ctx *c, int iters, l2r_timing *out)
{
    if (!c || !out || iters <= 0) return fail(-1, "[l2r_run_timed] bad argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = prepare_unsorted_windows(c);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    // every event lives in one holder that releases them on every way out of this function
    struct Events {
        hipEvent_t e[ST_N + 3]; int n = 0;
        ~Events() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(e[i]); }
    } evs;
    for (int i = 0; i < ST_N + 3; ++i) { HIP_TRY(hipEventCreate(&evs.e[i])); evs.n = i + 1; }
    hipEvent_t t0 = evs.e[ST_N + 1], t1 = evs.e[ST_N + 2], *ev = evs.e;
    // pass A: whole pipeline, back to back
    HIP_TRY(hipEventRecord(t0, c->stream));
    for (int it = 0; it < iters; ++it) { rc = launch_all(c, nullptr); if (rc) return rc; }
    HIP_TRY(hipEventRecord(t1, c->stream));
    HIP_TRY(hipEventSynchronize(t1));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, t0, t1));
    out->total_ms = ms / (float)iters;
    // pass B: per-stage events
    for (int it = 0; it < iters; ++it) {
        rc = launch_all(c, ev); if (rc) return rc;
        HIP_TRY(hipEventSynchronize(ev[ST_N]));
        for (int i = 0; i < ST_N; ++i) { float d = 0; HIP_TRY(hipEventElapsedTime(&d, ev[i], ev[i + 1])); out->stage_ms[i] += d / (float)iters; }
    }
    out->iters = iters;
    c->ran = true; c->totals_valid = false;
    return 0;
}

int l2r_result_sizes(l2r_ctx *c, int64_t *n_reads, int64_t *n_exons, int64_t *n_acc, int64_t *n_acc_ex)
{
    if (!c) return fail(-1, "[l2r_result_sizes] null context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = fetch_totals(c);
    if (rc) return rc;
    if (n_reads) *n_reads = c->n_reads;
    if (n_exons) *n_exons = c->h_totals[0];
    if (n_acc) *n_acc = c->h_totals[1];
    if (n_acc_ex) *n_acc_ex = c->h_totals[2];
    return 0;
}

int l2r_download(l2r_ctx *c, l2r_result *res)
{
    if (!c || !res) return fail(-1, "[l2r_download] null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = fetch_totals(c);
    if (rc) return rc;
    const int64_t N = c->n_reads, X = c->h_totals[0];
    if (res->n_reads < N || res->ex_cap < X) return fail(-3, "[l2r_download] buffers too small: need %lld reads, %lld exons", (long long)N, (long long)X);
    // both pipelines leave the results in read order: exon k of read i at ex_off[i] + k, offsets = the running sum of the exon counts
    std::vector<uint32_t> off((size_t)N);
    if (N) {
        HIP_TRY(hipMemcpyAsync(off.data(), c->ex_off.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(res->info, c->info.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(res->ref_tx, c->ref_tx.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (X) {
        HIP_TRY(hipMemcpyAsync(res->ex_start, c->ex_start.p, (size_t)X * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(res->ex_end, c->ex_end.p, (size_t)X * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(res->ex_flag, c->ex_flag.p, (size_t)X, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    {
        int64_t at = 0;
        for (int64_t i = 0; i < N; ++i) {
            if ((int64_t)off[(size_t)i] != at) return fail(-5, "[l2r_download] exon offsets are not the running sum of the exon counts at read %lld (%u, expected %lld)", (long long)i, off[(size_t)i], (long long)at);
            res->ex_off[i] = at; at += (int64_t)(res->info[i] >> 8);
        }
        if (at != X) return fail(-5, "[l2r_download] exon counts (%lld) do not add up to the exon total (%lld)", (long long)at, (long long)X);
    }
    res->ex_off[N] = X;
    res->n_reads = N; res->n_exons = X;
    return 0;
}

// The accepted list of one engine as it lies in HBM (per-tile chunks in the order they were handed out, see k_gather_accepted) -> read
// order, appended to `a` at record at_r / exon at: the chunks are told apart by the first-record slots the tiles left (starts), each is
// in read order inside, and the exons are laid out record by record, so that ex_off is the running sum.
static int order_accepted(const AccRec *rec, const uint32_t *off, std::vector<uint32_t> starts, const int32_t *xs, const int32_t *xe, const uint8_t *xf,
                          int64_t M, int64_t X, l2r_accepted *a, int64_t &at_r, int64_t &at)
{
    if (!M) return 0;
    const int64_t r_end = at_r + M, x_base = at;
    // (a tile without accepted reads leaves the slot of some other chunk, 0 or M: duplicates and M drop out)
    starts.push_back(0u);
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    while (!starts.empty() && (int64_t)starts.back() >= M) starts.pop_back();
    std::vector<std::pair<uint64_t, std::pair<uint32_t, uint32_t>>> chunks;        // first read index -> [from, to)
    for (size_t k = 0; k < starts.size(); ++k) {
        const uint32_t from = starts[k], to = k + 1 < starts.size() ? starts[k + 1] : (uint32_t)M;
        chunks.push_back({((uint64_t)rec[from].read_hi << 32) | rec[from].read_lo, {from, to}});
    }
    std::sort(chunks.begin(), chunks.end());
    for (const auto &ch : chunks) {
        for (uint32_t i = ch.second.first; i < ch.second.second; ++i) {
            const int64_t n = (int64_t)(rec[i].info >> 8), from = off[i];
            if (from + n > X || at - x_base + n > X || at_r >= r_end) return fail(-5, "[l2r_download_accepted] inconsistent accepted list");
            memcpy(&a->rec[at_r], &rec[i], sizeof(AccRec));
            a->ex_off[at_r] = at;
            memcpy(a->ex_start + at, xs + from, (size_t)n * 4);
            memcpy(a->ex_end + at, xe + from, (size_t)n * 4);
            memcpy(a->ex_flag + at, xf + from, (size_t)n);
            at += n; ++at_r;
        }
    }
    if (at_r != r_end) return fail(-5, "[l2r_download_accepted] inconsistent accepted list (%lld of %lld records)", (long long)(at_r - (r_end - M)), (long long)M);
    return 0;
}

int l2r_download_accepted(l2r_ctx *c, l2r_accepted *a)
{
    if (!c || !a) return fail(-1, "[l2r_download_accepted] null argument");
    HIP_TRY(hipSetDevice(c->device));
    if (!(c->want & L2R_WANT_ACCEPTED)) return fail(-1, "[l2r_download_accepted] the accepted list was not requested (l2r_set_outputs)");
    int rc = fetch_totals(c);
    if (rc) return rc;
    const int64_t M = c->h_totals[1], X = c->h_totals[2];
    if (a->n_reads < M || a->ex_cap < X) return fail(-3, "[l2r_download_accepted] buffers too small: need %lld records, %lld exons", (long long)M, (long long)X);
    // On the device the list is a sequence of per-tile chunks in the order they were handed out (see k_gather_accepted):
    // the chunks are put into read order here (each is in read order inside; they are told apart by the first-record
    // slots the tiles left in tile_rchunk) and the exons laid out record by record, so that ex_off is the running sum.
    std::vector<AccRec> rec((size_t)M);
    std::vector<uint32_t> off((size_t)M), starts((size_t)c->n_tiles);
    std::vector<int32_t> xs((size_t)X), xe((size_t)X);
    std::vector<uint8_t> xf((size_t)X);
    if (M) {
        HIP_TRY(hipMemcpyAsync(rec.data(), c->acc_rec.p, (size_t)M * sizeof(AccRec), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(off.data(), c->acc_ex_off.p, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(starts.data(), c->tile_rchunk.p, (size_t)c->n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (X) {
        HIP_TRY(hipMemcpyAsync(xs.data(), c->acc_start.p, (size_t)X * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(xe.data(), c->acc_end.p, (size_t)X * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(xf.data(), c->acc_flag.p, (size_t)X, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t at_r = 0, at = 0;
    rc = order_accepted(rec.data(), off.data(), starts, xs.data(), xe.data(), xf.data(), M, X, a, at_r, at);
    if (rc) return rc;
    a->ex_off[M] = at;
    a->n_reads = M; a->n_exons = X;
    return 0;
}

int l2r_device_view_get(l2r_ctx *c, l2r_device_view *v)
{
    if (!c || !v) return fail(-1, "[l2r_device_view_get] null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = fetch_totals(c);
    if (rc) return rc;
    v->n_reads = c->n_reads; v->n_exons = c->h_totals[0]; v->n_accepted = c->h_totals[1]; v->n_accepted_exons = c->h_totals[2];
    v->ex_off = nullptr; v->ex_start = nullptr; v->ex_end = nullptr; v->ex_flag = nullptr;
    if (c->want & L2R_WANT_RESULTS) { v->ex_off = c->ex_off.p; v->ex_start = c->ex_start.p; v->ex_end = c->ex_end.p; v->ex_flag = c->ex_flag.p; }      // (read order, as the kernels left them; fetch_totals has waited for the stream)
    v->info = c->info.p; v->ref_tx = c->ref_tx.p;
    v->acc_rec = (const l2r_accepted_read *)c->acc_rec.p; v->acc_ex_off = c->acc_ex_off.p;
    v->acc_ex_start = c->acc_start.p; v->acc_ex_end = c->acc_end.p; v->acc_ex_flag = c->acc_flag.p;
    return 0;
}

int l2r_classify(l2r_ctx *c, const l2r_reads *reads, l2r_result *res)
{
    if (!c) return fail(-1, "[l2r_classify] null context");
    // ONE run follows this upload: by total GPU time the two-kernel (slab) pipeline wins that case -- measured on 10 M reads 0.62 ms against
    // tile index + first run of the one-kernel path 0.68 ms (0.80 ms where the engine has to walk the CIGARs for the index itself); the
    // one-kernel path pays off from the second run of an upload on (0.50 ms a run).  So this upload makes no tile index and its run takes
    // the slab pipeline (L2R_PIPELINE=tile or L2R_TILE_ANYWAY=1: index + tile path all the same).
    const bool was = c->one_shot_upload;
    c->one_shot_upload = true;
    int rc = l2r_upload_reads(c, reads);
    c->one_shot_upload = was;
    if (rc) return rc;
    if ((rc = l2r_run(c))) return rc;
    if ((rc = l2r_sync(c))) return rc;
    return l2r_download(c, res);
}

// ---------------------------------------------------------------------------------------------- filter
// slots of l2r_fusion_stats
enum { FUS_WAVE = 0, FUS_K_SEG, FUS_K_SELECT, FUS_K_FILTER_SCORE, FUS_K_FILTER_SELECT, FUS_N };

// In front of the launch of a `filter` / `fusion` entry point: its word of l2r_fusion_stats starts at 0 (the timer adds), and the timer is
// armed: with L2R_FUSION_TIMING=1 (tools/bench_fusion.py) the launch is bracketed by events and waited for
static int fusion_begin(l2r_ctx *c, int slot)
{
    c->fusion_stats[slot] = 0;
    return c->fusion_clk.begin(env_on("L2R_FUSION_TIMING"), false);
}

int l2r_filter_score(l2r_ctx *c, const l2r_filter_records *r, const l2r_filter_params *prm, const l2r_filter_spans *rm,
                     uint8_t *drop, int32_t *score, int32_t *intron_n)
{
    {   std::string msg;
        if (filter_score_check(c, r, prm, rm, drop, score, intron_n, msg)) return fail(-1, "%s", msg.c_str()); }
    const size_t N = (size_t)r->n;
    if (N == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // the -r transcripts a record of every chromosome can meet (l2r_filterplan.hip.h), on the host
    FilterSpanTable tab;
    filter_spans_build(rm, tab);
    const std::vector<int64_t> &off = tab.off; const std::vector<int32_t> &st = tab.start, &pe = tab.pmax_end;
    const int32_t n_tid = tab.n_tid;
    DevBuf<uint16_t> d_flag; DevBuf<int32_t> d_tid, d_pos, d_lq, d_nm, d_score, d_in, d_st, d_pe; DevBuf<int64_t> d_off, d_soff; DevBuf<uint32_t> d_cig; DevBuf<uint8_t> d_drop;
    int rc = 0;
    if ((rc = to_dev(c, d_flag, r->flag, N)) || (rc = to_dev(c, d_tid, r->tid, N)) || (rc = to_dev(c, d_pos, r->pos, N)) || (rc = to_dev(c, d_lq, r->l_qseq, N)) ||
        (rc = to_dev(c, d_nm, r->nm, N)) || (rc = to_dev(c, d_off, r->cig_off, N + 1)) || (rc = to_dev(c, d_cig, r->cig, (size_t)r->n_cigar)) ||
        (rc = to_dev(c, d_soff, off.data(), off.size())) || (rc = to_dev(c, d_st, st.data(), st.size())) || (rc = to_dev(c, d_pe, pe.data(), pe.size())) ||
        d_drop.ensure(N) || d_score.ensure(N) || d_in.ensure(N)) { rc = rc ? rc : -2; }
    if (!rc && !(rc = fusion_begin(c, FUS_K_FILTER_SCORE))) {
        const FilterPrm fp{prm->cov_rate, prm->map_qual, prm->sec_rat, prm->min_intron_n};
        const FilterSpans sp{d_soff.p, d_st.p, d_pe.p, n_tid};
        rc = c->fusion_clk.launch(c, &c->fusion_stats[FUS_K_FILTER_SCORE], [&] {
            hipLaunchKernelGGL(k_filter_score, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (int64_t)N, (const uint16_t *)d_flag.p, (const int32_t *)d_tid.p,
                               (const int32_t *)d_pos.p, (const int32_t *)d_lq.p, (const int32_t *)d_nm.p, (const int64_t *)d_off.p, (const uint32_t *)d_cig.p, fp, sp,
                               d_drop.p, d_score.p, d_in.p);
        });
    }
    return download_all(c, rc, {{drop, d_drop.p, N}, {score, d_score.p, N * 4}, {intron_n, d_in.p, N * 4}}, "l2r_filter_score");
}

int l2r_filter_select(l2r_ctx *c, int64_t n_groups, const int64_t *group_off, const int32_t *score, const int32_t *intron_n,
                      const l2r_filter_params *prm, int64_t *winner)
{
    {   std::string msg;
        if (filter_select_check(c, n_groups, group_off, score, intron_n, prm, winner, msg)) return fail(-1, "%s", msg.c_str()); }
    if (n_groups == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t G = (size_t)n_groups, R = (size_t)group_off[G];
    DevBuf<int64_t> d_off, d_win; DevBuf<int32_t> d_score, d_in;
    int rc = 0;
    if ((rc = to_dev(c, d_off, group_off, G + 1)) || (rc = to_dev(c, d_score, score, R)) || (rc = to_dev(c, d_in, intron_n, R)) || d_win.ensure(G)) rc = rc ? rc : -2;
    if (!rc && !(rc = fusion_begin(c, FUS_K_FILTER_SELECT))) {
        const FilterPrm fp{prm->cov_rate, prm->map_qual, prm->sec_rat, prm->min_intron_n};
        rc = c->fusion_clk.launch(c, &c->fusion_stats[FUS_K_FILTER_SELECT], [&] {
            hipLaunchKernelGGL(k_filter_select, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, (int64_t)G, (const int64_t *)d_off.p, (const int32_t *)d_score.p,
                               (const int32_t *)d_in.p, fp, d_win.p);
        });
    }
    return download_all(c, rc, {{winner, d_win.p, G * 8}}, "l2r_filter_select");
}

// ---------------------------------------------------------------------------------------------- fusion
int l2r_fusion_segments(l2r_ctx *c, const l2r_fusion_records *r, int32_t *read_start, int32_t *read_end, int32_t *ref_start, int32_t *ref_end,
                        int32_t *qlen)
{
    {   std::string msg;
        if (fusion_segments_check(c, r, read_start, read_end, ref_start, ref_end, qlen, msg)) return fail(-1, "%s", msg.c_str()); }
    const size_t N = (size_t)r->n;
    if (N == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const bool wave = wave_form((double)r->n_cigar / (double)N, "L2R_FUSION_WAVE");
    DevBuf<uint16_t> d_flag; DevBuf<int32_t> d_pos, d_out; DevBuf<int64_t> d_off; DevBuf<uint32_t> d_cig;
    int rc = 0;
    if ((rc = to_dev(c, d_flag, r->flag, N)) || (rc = to_dev(c, d_pos, r->pos, N)) || (rc = to_dev(c, d_off, r->cig_off, N + 1)) ||
        (rc = to_dev(c, d_cig, r->cig, (size_t)r->n_cigar)) || d_out.ensure(5 * N)) rc = rc ? rc : -2;
    if (rc) return download_all(c, rc, {}, "l2r_fusion_segments");
    int32_t *o = d_out.p;
    if (!(rc = fusion_begin(c, FUS_K_SEG))) {
        const size_t threads = wave ? N * 64 : N;
        const dim3 grid((unsigned)((threads + 255) / 256));
        c->fusion_stats[FUS_WAVE] = wave ? 1.0 : 0.0;
        rc = c->fusion_clk.launch(c, &c->fusion_stats[FUS_K_SEG], [&] {
            if (wave) hipLaunchKernelGGL(k_fusion_seg<true>, grid, dim3(256), 0, c->stream, (int64_t)N, (const uint16_t *)d_flag.p, (const int32_t *)d_pos.p,
                                         (const int64_t *)d_off.p, (const uint32_t *)d_cig.p, o, o + N, o + 2 * N, o + 3 * N, o + 4 * N);
            else hipLaunchKernelGGL(k_fusion_seg<false>, grid, dim3(256), 0, c->stream, (int64_t)N, (const uint16_t *)d_flag.p, (const int32_t *)d_pos.p,
                                    (const int64_t *)d_off.p, (const uint32_t *)d_cig.p, o, o + N, o + 2 * N, o + 3 * N, o + 4 * N);
        });
    }
    return download_all(c, rc, {{read_start, o, N * 4}, {read_end, o + N, N * 4}, {ref_start, o + 2 * N, N * 4}, {ref_end, o + 3 * N, N * 4}, {qlen, o + 4 * N, N * 4}},
                        "l2r_fusion_segments");
}

int l2r_fusion_select(l2r_ctx *c, int64_t n_groups, const int64_t *group_off, const int32_t *score, const int32_t *ed, const int32_t *tid,
                      const int32_t *read_start, const int32_t *read_end, const int32_t *ref_start, const int32_t *ref_end,
                      const int32_t *rlen_of_group, const l2r_fusion_params *prm, int64_t *first, int64_t *second)
{
    {   std::string msg;
        if (fusion_select_check(c, n_groups, group_off, score, ed, tid, read_start, read_end, ref_start, ref_end, rlen_of_group, prm, first, second, msg))
            return fail(-1, "%s", msg.c_str()); }
    if (n_groups == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t G = (size_t)n_groups;
    const size_t R = (size_t)group_off[G];
    DevBuf<int64_t> d_off, d_out; DevBuf<int32_t> d_score, d_ed, d_tid, d_rs, d_re, d_fs, d_fe, d_rlen;
    int rc = 0;
    if ((rc = to_dev(c, d_off, group_off, G + 1)) || (rc = to_dev(c, d_score, score, R)) || (rc = to_dev(c, d_ed, ed, R)) || (rc = to_dev(c, d_tid, tid, R)) ||
        (rc = to_dev(c, d_rs, read_start, R)) || (rc = to_dev(c, d_re, read_end, R)) || (rc = to_dev(c, d_fs, ref_start, R)) ||
        (rc = to_dev(c, d_fe, ref_end, R)) || (rc = to_dev(c, d_rlen, rlen_of_group, G)) || d_out.ensure(2 * G)) rc = rc ? rc : -2;
    if (rc) return download_all(c, rc, {}, "l2r_fusion_select");
    if (!(rc = fusion_begin(c, FUS_K_SELECT))) {
        const FusionPrm fp{prm->ovlp_frac, prm->each_cov, prm->all_cov, prm->dis};
        rc = c->fusion_clk.launch(c, &c->fusion_stats[FUS_K_SELECT], [&] {
            hipLaunchKernelGGL(k_fusion_select, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, (int64_t)G, (const int64_t *)d_off.p,
                               (const int32_t *)d_score.p, (const int32_t *)d_ed.p, (const int32_t *)d_tid.p, (const int32_t *)d_rs.p, (const int32_t *)d_re.p,
                               (const int32_t *)d_fs.p, (const int32_t *)d_fe.p, (const int32_t *)d_rlen.p, fp, d_out.p, d_out.p + G);
        });
    }
    return download_all(c, rc, {{first, d_out.p, G * 8}, {second, d_out.p + G, G * 8}}, "l2r_fusion_select");
}

int l2r_fusion_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->fusion_stats : nullptr, FUS_N, out, n, "l2r_fusion_stats"); }

// ---------------------------------------------------------------------------------------------- bam2sj, sjtab
extern "C++" {
// v[0, n] <- the exclusive scan of v[0, n), *total_word <- the sum: one workgroup
static void scan_u32(l2r_ctx *c, uint32_t *v, int64_t n, uint32_t *total_word)
{
    ScanJobs jobs = {}; jobs.job[0] = ScanJob{v, n, total_word}; jobs.job[1] = jobs.job[0];
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, c->stream, jobs);
}

// hist: the 256 words of one key byte over n keys.  A byte that is equal in every key is a pass that is not run.
static bool byte_is_one_value(const uint32_t *hist, uint32_t n)
{
    for (int d = 0; d < 256; ++d) if (hist[d] == n) return true;
    return false;
}

// The passes of l2r_radix.hip.h over n rows, one per key byte of byte[0, n_pass), least significant first: digit histogram of every
// tile -> its scan -> scatter.  The caller owns the rows and their two sides: hist(b, p, n_tiles) and scatter(b, p, last, n_tiles)
// launch pass p over byte b, which reads the side pass p - 1 wrote.  The launches go through the caller's timer, which adds the time of
// the digit histogram to *ms[0], of the scan to *ms[1], of the scatter to *ms[2].  Which bytes run is the caller's rule.
template <typename Hist, typename Scatter>
static int radix_passes(l2r_ctx *c, StageTimer &clk, double *const ms[3], const int *byte, int n_pass, uint32_t n, DevBuf<uint32_t> &tile_hist, uint32_t *total_word,
                        Hist hist, Scatter scatter)
{
    const uint32_t n_tiles = (uint32_t)(((size_t)n + RADIX_TILE - 1) / RADIX_TILE);
    if (n_pass && tile_hist.ensure((size_t)256 * n_tiles + 1)) return -2;
    int rc;
    for (int p = 0; p < n_pass; ++p) {
        if ((rc = clk.launch(c, ms[0], [&] { hist(byte[p], p, n_tiles); }))) return rc;
        if ((rc = clk.launch(c, ms[1], [&] { scan_u32(c, tile_hist.p, (int64_t)256 * n_tiles, total_word); }))) return rc;
        if ((rc = clk.launch(c, ms[2], [&] { scatter(byte[p], p, p == n_pass - 1, n_tiles); }))) return rc;
    }
    return 0;
}

// The radix passes over the keys in c->sort.key[0][0, n), behind a keys kernel that left the histograms of the eight key bytes and the
// descent word in c->sort.hist.  A byte that is equal in every key is a pass that is not run, keys that never descend run none
// (L2R_SORT_FORCE=1: all eight, whatever the keys).  *n_pass_out: passes run; the order is then in c->sort.idx[*src_out], and with no
// pass it is the identity and no index column is written.  in_order_out may be null.  clk, ms: the caller's, as radix_passes takes them
// -- the sort buffers are lent to `sjtab -d`, `sort -n` and `sort-gtf`, the words of l2r_sort_stats are not.
static int sort_passes(l2r_ctx *c, StageTimer &clk, double *const ms[3], uint32_t n, int *n_pass_out, bool *in_order_out, int *src_out)
{
    SortState &s = c->sort;
    const bool force = env_on("L2R_SORT_FORCE");
    const size_t N = n;
    uint32_t h8[SORT_KEY_BYTES * 256 + 1];
    HIP_TRY(hipMemcpyAsync(h8, s.hist.p, sizeof h8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool in_order = h8[SORT_KEY_BYTES * 256] == 0u;
    int pass_byte[SORT_KEY_BYTES], n_pass = 0;
    for (int b = 0; b < SORT_KEY_BYTES; ++b) if (force || (!in_order && !byte_is_one_value(h8 + b * 256, n))) pass_byte[n_pass++] = b;
    *n_pass_out = n_pass; *src_out = n_pass & 1;
    if (in_order_out) *in_order_out = in_order;
    if (n_pass == 0) return 0;
    if (s.idx[0].ensure(N) || s.idx[1].ensure(N) || (n_pass > 1 && s.key[1].ensure(N))) return -2;
    return radix_passes(c, clk, ms, pass_byte, n_pass, n, s.tile_hist, s.word.p,
        [&](int b, int p, uint32_t n_tiles) {
            hipLaunchKernelGGL((k_radix_digit_hist<SortRows<false, false>>), dim3(n_tiles), dim3(RADIX_THREADS), 0, c->stream,
                               SortRows<false, false>{s.key[p & 1].p, nullptr, nullptr, nullptr}, n, b, n_tiles, s.tile_hist.p);
        },
        [&](int b, int p, bool last, uint32_t n_tiles) {
            const int from = p & 1;
#define SORT_SCATTER(F, L) hipLaunchKernelGGL((k_radix_scatter<SortRows<F, L>>), dim3(n_tiles), dim3(RADIX_THREADS), 0, c->stream, \
                                              SortRows<F, L>{s.key[from].p, s.idx[from].p, s.key[1 - from].p, s.idx[1 - from].p}, n, b, n_tiles, (const uint32_t *)s.tile_hist.p)
            if (p == 0 && last) SORT_SCATTER(true, true); else if (p == 0) SORT_SCATTER(true, false); else if (last) SORT_SCATTER(false, true); else SORT_SCATTER(false, false);
#undef SORT_SCATTER
        });
}

static_assert(SORT_THREADS == RADIX_THREADS && NAME_THREADS == RADIX_THREADS && SJ_THREADS == RADIX_THREADS && GTF_THREADS == RADIX_THREADS,
              "order_by_keys: one grid of k_radix_keys, whichever command's rows the keys are made of");

// The stable order of n rows by the 64-bit keys key_of makes of them, in the context's sort buffers: k_radix_keys<KeyOf> (the keys, which
// of their bytes differ at all, whether they descend anywhere), then sort_passes.  *idx: the order, null where no pass ran (the
// identity).  keys_copy: null, or where the keys go in row order before the passes use both key columns in turn.  clk: the caller's
// timer; the keys kernel's time is added to *ms_keys, the passes' to *ms_passes[0 .. 2].
template <typename KeyOf>
static int order_by_keys(l2r_ctx *c, StageTimer &clk, KeyOf key_of, uint32_t n, double *ms_keys, double *const ms_passes[3], int *n_pass, bool *in_order,
                         const uint32_t **idx, uint64_t *keys_copy = nullptr)
{
    SortState &o = c->sort;
    if (o.key[0].ensure(n) || o.hist.ensure(SORT_KEY_BYTES * 256 + 1) || o.word.ensure(4)) return -2;
    HIP_TRY(hipMemsetAsync(o.hist.p, 0, (SORT_KEY_BYTES * 256 + 1) * sizeof(uint32_t), c->stream));
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)n + RADIX_THREADS - 1) / RADIX_THREADS, 2048);
    int rc, src = 0;
    if ((rc = clk.launch(c, ms_keys, [&] {
            hipLaunchKernelGGL(k_radix_keys<KeyOf>, dim3(grid), dim3(RADIX_THREADS), 0, c->stream, key_of, (int64_t)n, o.key[0].p, o.hist.p, o.hist.p + SORT_KEY_BYTES * 256);
        }))) return rc;
    if (keys_copy) HIP_TRY(hipMemcpyAsync(keys_copy, o.key[0].p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = sort_passes(c, clk, ms_passes, n, n_pass, in_order, &src))) return rc;
    *idx = *n_pass ? o.idx[src].p : nullptr;
    return 0;
}
}

// slots of l2r_sort_stats
enum { SORTS_ROWS = 0, SORTS_PASSES, SORTS_IN_ORDER, SORTS_K_KEYS, SORTS_K_HIST, SORTS_K_SCAN, SORTS_K_SCATTER, SORTS_N };

// slots of l2r_sj_stats, in the order of SJ_STAT_NAMES (capi.py): the fifteen of `bam2sj`, behind them those of `sjtab`
enum { SJS_ROWS_MADE = 0, SJS_ROUNDS, SJS_PASSES, SJS_ROWS_IN, SJS_ROWS_OUT, SJS_K_COUNT, SJS_K_COUNT_SCAN, SJS_K_FILL, SJS_K_HIST12,
       SJS_K_HIST, SJS_K_HIST_SCAN, SJS_K_SCATTER, SJS_K_HEADS, SJS_K_REDUCE, SJS_K_MOTIF,
       SJS_DROPPED, SJS_INTRONS, SJS_K_INTRONS, SJS_K_ANNOTATE, SJS_K_KEEP, SJS_K_KEEP_SCAN, SJS_K_TAKE, SJS_INTRON_SORT,
       SJS_NEAR_DROPPED, SJS_ACC_PASSES, SJS_K_ACC_KEYS, SJS_K_ACC_ORDER, SJS_K_NEAR_ACC, SJS_K_KEEP_NEAR, SJS_LONG_DROPPED, SJS_N };
static_assert(SJS_K_HIST == 9 && SJS_DROPPED == 15 && SJS_NEAR_DROPPED == 23 && SJS_N <= 32, "l2r_sj_stats: the words of include/lr2rmats_hip.h");

// room for `want` rows; the first `keep` rows stay (DevBuf::ensure carries nothing over, so the columns are moved here)
static int sj_rows_reserve(l2r_ctx *c, const SjState &s, SjRowBuf &b, size_t want, size_t keep)
{
    const int n_col = s.over ? 6 : 5;
    if (want <= b.cap && (!s.over || b.col[5].cap >= b.cap)) return 0;
    const size_t cap = want <= b.cap ? b.cap : std::max(std::max(want, b.cap * 2), (size_t)1 << 16);      // (want <= cap: only the sixth column is missing)
    int32_t *q[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < n_col && e == hipSuccess; ++k) {
        e = hipMalloc((void **)&q[k], cap * sizeof(int32_t));
        if (e == hipSuccess && keep) e = hipMemcpyAsync(q[k], b.col[k].p, keep * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        for (int k = 0; k < n_col; ++k) if (q[k]) (void)hipFree(q[k]);
        return fail(-2, "[l2r_sj] %zu junction rows: %s", cap, hipGetErrorString(e));
    }
    for (int k = 0; k < n_col; ++k) { b.col[k].release(); b.col[k].p = q[k]; b.col[k].cap = cap; }
    b.cap = cap;
    return 0;
}

// s.rows[cur][0, n_rows) -> sorted by (tid, don, acc), one row per key with the count columns summed (and, s.over, the overhangs' maximum)
static int sj_compact(l2r_ctx *c, SjState &s)
{
    const int64_t n64 = s.n_rows;
    s.stats[SJS_ROUNDS] += 1; s.stats[SJS_PASSES] = 0; s.stats[SJS_ROWS_IN] = (double)n64; s.stats[SJS_ROWS_OUT] = 0;
    if (n64 == 0) return 0;
    if (n64 >= ((int64_t)1 << 31)) return fail(-1, "[l2r_sj] %lld junction rows in one sort (2^31 at most)", (long long)n64);
    const uint32_t n = (uint32_t)n64;
    const unsigned grid = (n + SJ_THREADS - 1) / SJ_THREADS;
    if (sj_rows_reserve(c, s, s.rows[1 - s.cur], n, 0) || s.hist12.ensure(SJ_KEY_BYTES * 256) || s.head.ensure((size_t)n + 1) || s.word.ensure(4)) return -2;
    // which key bytes differ at all
    uint32_t h12[SJ_KEY_BYTES * 256];
    HIP_TRY(hipMemsetAsync(s.hist12.p, 0, sizeof h12, c->stream));
    int rc = s.clk.launch(c, &s.stats[SJS_K_HIST12], [&] { hipLaunchKernelGGL(k_sj_hist12, dim3(std::min(grid, 2048u)), dim3(SJ_THREADS), 0, c->stream, s.rows[s.cur].cols(), n, s.hist12.p); });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h12, s.hist12.p, sizeof h12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int pass_byte[SJ_KEY_BYTES], passes = 0;
    for (int b = 0; b < SJ_KEY_BYTES; ++b) if (!byte_is_one_value(h12 + b * 256, n)) pass_byte[passes++] = b;
    auto rows = [&](int p) { const int from = s.cur ^ (p & 1); return SjRows<false>{s.rows[from].cols(), s.rows[1 - from].cols()}; };
    double *const ms[3] = {&s.stats[SJS_K_HIST], &s.stats[SJS_K_HIST_SCAN], &s.stats[SJS_K_SCATTER]};
    rc = radix_passes(c, s.clk, ms, pass_byte, passes, n, s.tile_hist, s.word.p,
        [&](int b, int p, uint32_t n_tiles) { hipLaunchKernelGGL(k_radix_digit_hist<SjRows<false>>, dim3(n_tiles), dim3(RADIX_THREADS), 0, c->stream, rows(p), n, b, n_tiles, s.tile_hist.p); },
        [&](int b, int p, bool, uint32_t n_tiles) {
            const SjRows<false> r = rows(p);
            if (s.over) hipLaunchKernelGGL(k_radix_scatter<SjRows<true>>, dim3(n_tiles), dim3(RADIX_THREADS), 0, c->stream, SjRows<true>{r.in, r.out}, n, b, n_tiles, (const uint32_t *)s.tile_hist.p);
            else hipLaunchKernelGGL(k_radix_scatter<SjRows<false>>, dim3(n_tiles), dim3(RADIX_THREADS), 0, c->stream, r, n, b, n_tiles, (const uint32_t *)s.tile_hist.p);
        });
    if (rc) return rc;
    const int src = s.cur ^ (passes & 1);
    // runs of equal keys
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_HEADS], [&] { hipLaunchKernelGGL(k_sj_heads, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[src].cols(), n, s.head.p); }))) return rc;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_HEADS], [&] { scan_u32(c, s.head.p, (int64_t)n, s.word.p); }))) return rc;
    uint32_t n_runs = 0;
    HIP_TRY(hipMemcpyAsync(&n_runs, s.word.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_runs == 0 || n_runs > n) return fail(-2, "[l2r_sj] %u runs in %u rows", n_runs, n);
    const int dst = 1 - src;
    HIP_TRY(hipMemsetAsync(s.rows[dst].col[3].p, 0, (size_t)n_runs * 4, c->stream));
    HIP_TRY(hipMemsetAsync(s.rows[dst].col[4].p, 0, (size_t)n_runs * 4, c->stream));
    if (s.over) { HIP_TRY(hipMemsetAsync(s.rows[dst].col[5].p, 0, (size_t)n_runs * 4, c->stream)); }
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_REDUCE], [&] {
            if (s.over) hipLaunchKernelGGL(k_sj_reduce<true>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[src].cols(), n, (const uint32_t *)s.head.p, s.rows[dst].cols(), n_runs);
            else hipLaunchKernelGGL(k_sj_reduce<false>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[src].cols(), n, (const uint32_t *)s.head.p, s.rows[dst].cols(), n_runs);
        }))) return rc;
    s.cur = dst; s.n_rows = n_runs;
    s.stats[SJS_PASSES] = passes; s.stats[SJS_ROWS_OUT] = n_runs;
    s.compact_at = std::max(s.compact_rows, 2 * s.n_rows);
    return 0;
}

// what l2r_sj_begin and l2r_sj_begin_tab share, and the state of the annotation's introns (no genome, no batches).  timing: L2R_SJ_TIMING=1
// as l2r_sj_begin found it
static int sj_state_begin(l2r_ctx *c, SjState &s, bool over, bool timing)
{
    s.open = false; s.finished = false; s.n_rows = 0; s.cur = 0; s.bcur = 0; s.n_seq = 0; s.over = over;
    for (double &v : s.stats) v = 0;
    const char *e = getenv("L2R_SJ_COMPACT_ROWS");
    s.compact_rows = e && atoll(e) > 0 ? atoll(e) : (int64_t)1 << 24;
    s.compact_at = s.compact_rows;
    if (s.word.ensure(4)) return -2;
    return s.clk.begin(timing, false);
}

static int sj_begin(l2r_ctx *c, const l2r_sj_params *prm, const l2r_sj_genome *g, bool over, const char *who)
{
    if (!c || !prm) return fail(-1, "[%s] null argument", who);
    if (g && (g->n_seq < 0 || (g->n_seq > 0 && (!g->seq_off || !g->bases)))) return fail(-1, "[%s] bad genome", who);
    HIP_TRY(hipSetDevice(c->device));
    SjState &s = c->sj;
    int rc;
    if ((rc = sj_state_begin(c, s, over, env_on("L2R_SJ_TIMING")))) return rc;
    s.prm = SjPrm{prm->min_intron, prm->pair_only};
    if (g && g->n_seq > 0) {
        for (int32_t k = 0; k < g->n_seq; ++k) if (g->seq_off[k + 1] < g->seq_off[k] || g->seq_off[0] != 0) return fail(-1, "[%s] sequence offsets do not ascend from 0", who);
        if ((rc = to_dev(c, s.seq_off, g->seq_off, (size_t)g->n_seq + 1)) || (rc = to_dev(c, s.bases, g->bases, (size_t)g->seq_off[g->n_seq]))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        s.n_seq = g->n_seq;
    }
    s.open = true;
    return 0;
}

int l2r_sj_begin(l2r_ctx *c, const l2r_sj_params *prm, const l2r_sj_genome *g) { return sj_begin(c, prm, g, false, "l2r_sj_begin"); }
int l2r_sj_begin_tab(l2r_ctx *c, const l2r_sj_params *prm, const l2r_sj_genome *g) { return sj_begin(c, prm, g, true, "l2r_sj_begin_tab"); }

static int sj_after_add(l2r_ctx *c, int64_t added)
{
    SjState &s = c->sj;
    s.n_rows += added; s.stats[SJS_ROWS_MADE] += (double)added; s.finished = false;
    return s.n_rows > s.compact_at ? sj_compact(c, s) : 0;
}

int l2r_sj_add(l2r_ctx *c, const l2r_sj_records *r)
{
    if (!c || !r) return fail(-1, "[l2r_sj_add] null argument");
    SjState &s = c->sj;
    if (!s.open) return fail(-1, "[l2r_sj_add] l2r_sj_begin comes first");
    if (r->n < 0 || r->n_cigar < 0 || r->n >= ((int64_t)1 << 31) || r->n_cigar >= ((int64_t)1 << 31)) return fail(-1, "[l2r_sj_add] a batch holds fewer than 2^31 records and CIGAR operations");
    if (r->n == 0) return 0;
    if (!r->flag || !r->tid || !r->pos || !r->uniq || !r->cig_off || (r->n_cigar && !r->cig)) return fail(-1, "[l2r_sj_add] null column");
    const size_t N = (size_t)r->n;
    if (r->cig_off[0] != 0 || r->cig_off[N] != r->n_cigar) return fail(-1, "[l2r_sj_add] cig_off does not span the CIGAR array");
    for (size_t i = 0; i < N; ++i) if (r->cig_off[i + 1] < r->cig_off[i]) return fail(-1, "[l2r_sj_add] cig_off descends at record %zu", i);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = to_dev(c, s.flag, r->flag, N)) || (rc = to_dev(c, s.tid, r->tid, N)) || (rc = to_dev(c, s.pos, r->pos, N)) || (rc = to_dev(c, s.uniq, r->uniq, N)) ||
        (rc = to_dev(c, s.cig_off, r->cig_off, N + 1)) || (rc = to_dev(c, s.cig, r->cig, (size_t)r->n_cigar))) return rc;
    if (s.cnt.ensure(N + 1)) return -2;
    const SjRecs recs{(int64_t)N, s.flag.p, s.tid.p, s.pos.p, s.uniq.p, s.cig_off.p, s.cig.p};
    const unsigned grid = (unsigned)((N + SJ_THREADS - 1) / SJ_THREADS);
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_COUNT], [&] { hipLaunchKernelGGL(k_sj_count, dim3(grid), dim3(SJ_THREADS), 0, c->stream, recs, s.prm, s.cnt.p); }))) return rc;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_COUNT_SCAN], [&] { scan_u32(c, s.cnt.p, (int64_t)N, s.word.p); }))) return rc;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, s.word.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (total == 0) return 0;
    if ((rc = sj_rows_reserve(c, s, s.rows[s.cur], (size_t)s.n_rows + total, (size_t)s.n_rows))) return rc;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_FILL], [&] {
            if (s.over) hipLaunchKernelGGL(k_sj_fill<true>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, recs, s.prm, (const uint32_t *)s.cnt.p, s.rows[s.cur].cols(), s.n_rows, s.n_rows + (int64_t)total);
            else hipLaunchKernelGGL(k_sj_fill<false>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, recs, s.prm, (const uint32_t *)s.cnt.p, s.rows[s.cur].cols(), s.n_rows, s.n_rows + (int64_t)total);
        }))) return rc;
    return sj_after_add(c, (int64_t)total);
}

// max_over: NULL -> the rows' overhang is 0 (only looked at in a table that has the column)
static int sj_add_rows(l2r_ctx *c, const l2r_junctions *j, const int32_t *max_over, const char *who)
{
    SjState &s = c->sj;
    if (j->n < 0 || j->n >= ((int64_t)1 << 31)) return fail(-1, "[%s] fewer than 2^31 rows at a time", who);
    if (j->n == 0) return 0;
    if (!j->tid || !j->don || !j->acc || !j->uniq_c || !j->multi_c) return fail(-1, "[%s] null column", who);
    if (max_over) for (int64_t i = 0; i < j->n; ++i) if (max_over[i] < 0) return fail(-1, "[%s] row %lld: negative overhang", who, (long long)i);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = sj_rows_reserve(c, s, s.rows[s.cur], (size_t)(s.n_rows + j->n), (size_t)s.n_rows))) return rc;
    const int32_t *src[5] = {j->tid, j->don, j->acc, j->uniq_c, j->multi_c};
    for (int k = 0; k < 5; ++k) HIP_TRY(hipMemcpyAsync(s.rows[s.cur].col[k].p + s.n_rows, src[k], (size_t)j->n * 4, hipMemcpyHostToDevice, c->stream));
    if (s.over) {
        if (max_over) { HIP_TRY(hipMemcpyAsync(s.rows[s.cur].col[5].p + s.n_rows, max_over, (size_t)j->n * 4, hipMemcpyHostToDevice, c->stream)); }
        else { HIP_TRY(hipMemsetAsync(s.rows[s.cur].col[5].p + s.n_rows, 0, (size_t)j->n * 4, c->stream)); }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return sj_after_add(c, j->n);
}

int l2r_sj_add_rows(l2r_ctx *c, const l2r_junctions *j)
{
    if (!c || !j) return fail(-1, "[l2r_sj_add_rows] null argument");
    if (!c->sj.open) return fail(-1, "[l2r_sj_add_rows] l2r_sj_begin comes first");
    return sj_add_rows(c, j, nullptr, "l2r_sj_add_rows");
}

int l2r_sj_add_rows_over(l2r_ctx *c, const l2r_junctions *j, const int32_t *max_over)
{
    if (!c || !j) return fail(-1, "[l2r_sj_add_rows_over] null argument");
    if (!c->sj.open) return fail(-1, "[l2r_sj_add_rows_over] l2r_sj_begin_tab comes first");
    if (!c->sj.over) return fail(-1, "[l2r_sj_add_rows_over] the table was begun with l2r_sj_begin: it has no overhang column (l2r_sj_begin_tab)");
    if (j->n > 0 && !max_over) return fail(-1, "[l2r_sj_add_rows_over] null column");
    return sj_add_rows(c, j, max_over, "l2r_sj_add_rows_over");
}

int l2r_sj_finish(l2r_ctx *c, int64_t *n_rows)
{
    if (!c || !n_rows) return fail(-1, "[l2r_sj_finish] null argument");
    SjState &s = c->sj;
    if (!s.open) return fail(-1, "[l2r_sj_finish] l2r_sj_begin comes first");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = sj_compact(c, s))) return rc;
    const uint32_t n = (uint32_t)s.n_rows;
    s.bcur = 0;
    if (s.strand[0].ensure(n ? n : 1) || s.motif[0].ensure(n ? n : 1)) return -2;
    if (s.over) {                                               // anno: all 0 until l2r_sj_annotate says otherwise
        if (s.anno[0].ensure(n ? n : 1)) return -2;
        HIP_TRY(hipMemsetAsync(s.anno[0].p, 0, n ? n : 1, c->stream));
        s.stats[SJS_DROPPED] = 0; s.stats[SJS_INTRONS] = 0;
    }
    if (n) {
        uint32_t bad = 0xffffffffu;
        HIP_TRY(hipMemcpyAsync(s.word.p + 1, &bad, 4, hipMemcpyHostToDevice, c->stream));
        const SjGenome g{s.n_seq, s.seq_off.p, s.bases.p};
        const SjCols t = s.rows[s.cur].cols();
        if ((rc = s.clk.launch(c, &s.stats[SJS_K_MOTIF], [&] { hipLaunchKernelGGL(k_sj_motif, dim3((n + SJ_THREADS - 1) / SJ_THREADS), dim3(SJ_THREADS), 0, c->stream, (const int32_t *)t.tid, (const int32_t *)t.don,
                                                             (const int32_t *)t.acc, n, g, s.strand[0].p, s.motif[0].p, s.word.p + 1); }))) return rc;
        HIP_TRY(hipMemcpyAsync(&bad, s.word.p + 1, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad != 0xffffffffu) {
            int32_t tid = -1;
            if (bad < n) HIP_TRY(hipMemcpy(&tid, t.tid + bad, 4, hipMemcpyDeviceToHost));
            return fail(L2R_SJ_E_UNKNOWN_TID, "[intr_deri_str] unknown tid: %d", tid);
        }
    }
    s.finished = true;
    *n_rows = s.n_rows;
    return 0;
}

// the calls behind l2r_sj_finish that only a table with the overhang column takes
static int sj_tab_ready(l2r_ctx *c, const char *who)
{
    const SjState &s = c->sj;
    if (s.open && !s.over) return fail(-1, "[%s] the table was begun with l2r_sj_begin: l2r_sj_begin_tab makes the table this call works on", who);
    if (!s.finished) return fail(-1, "[%s] l2r_sj_finish comes first", who);
    return 0;
}

int l2r_sj_annotate(l2r_ctx *c, const l2r_annotation *a)
{
    if (!c || !a) return fail(-1, "[l2r_sj_annotate] null argument");
    int rc;
    if ((rc = sj_tab_ready(c, "l2r_sj_annotate"))) return rc;
    if (a->n_tx < 0 || a->n_exon < 0 || a->n_exon >= ((int64_t)1 << 31) || a->n_tx >= ((int64_t)1 << 31)) return fail(-1, "[l2r_sj_annotate] fewer than 2^31 transcripts and exons");
    if (a->n_tx > 0 && (!a->tx_tid || !a->tx_ex_off)) return fail(-1, "[l2r_sj_annotate] null column");
    if (a->n_exon > 0 && (a->n_tx == 0 || !a->ex_start || !a->ex_end)) return fail(-1, "[l2r_sj_annotate] null column");
    if (a->n_tx > 0) {
        if (a->tx_ex_off[0] != 0 || a->tx_ex_off[a->n_tx] != a->n_exon) return fail(-1, "[l2r_sj_annotate] tx_ex_off does not span the exon array");
        for (int64_t t = 0; t < a->n_tx; ++t) if (a->tx_ex_off[t + 1] < a->tx_ex_off[t]) return fail(-1, "[l2r_sj_annotate] tx_ex_off descends at transcript %lld", (long long)t);
    }
    HIP_TRY(hipSetDevice(c->device));
    SjState &s = c->sj;
    SjIntrons &in = c->sj_intr;
    SjState &is = in.st;
    if ((rc = sj_state_begin(c, is, false, s.clk.on))) return rc;
    uint32_t n_in = 0;
    if (a->n_exon > 0) {
        const size_t T = (size_t)a->n_tx, E = (size_t)a->n_exon;
        if ((rc = to_dev(c, in.tx_tid, a->tx_tid, T)) || (rc = to_dev(c, in.tx_ex_off, a->tx_ex_off, T + 1)) || (rc = to_dev(c, in.ex_start, a->ex_start, E)) ||
            (rc = to_dev(c, in.ex_end, a->ex_end, E))) return rc;
        if ((rc = sj_rows_reserve(c, is, is.rows[0], E, 0))) return rc;
        HIP_TRY(hipMemsetAsync(is.word.p + 2, 0, 4, c->stream));
        const SjAnno an{a->n_tx, a->n_exon, in.tx_tid.p, in.tx_ex_off.p, in.ex_start.p, in.ex_end.p};
        if ((rc = s.clk.launch(c, &s.stats[SJS_K_INTRONS], [&] { hipLaunchKernelGGL(k_sj_introns, dim3((unsigned)((E + SJ_THREADS - 1) / SJ_THREADS)), dim3(SJ_THREADS), 0, c->stream, an, is.rows[0].cols(),
                                                                          is.word.p + 2, (uint32_t)E); }))) return rc;
        HIP_TRY(hipMemcpyAsync(&n_in, is.word.p + 2, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (n_in > E) return fail(-2, "[l2r_sj_annotate] %u introns from %zu exons", n_in, E);
        is.n_rows = n_in;
        if ((rc = sj_compact(c, is))) return rc;
        n_in = (uint32_t)is.n_rows;
        for (int k = SJS_K_HIST12; k <= SJS_K_REDUCE; ++k) s.stats[SJS_INTRON_SORT] += is.stats[k];
    }
    s.stats[SJS_INTRONS] = n_in;
    const uint32_t n = (uint32_t)s.n_rows;
    if (n) {
        const SjCols t = s.rows[s.cur].cols();
        if ((rc = s.clk.launch(c, &s.stats[SJS_K_ANNOTATE], [&] { hipLaunchKernelGGL(k_sj_annotate, dim3((n + SJ_THREADS - 1) / SJ_THREADS), dim3(SJ_THREADS), 0, c->stream, (const int32_t *)t.tid,
                                                                           (const int32_t *)t.don, (const int32_t *)t.acc, n, is.rows[is.cur].cols(), n_in, s.anno[s.bcur].p); }))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// keep words in s.head -> their scan -> the kept rows in the other row buffer and byte set, which become the current ones; *kept_out = rows left
static int sj_take_kept(l2r_ctx *c, SjState &s, uint32_t n, const char *who, uint32_t *kept_out)
{
    int rc;
    const unsigned grid = (n + SJ_THREADS - 1) / SJ_THREADS;
    const int bsrc = s.bcur, bdst = 1 - s.bcur, src = s.cur, dst = 1 - s.cur;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_KEEP_SCAN], [&] { scan_u32(c, s.head.p, (int64_t)n, s.word.p); }))) return rc;
    uint32_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, s.word.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kept > n) return fail(-2, "[%s] %u of %u rows kept", who, kept, n);
    if (kept) {
        const SjBytes bin{s.strand[bsrc].p, s.motif[bsrc].p, s.anno[bsrc].p}, bout{s.strand[bdst].p, s.motif[bdst].p, s.anno[bdst].p};
        if ((rc = s.clk.launch(c, &s.stats[SJS_K_TAKE], [&] { hipLaunchKernelGGL(k_sj_take, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[src].cols(), bin, n, (const uint32_t *)s.head.p,
                                                                       s.rows[dst].cols(), bout, kept); }))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    s.cur = dst; s.bcur = bdst; s.n_rows = kept;
    *kept_out = kept;
    return 0;
}

// room for the keep words and for the rows a filter stage leaves
static int sj_filter_reserve(l2r_ctx *c, SjState &s, uint32_t n)
{
    const int bdst = 1 - s.bcur;
    if (s.head.ensure((size_t)n + 1) || s.strand[bdst].ensure(n) || s.motif[bdst].ensure(n) || s.anno[bdst].ensure(n)) return -2;
    return sj_rows_reserve(c, s, s.rows[1 - s.cur], n, 0);
}

// The row-local stage of both filter calls.  g: the intron-size rule as well (the INTRON instance of k_sj_keep), or null: the launches
// of l2r_sj_filter_rows.  *n_long: rows the intron-size rule alone dropped.
static int sj_filter_local(l2r_ctx *c, const l2r_sj_filter *f, const SjFilter2 *g, const char *who, uint32_t *n_long)
{
    SjState &s = c->sj;
    const uint32_t n = (uint32_t)s.n_rows;
    *n_long = 0;
    SjFilter flt;
    for (int k = 0; k < 5; ++k) { flt.anchor_min[k] = f->anchor_min[k]; flt.uniq_min[k] = f->uniq_min[k]; flt.all_min[k] = f->all_min[k]; }
    const unsigned grid = (n + SJ_THREADS - 1) / SJ_THREADS;
    int rc;
    if ((rc = sj_filter_reserve(c, s, n))) return rc;
    const SjFilter2 none = {};
    if (g) HIP_TRY(hipMemsetAsync(s.word.p + 3, 0, 4, c->stream));
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_KEEP], [&] {
            if (g) hipLaunchKernelGGL(k_sj_keep<true>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[s.cur].cols(), (const uint8_t *)s.motif[s.bcur].p,
                                      (const uint8_t *)s.anno[s.bcur].p, n, flt, *g, s.head.p, s.word.p + 3);
            else hipLaunchKernelGGL(k_sj_keep<false>, dim3(grid), dim3(SJ_THREADS), 0, c->stream, s.rows[s.cur].cols(), (const uint8_t *)s.motif[s.bcur].p,
                                    (const uint8_t *)s.anno[s.bcur].p, n, flt, none, s.head.p, (uint32_t *)nullptr);
        }))) return rc;
    if (g) HIP_TRY(hipMemcpyAsync(n_long, s.word.p + 3, 4, hipMemcpyDeviceToHost, c->stream));      // (waited for with the scan's total)
    uint32_t kept = 0;
    return sj_take_kept(c, s, n, who, &kept);
}

int l2r_sj_filter_rows(l2r_ctx *c, const l2r_sj_filter *f, int64_t *n_rows)
{
    if (!c || !f || !n_rows) return fail(-1, "[l2r_sj_filter_rows] null argument");
    int rc;
    if ((rc = sj_tab_ready(c, "l2r_sj_filter_rows"))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    SjState &s = c->sj;
    const int64_t n = s.n_rows;
    for (int k = SJS_NEAR_DROPPED; k < SJS_N; ++k) s.stats[k] = 0;
    s.stats[SJS_DROPPED] = 0;
    *n_rows = s.n_rows;
    if (!n) return 0;
    uint32_t n_long = 0;
    if ((rc = sj_filter_local(c, f, nullptr, "l2r_sj_filter_rows", &n_long))) return rc;
    s.stats[SJS_DROPPED] = (double)(n - s.n_rows);
    *n_rows = s.n_rows;
    return 0;
}

// The neighbour stage over the rows the row-local stage left (s.rows[s.cur], sorted by (tid, don, acc)).
static int sj_filter_near(l2r_ctx *c, const SjFilter2 &g)
{
    SjState &s = c->sj;
    const uint32_t n = (uint32_t)s.n_rows;
    if (!n) return 0;
    const unsigned grid = (n + SJ_THREADS - 1) / SJ_THREADS;
    int rc;
    if ((rc = sj_filter_reserve(c, s, n))) return rc;
    if (s.near_acc.ensure(n)) return -2;
    const SjCols t = s.rows[s.cur].cols();
    double *const ms[3] = {&s.stats[SJS_K_ACC_ORDER], &s.stats[SJS_K_ACC_ORDER], &s.stats[SJS_K_ACC_ORDER]};
    int n_pass = 0;
    const uint32_t *idx = nullptr;
    if ((rc = order_by_keys(c, s.clk, SjAccKeyOf{t.tid, t.acc}, n, &s.stats[SJS_K_ACC_KEYS], ms, &n_pass, nullptr, &idx))) return rc;
    s.stats[SJS_ACC_PASSES] = n_pass;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_NEAR_ACC], [&] {
            hipLaunchKernelGGL(k_sj_near_acc, dim3(grid), dim3(SJ_THREADS), 0, c->stream, (const int32_t *)t.tid, (const int32_t *)t.acc, idx, n, s.near_acc.p);
        }))) return rc;
    if ((rc = s.clk.launch(c, &s.stats[SJS_K_KEEP_NEAR], [&] {
            hipLaunchKernelGGL(k_sj_keep_near, dim3(grid), dim3(SJ_THREADS), 0, c->stream, (const int32_t *)t.tid, (const int32_t *)t.don, (const int32_t *)s.near_acc.p,
                               (const uint8_t *)s.motif[s.bcur].p, (const uint8_t *)s.anno[s.bcur].p, n, g, s.head.p);
        }))) return rc;
    uint32_t kept = 0;
    if ((rc = sj_take_kept(c, s, n, "l2r_sj_filter_rows2", &kept))) return rc;
    s.stats[SJS_NEAR_DROPPED] = (double)(n - kept);
    return 0;
}

int l2r_sj_filter_rows2(l2r_ctx *c, const l2r_sj_filter *f, const l2r_sj_filter2 *g, int64_t *n_rows)
{
    if (!c || !f || !n_rows) return fail(-1, "[l2r_sj_filter_rows2] null argument");
    int rc;
    if ((rc = sj_tab_ready(c, "l2r_sj_filter_rows2"))) return rc;
    SjFilter2 flt = {};
    bool near = false;
    if (g) {
        if (g->n_intron_max < 0 || g->n_intron_max > 8) return fail(-1, "[l2r_sj_filter_rows2] n_intron_max = %d: the list holds 0 to 8 lengths", g->n_intron_max);
        for (int k = 0; k < 5; ++k) {
            if (g->dist_min[k] < 0) return fail(-1, "[l2r_sj_filter_rows2] dist_min[%d] = %d: a distance is not negative", k, g->dist_min[k]);
            flt.dist_min[k] = g->dist_min[k]; near |= g->dist_min[k] != 0;
        }
        for (int k = 0; k < g->n_intron_max; ++k) {
            if (g->intron_max[k] < 0) return fail(-1, "[l2r_sj_filter_rows2] intron_max[%d] = %d: a length is not negative", k, g->intron_max[k]);
            flt.intron_max[k] = g->intron_max[k];
        }
        flt.n_intron_max = g->n_intron_max;
    }
    SjState &s = c->sj;
    if (s.n_rows > (int64_t)0xffffffffll - L2R_SORT_TILE)
        return fail(-1, "[l2r_sj_filter_rows2] %lld rows: the acceptor order takes 2^32 - 1 - %d at most (the index of a row is a 32-bit word)", (long long)s.n_rows, L2R_SORT_TILE);
    if (!near && flt.n_intron_max == 0) return l2r_sj_filter_rows(c, f, n_rows);
    HIP_TRY(hipSetDevice(c->device));
    const int64_t n = s.n_rows;
    for (int k = SJS_NEAR_DROPPED; k < SJS_N; ++k) s.stats[k] = 0;
    s.stats[SJS_DROPPED] = 0;
    *n_rows = s.n_rows;
    if (!n) return 0;
    if (s.word.ensure(4)) return -2;
    uint32_t n_long = 0;
    rc = sj_filter_local(c, f, flt.n_intron_max ? &flt : nullptr, "l2r_sj_filter_rows2", &n_long);
    if (!rc && near) rc = sj_filter_near(c, flt);
    // (a failure behind the first stage leaves that stage's table, and the words say so)
    s.stats[SJS_LONG_DROPPED] = (double)n_long;
    s.stats[SJS_DROPPED] = (double)(n - s.n_rows);
    *n_rows = s.n_rows;
    return rc;
}

static int sj_download(l2r_ctx *c, int64_t cap, int64_t *n_out, int32_t *const dst[6], uint8_t *const bytes[3], const char *who)
{
    SjState &s = c->sj;
    if (cap < s.n_rows) return fail(-1, "[%s] room for %lld rows, the table has %lld", who, (long long)cap, (long long)s.n_rows);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)s.n_rows;
    *n_out = s.n_rows;
    if (!n) return 0;
    for (int k = 0; k < 6; ++k) if (dst[k]) HIP_TRY(hipMemcpyAsync(dst[k], s.rows[s.cur].col[k].p, n * 4, hipMemcpyDeviceToHost, c->stream));
    const uint8_t *from[3] = {s.strand[s.bcur].p, s.motif[s.bcur].p, s.anno[s.bcur].p};
    for (int k = 0; k < 3; ++k) if (bytes[k]) HIP_TRY(hipMemcpyAsync(bytes[k], from[k], n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int l2r_sj_download(l2r_ctx *c, l2r_sj_table *t)
{
    if (!c || !t) return fail(-1, "[l2r_sj_download] null argument");
    SjState &s = c->sj;
    if (!s.finished) return fail(-1, "[l2r_sj_download] l2r_sj_finish comes first");
    if (t->cap >= s.n_rows && s.n_rows && (!t->tid || !t->don || !t->acc || !t->uniq_c || !t->multi_c || !t->strand || !t->motif)) return fail(-1, "[l2r_sj_download] null column");
    int32_t *const dst[6] = {t->tid, t->don, t->acc, t->uniq_c, t->multi_c, nullptr};
    uint8_t *const bytes[3] = {t->strand, t->motif, nullptr};
    return sj_download(c, t->cap, &t->n, dst, bytes, "l2r_sj_download");
}

int l2r_sj_download_tab(l2r_ctx *c, l2r_sj_tab *t)
{
    if (!c || !t) return fail(-1, "[l2r_sj_download_tab] null argument");
    int rc;
    if ((rc = sj_tab_ready(c, "l2r_sj_download_tab"))) return rc;
    SjState &s = c->sj;
    if (t->cap >= s.n_rows && s.n_rows && (!t->tid || !t->don || !t->acc || !t->uniq_c || !t->multi_c || !t->strand || !t->motif || !t->anno || !t->max_over))
        return fail(-1, "[l2r_sj_download_tab] null column");
    int32_t *const dst[6] = {t->tid, t->don, t->acc, t->uniq_c, t->multi_c, t->max_over};
    uint8_t *const bytes[3] = {t->strand, t->motif, t->anno};
    return sj_download(c, t->cap, &t->n, dst, bytes, "l2r_sj_download_tab");
}

int l2r_sj_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->sj.stats : nullptr, SJS_N, out, n, "l2r_sj_stats"); }

// ---------------------------------------------------------------------------------------------- sort, filter -S
int l2r_sort_order(l2r_ctx *c, const l2r_sort_records *r, uint32_t *order_out)
{
    if (!c || !r) return fail(-1, "[l2r_sort_order] null argument");
    SortState &s = c->sort;
    for (double &v : s.stats) v = 0;
    if (r->n < 0) return fail(-1, "[l2r_sort_order] %lld records", (long long)r->n);
    if (r->n > (int64_t)0xffffffffll - L2R_SORT_TILE)
        return fail(-1, "[l2r_sort_order] %lld records: one sort takes 2^32 - 1 - %d at most (the index of a record is a 32-bit word)", (long long)r->n, L2R_SORT_TILE);
    if (r->n == 0) { s.stats[SORTS_IN_ORDER] = 1; return 0; }
    if (!r->flag || !r->tid || !r->pos || !order_out) return fail(-1, "[l2r_sort_order] null column");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = s.clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    const size_t N = (size_t)r->n;
    s.stats[SORTS_ROWS] = (double)r->n;
    if ((rc = to_dev(c, s.flag, r->flag, N)) || (rc = to_dev(c, s.tid, r->tid, N)) || (rc = to_dev(c, s.pos, r->pos, N))) return rc;
    double *const ms[3] = {&s.stats[SORTS_K_HIST], &s.stats[SORTS_K_SCAN], &s.stats[SORTS_K_SCATTER]};
    int n_pass = 0; bool in_order = false;
    const uint32_t *idx = nullptr;
    if ((rc = order_by_keys(c, s.clk, SortKeyOf{s.flag.p, s.tid.p, s.pos.p}, (uint32_t)r->n, &s.stats[SORTS_K_KEYS], ms, &n_pass, &in_order, &idx))) return rc;
    s.stats[SORTS_IN_ORDER] = in_order ? 1 : 0;
    if (n_pass == 0) {                                              // (keys that never descend: the order is the identity)
        for (size_t i = 0; i < N; ++i) order_out[i] = (uint32_t)i;
        return 0;
    }
    s.stats[SORTS_PASSES] = n_pass;
    HIP_TRY(hipMemcpyAsync(order_out, idx, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int l2r_sort_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->sort.stats : nullptr, SORTS_N, out, n, "l2r_sort_stats"); }

// ---------------------------------------------------------------------------------------------- sort -n, filter -N, fusion -N
// slots of l2r_name_stats
enum { NAMES_ROWS = 0, NAMES_GROUPS, NAMES_PASSES, NAMES_IDENTITY, NAMES_ROUTE, NAMES_MISMATCH, NAMES_K_HASH, NAMES_K_PASSES, NAMES_K_HEADS, NAMES_K_SCANS, NAMES_K_PLACE, NAMES_N };
static_assert(NAMES_N == sizeof(NameState::stats) / sizeof(double), "l2r_name_stats: the words of include/lr2rmats_hip.h");

// One run over the names on the device with one seed: the order in m.order, *groups, *mismatch (pairs with one hash and two names: the
// order is exact iff 0), *moved (0: the identity).
static int name_order_seeded(l2r_ctx *c, uint32_t n, int64_t off0, uint64_t seed, uint64_t mask, uint32_t *groups, uint32_t *mismatch, uint32_t *moved)
{
    NameState &m = c->name;
    const size_t N = n;
    const unsigned grid = (unsigned)((N + NAME_THREADS - 1) / NAME_THREADS);
    const NameCols cols{m.blob.p, m.off.p, off0};
    int rc;
    HIP_TRY(hipMemsetAsync(m.word.p, 0, 4 * sizeof(uint32_t), c->stream));
    // the order by the hashes; a copy of them in record order for k_name_heads
    double *const ms[3] = {&m.stats[NAMES_K_PASSES], &m.stats[NAMES_K_PASSES], &m.stats[NAMES_K_PASSES]};
    int n_pass = 0;
    const uint32_t *idx = nullptr;
    if ((rc = order_by_keys(c, m.clk, NameHashOf{cols, seed, mask}, n, &m.stats[NAMES_K_HASH], ms, &n_pass, nullptr, &idx, m.hkey.p))) return rc;
    m.stats[NAMES_PASSES] = n_pass;
    if ((rc = m.clk.launch(c, &m.stats[NAMES_K_HEADS], [&] {
            hipLaunchKernelGGL(k_name_heads, dim3(grid), dim3(NAME_THREADS), 0, c->stream, cols, (const uint64_t *)m.hkey.p, idx, n, m.head.p, m.word.p + 1);
        }))) return rc;
    if ((rc = m.clk.launch(c, &m.stats[NAMES_K_SCANS], [&] { scan_u32(c, m.head.p, (int64_t)n, m.word.p); }))) return rc;
    HIP_TRY(hipMemsetAsync(m.sizes.p, 0, (N + 1) * sizeof(uint32_t), c->stream));
    if ((rc = m.clk.launch(c, &m.stats[NAMES_K_PLACE], [&] {
            hipLaunchKernelGGL(k_name_firsts, dim3(grid), dim3(NAME_THREADS), 0, c->stream, (const uint32_t *)m.head.p, idx, n, m.head_pos.p, m.first_idx.p);
            hipLaunchKernelGGL(k_name_sizes, dim3(grid), dim3(NAME_THREADS), 0, c->stream, (const uint32_t *)m.head.p, (const uint32_t *)m.head_pos.p, (const uint32_t *)m.first_idx.p, n, m.sizes.p);
        }))) return rc;
    if ((rc = m.clk.launch(c, &m.stats[NAMES_K_SCANS], [&] { scan_u32(c, m.sizes.p, (int64_t)n, m.word.p + 3); }))) return rc;
    if ((rc = m.clk.launch(c, &m.stats[NAMES_K_PLACE], [&] {
            hipLaunchKernelGGL(k_name_place, dim3(grid), dim3(NAME_THREADS), 0, c->stream, (const uint32_t *)m.head.p, idx, (const uint32_t *)m.head_pos.p, (const uint32_t *)m.first_idx.p,
                               (const uint32_t *)m.sizes.p, n, m.order.p, m.word.p + 2);
        }))) return rc;
    uint32_t w[4];
    HIP_TRY(hipMemcpyAsync(w, m.word.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *groups = w[0]; *mismatch = w[1]; *moved = w[2];
    return 0;
}

int l2r_name_order(l2r_ctx *c, const l2r_name_records *r, uint32_t *order_out, int64_t *n_groups)
{
    if (!c) return fail(-1, "[l2r_name_order] null argument");
    NameState &m = c->name;
    for (double &v : m.stats) v = 0;
    {   std::string msg;
        if (name_check(r, order_out, n_groups, msg)) return fail(-1, "%s", msg.c_str()); }
    *n_groups = 0;
    if (r->n == 0) { m.stats[NAMES_IDENTITY] = 1; return 0; }
    uint64_t mask = ~0ull;
    if (const char *e = getenv("L2R_NAME_HASH_BITS")) { const int b = atoi(e); mask = b >= 64 ? ~0ull : b <= 0 ? 0ull : (1ull << b) - 1ull; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    const size_t N = (size_t)r->n;
    const uint32_t n = (uint32_t)r->n;
    const int64_t off0 = r->name_off[0];
    const size_t bytes = (size_t)(r->name_off[N] - off0);
    m.stats[NAMES_ROWS] = (double)r->n;
    if ((rc = to_dev(c, m.off, r->name_off, N + 1))) return rc;
    if (m.blob.ensure((bytes + NAME_BLOB_ROOM + 7) / 8)) return -2;
    if (bytes) HIP_TRY(hipMemcpyAsync(m.blob.p, r->names + off0, bytes, hipMemcpyHostToDevice, c->stream));
    if (m.hkey.ensure(N) || m.head.ensure(N + 1) || m.head_pos.ensure(N + 1) || m.first_idx.ensure(N) || m.sizes.ensure(N + 1) || m.order.ensure(N) || m.word.ensure(4)) return -2;
    static const uint64_t seeds[2] = {0x243f6a8885a308d3ull, 0x13198a2e03707344ull};
    uint32_t groups = 0, mismatch = 1, moved = 1;
    int route = 0;
    for (; route < 2 && mismatch; ++route) {
        if ((rc = name_order_seeded(c, n, off0, seeds[route], mask, &groups, &mismatch, &moved))) return rc;
        if (route == 0) m.stats[NAMES_MISMATCH] = (double)mismatch;
    }
    if (mismatch) {                                                 // both seeds left a pair with one hash and two names: the exact routine
        *n_groups = name_order_host(r->n, r->name_off, r->names, order_out);
        moved = 0;
        for (size_t i = 0; i < N && !moved; ++i) moved = order_out[i] != (uint32_t)i;
        m.stats[NAMES_ROUTE] = 2;
    } else {
        HIP_TRY(hipMemcpyAsync(order_out, m.order.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *n_groups = (int64_t)groups;
        m.stats[NAMES_ROUTE] = route - 1;
    }
    m.stats[NAMES_GROUPS] = (double)*n_groups;
    m.stats[NAMES_IDENTITY] = moved ? 0 : 1;
    return 0;
}

int l2r_name_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->name.stats : nullptr, NAMES_N, out, n, "l2r_name_stats"); }

// ---------------------------------------------------------------------------------------------- sort-gtf
// slots of l2r_gtf_stats
enum { GTFS_BYTES = 0, GTFS_LINES, GTFS_ROWS, GTFS_TX, GTFS_HEADS, GTFS_BEYOND, GTFS_PASSES1, GTFS_PASSES2, GTFS_IDENTITY, GTFS_ROUTE,
       GTFS_K_LINES, GTFS_K_FIELDS, GTFS_K_SCANS, GTFS_K_ROWS, GTFS_K_SORT, GTFS_K_COMPOSE, GTFS_NAMES, GTFS_N };
static_assert(GTFS_N == sizeof(GtfState::stats) / sizeof(double) && GTFS_K_LINES == 10, "l2r_gtf_stats: the words of include/lr2rmats_hip.h");
// words of GtfState::word
enum { GTFW_NEWLINES = 0, GTFW_NUL, GTFW_BAD_LINE, GTFW_ROWS, GTFW_TX, GTFW_HEADS, GTFW_DESCENDS, GTFW_N };

// the host route: the exact routine of l2r_gtforder.hip.h
static int gtf_order_on_host(l2r_ctx *c, const l2r_gtf_text *t, int64_t *n_rows)
{
    GtfState &m = c->gtf;
    GtfOrder o;
    std::string msg;
    if (gtf_order_host(t->text, (uint64_t)t->n_bytes, o, msg)) return fail(-1, "%s", msg.c_str());
    m.res_start.swap(o.start); m.res_len.swap(o.len); m.res_line.swap(o.line);
    m.stats[GTFS_LINES] = (double)o.n_lines; m.stats[GTFS_ROWS] = (double)m.res_start.size(); m.stats[GTFS_TX] = (double)o.n_tx;
    m.stats[GTFS_HEADS] = (double)o.n_heads; m.stats[GTFS_BEYOND] = (double)o.n_beyond; m.stats[GTFS_NAMES] = (double)o.n_names;
    m.stats[GTFS_IDENTITY] = o.descent_line ? 0 : 1;
    m.stats[GTFS_ROUTE] = 1;
    *n_rows = (int64_t)m.res_start.size();
    return 0;
}

int l2r_gtf_order(l2r_ctx *c, const l2r_gtf_text *t, int64_t *n_rows)
{
    if (!c) return fail(-1, "[l2r_gtf_order] null argument");
    GtfState &m = c->gtf;
    for (double &v : m.stats) v = 0;
    m.res_start.clear(); m.res_len.clear(); m.res_line.clear();
    {   std::string msg;
        if (gtf_check(t, n_rows, msg)) return fail(-1, "%s", msg.c_str()); }
    *n_rows = 0;
    m.stats[GTFS_BYTES] = (double)t->n_bytes;
    if (t->n_bytes == 0) { m.stats[GTFS_IDENTITY] = 1; return 0; }
    const char *e = getenv("L2R_GTF_ROUTE");
    if ((e && strcmp(e, "host") == 0) || !gtf_text_fits_device(t->n_bytes)) return gtf_order_on_host(c, t, n_rows);
    const bool force = env_on("L2R_SORT_FORCE");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    const uint32_t n = (uint32_t)t->n_bytes;
    const size_t n_words = ((size_t)n + GTF_TEXT_ROOM + 15) / 16;
    const unsigned n_tiles = (unsigned)(((size_t)n + GTF_TILE - 1) / GTF_TILE);
    // ---- lines
    if (m.text.ensure(n_words) || m.tile_cnt.ensure((size_t)n_tiles + 1) || m.word.ensure(GTFW_N)) return -2;
    HIP_TRY(hipMemsetAsync((uint8_t *)m.text.p + n, 0, n_words * 16 - n, c->stream));
    HIP_TRY(hipMemcpyAsync(m.text.p, t->text, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(m.word.p, 0, GTFW_N * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(m.word.p + GTFW_BAD_LINE, 0xff, sizeof(uint32_t), c->stream));
    const uint8_t *text8 = (const uint8_t *)m.text.p;
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_LINES], [&] {
            hipLaunchKernelGGL(k_gtf_count, dim3(n_tiles), dim3(GTF_THREADS), 0, c->stream, (const uint4 *)m.text.p, n, m.tile_cnt.p, m.word.p + GTFW_NUL);
        }))) return rc;
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_SCANS], [&] { scan_u32(c, m.tile_cnt.p, (int64_t)n_tiles, m.word.p + GTFW_NEWLINES); }))) return rc;
    uint32_t w[GTFW_N];
    HIP_TRY(hipMemcpyAsync(w, m.word.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t open_end = t->text[n - 1] != '\n' ? 1u : 0u;
    if ((uint64_t)w[GTFW_NEWLINES] > (uint64_t)n) return fail(-2, "[l2r_gtf_order] %u newlines in %u bytes", w[GTFW_NEWLINES], n);
    const uint32_t L = w[GTFW_NEWLINES] + open_end;                 // (>= 1: the text is not empty; <= n < 2^32 - 64)
    const size_t NL = L;
    const unsigned grid_l = (unsigned)((NL + GTF_THREADS - 1) / GTF_THREADS);
    m.stats[GTFS_LINES] = (double)L;
    if (m.start.ensure(NL + 1) || m.kept.ensure(NL + 1) || m.tx.ensure(NL + 1) || m.l_name_off.ensure(NL) || m.l_name_len.ensure(NL) || m.l_s.ensure(NL) || m.l_e.ensure(NL)) return -2;
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_LINES], [&] {
            hipLaunchKernelGGL(k_gtf_starts, dim3(n_tiles), dim3(GTF_THREADS), 0, c->stream, (const uint4 *)m.text.p, n, (const uint32_t *)m.tile_cnt.p, L, open_end, m.start.p);
        }))) return rc;
    // ---- fields
    const GtfLineCols lines{m.kept.p, m.tx.p, m.l_name_off.p, m.l_name_len.p, m.l_s.p, m.l_e.p};
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_FIELDS], [&] {
            hipLaunchKernelGGL(k_gtf_fields, dim3(grid_l), dim3(GTF_THREADS), 0, c->stream, text8, n, (const uint32_t *)m.start.p, L, lines, m.word.p + GTFW_BAD_LINE);
        }))) return rc;
    // ---- compaction and carry: both scans in one launch
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_SCANS], [&] {
            ScanJobs jobs = {}; jobs.job[0] = ScanJob{m.kept.p, (int64_t)L, m.word.p + GTFW_ROWS}; jobs.job[1] = ScanJob{m.tx.p, (int64_t)L, m.word.p + GTFW_TX};
            hipLaunchKernelGGL(k_scan_u32, dim3(2), dim3(1024), 0, c->stream, jobs);
        }))) return rc;
    HIP_TRY(hipMemcpyAsync(w, m.word.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    {   // the domain: the smallest of the first line with a NUL byte and the first bad transcript line
        int64_t bad = w[GTFW_BAD_LINE] == 0xffffffffu ? 0 : (int64_t)w[GTFW_BAD_LINE];
        if (w[GTFW_NUL]) { const int64_t z = gtf_first_nul_line(t->text, n); if (z && (!bad || z < bad)) bad = z; }
        if (bad) {
            uint64_t lb = 0, le = 0;
            std::string msg;
            if (!gtf_find_line(t->text, n, bad, &lb, &le)) return fail(-2, "[l2r_gtf_order] the device names line %lld of %u", (long long)bad, L);
            (void)gtf_line_error(t->text, lb, le, bad, msg);
            return fail(-1, "%s", msg.c_str());
        }
    }
    const uint32_t R = w[GTFW_ROWS], T = w[GTFW_TX];
    if (R > L || T > R) return fail(-2, "[l2r_gtf_order] %u rows and %u transcripts of %u lines", R, T, L);
    m.stats[GTFS_ROWS] = (double)R; m.stats[GTFS_TX] = (double)T;
    if (R == 0) { m.stats[GTFS_IDENTITY] = 1; return 0; }
    if (!gtf_rows_fit_device((int64_t)R)) { for (double &v : m.stats) v = 0; m.stats[GTFS_BYTES] = (double)t->n_bytes; return gtf_order_on_host(c, t, n_rows); }
    const size_t NR = R, NT = T;
    const unsigned grid_r = (unsigned)((NR + GTF_THREADS - 1) / GTF_THREADS), grid_t = (unsigned)((NT + GTF_THREADS - 1) / GTF_THREADS);
    if (m.r_start.ensure(NR) || m.r_len.ensure(NR) || m.r_line.ensure(NR) || m.r_tx.ensure(NR) || m.t_name_off.ensure(NT) || m.t_name_len.ensure(NT) || m.t_s.ensure(NT) || m.t_e.ensure(NT) ||
        m.head.ensure(NT + 1) || m.c.ensure(NR) || m.s.ensure(NR) || m.e.ensure(NR)) return -2;
    const GtfTxCols txs{m.t_name_off.p, m.t_name_len.p, m.t_s.p, m.t_e.p};
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_ROWS], [&] {
            hipLaunchKernelGGL(k_gtf_rows, dim3(grid_l), dim3(GTF_THREADS), 0, c->stream, (const uint32_t *)m.start.p, n, L, (const uint32_t *)m.kept.p, (const uint32_t *)m.tx.p, lines, R, T,
                               GtfRowCols{m.r_start.p, m.r_len.p, m.r_line.p, m.r_tx.p}, txs);
            if (T) hipLaunchKernelGGL(k_gtf_chr_heads, dim3(grid_t), dim3(GTF_THREADS), 0, c->stream, text8, n, txs, T, m.head.p);
        }))) return rc;
    // ---- chromosome ranks: the heads to the host, one word per head back
    uint32_t H = 0;
    if (T) {
        if ((rc = m.clk.launch(c, &m.stats[GTFS_K_SCANS], [&] { scan_u32(c, m.head.p, (int64_t)T, m.word.p + GTFW_HEADS); }))) return rc;
        HIP_TRY(hipMemcpyAsync(&H, m.word.p + GTFW_HEADS, sizeof H, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (H == 0 || H > T) return fail(-2, "[l2r_gtf_order] %u heads of %u transcripts", H, T);
        if (m.h_off.ensure(H) || m.h_len.ensure(H) || m.rank.ensure(H)) return -2;
        if ((rc = m.clk.launch(c, &m.stats[GTFS_K_ROWS], [&] {
                hipLaunchKernelGGL(k_gtf_head_take, dim3(grid_t), dim3(GTF_THREADS), 0, c->stream, (const uint32_t *)m.head.p, txs, T, H, m.h_off.p, m.h_len.p);
            }))) return rc;
        std::vector<uint32_t> off(H), len(H), rank(H);
        HIP_TRY(hipMemcpyAsync(off.data(), m.h_off.p, (size_t)H * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(len.data(), m.h_len.p, (size_t)H * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        GtfChrRanks ranks;
        if (gtf_rank_heads(t->text, n, off.data(), len.data(), H, rank.data(), ranks)) return fail(-2, "[l2r_gtf_order] a head's name reaches beyond the text");
        m.stats[GTFS_BEYOND] = (double)ranks.beyond; m.stats[GTFS_NAMES] = (double)ranks.distinct();
        HIP_TRY(hipMemcpyAsync(m.rank.p, rank.data(), (size_t)H * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                   // (rank is this scope's)
    }
    m.stats[GTFS_HEADS] = (double)H;
    // ---- keys and order
    if ((rc = m.clk.launch(c, &m.stats[GTFS_K_ROWS], [&] {
            hipLaunchKernelGGL(k_gtf_triples, dim3(grid_r), dim3(GTF_THREADS), 0, c->stream,
                               GtfTripleIn{m.r_tx.p, m.head.p, m.rank.p, m.t_s.p, m.t_e.p, T, H}, R, m.c.p, m.s.p, m.e.p, m.word.p + GTFW_DESCENDS);
        }))) return rc;
    uint32_t descends = 0;
    HIP_TRY(hipMemcpyAsync(&descends, m.word.p + GTFW_DESCENDS, sizeof descends, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.stats[GTFS_IDENTITY] = descends ? 0 : 1;
    const bool sorted = descends || force;
    if (sorted) {
        if (m.order1.ensure(NR) || m.order.ensure(NR)) return -2;
        double *const ms[3] = {&m.stats[GTFS_K_SORT], &m.stats[GTFS_K_SORT], &m.stats[GTFS_K_SORT]};
        const uint32_t *order1 = nullptr, *perm2 = nullptr;
        int n_pass = 0;
        // stage 1: by e
        if ((rc = order_by_keys(c, m.clk, GtfEndKeyOf{m.e.p}, R, ms[0], ms, &n_pass, nullptr, &order1))) return rc;
        m.stats[GTFS_PASSES1] = n_pass;
        if (order1) {                                               // (stage 2 runs in the same index columns)
            HIP_TRY(hipMemcpyAsync(m.order1.p, order1, NR * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            order1 = m.order1.p;
        }
        // stage 2: by c << 32 | s, read through stage 1's order
        if ((rc = order_by_keys(c, m.clk, GtfChrStartKeyOf{m.c.p, m.s.p, order1, R}, R, ms[0], ms, &n_pass, nullptr, &perm2))) return rc;
        m.stats[GTFS_PASSES2] = n_pass;
        if ((rc = m.clk.launch(c, &m.stats[GTFS_K_COMPOSE], [&] {
                hipLaunchKernelGGL(k_gtf_compose, dim3(grid_r), dim3(GTF_THREADS), 0, c->stream, order1, perm2, R, m.order.p);
            }))) return rc;
    }
    // ---- the rows, in the order
    std::vector<uint32_t> r_start(NR), r_len(NR), r_line(NR), order(sorted ? NR : 0);
    HIP_TRY(hipMemcpyAsync(r_start.data(), m.r_start.p, NR * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r_len.data(), m.r_len.p, NR * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(r_line.data(), m.r_line.p, NR * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (sorted) HIP_TRY(hipMemcpyAsync(order.data(), m.order.p, NR * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.res_start.resize(NR); m.res_len.resize(NR); m.res_line.resize(NR);
    for (size_t k = 0; k < NR; ++k) {
        const size_t r = sorted ? order[k] : k;
        if (r >= NR) { m.res_start.clear(); m.res_len.clear(); m.res_line.clear(); return fail(-2, "[l2r_gtf_order] rank %zu holds row %zu of %zu", k, r, NR); }
        m.res_start[k] = r_start[r]; m.res_len[k] = r_len[r]; m.res_line[k] = r_line[r];
    }
    *n_rows = (int64_t)R;
    return 0;
}

int l2r_gtf_rows_out(l2r_ctx *c, l2r_gtf_rows *rows)
{
    if (!c || !rows) return fail(-1, "[l2r_gtf_rows_out] null argument");
    const GtfState &m = c->gtf;
    const size_t N = m.res_start.size();
    if (rows->cap < (int64_t)N) return fail(-1, "[l2r_gtf_rows_out] room for %lld rows, the last l2r_gtf_order left %zu", (long long)rows->cap, N);
    if (N && (!rows->start || !rows->len || !rows->line)) return fail(-1, "[l2r_gtf_rows_out] null column");
    if (N) {
        memcpy(rows->start, m.res_start.data(), N * sizeof(uint64_t));
        memcpy(rows->len, m.res_len.data(), N * sizeof(uint32_t));
        memcpy(rows->line, m.res_line.data(), N * sizeof(uint32_t));
    }
    rows->n = (int64_t)N;
    return 0;
}

int l2r_gtf_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->gtf.stats : nullptr, GTFS_N, out, n, "l2r_gtf_stats"); }

int l2r_gtf_check(const l2r_gtf_text *t, int64_t *line, int64_t *counts)
{
    std::string msg;
    int64_t dummy = 0;
    if (!line) return fail(-1, "[l2r_gtf_check] null argument");
    if (gtf_check(t, &dummy, msg)) return fail(-1, "%s", msg.c_str());
    GtfOrder o;
    if (gtf_order_host(t->text, (uint64_t)t->n_bytes, o, msg, false)) return fail(-1, "%s", msg.c_str());
    *line = o.descent_line;
    if (counts) { counts[0] = o.n_lines; counts[1] = (int64_t)o.start.size(); counts[2] = o.n_tx; counts[3] = o.n_names; }
    return o.descent_line ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- bam2bed
// slots of l2r_bed_stats
enum { BEDS_RECORDS = 0, BEDS_LINES, BEDS_BYTES, BEDS_WAVE, BEDS_TILES_LDS, BEDS_TILES_DIRECT, BEDS_ROUTE, BEDS_GUARD, BEDS_K_MEASURE, BEDS_K_SCAN, BEDS_K_WRITE, BEDS_N };
static_assert(BEDS_N == sizeof(BedState::stats) / sizeof(double) && BEDS_K_MEASURE == 8, "l2r_bed_stats: the words of include/lr2rmats_hip.h");
// words of BedState::word
enum { BEDW_BAD = 0, BEDW_TOTAL, BEDW_DIRECT, BEDW_N };

int l2r_bed_begin(l2r_ctx *c, const l2r_bed_params *p)
{
    if (!c) return fail(-1, "[l2r_bed_begin] null argument");
    BedState &m = c->bed;
    m.begun = false; m.out.have = false;
    {   std::string msg;
        if (bed_check_params(p, msg)) return fail(-1, "%s", msg.c_str()); }
    m.ref.set(p->n_ref, p->ref_off, p->ref_names);
    m.prm = *p;
    m.prm.ref_off = m.ref.h_off.data(); m.prm.ref_names = m.ref.h_names.data();
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = m.ref.upload(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.begun = true;
    return 0;
}

int l2r_bed_lines(l2r_ctx *c, const l2r_bed_records *r, int64_t *n_lines, int64_t *n_bytes)
{
    if (!c || !n_lines || !n_bytes) return fail(-1, "[l2r_bed_lines] null argument");
    BedState &m = c->bed;
    for (double &v : m.stats) v = 0;
    m.out.reset();
    if (!m.begun) return fail(-1, "[l2r_bed_lines] no l2r_bed_begin in front");
    {   std::string msg;
        if (bed_check_records(r, msg)) return fail(-1, "%s", msg.c_str()); }
    *n_lines = 0; *n_bytes = 0;
    const size_t N = (size_t)r->n;
    m.stats[BEDS_RECORDS] = (double)N; m.stats[BEDS_GUARD] = 1;
    const bool on_host = route_is_host("L2R_BED_ROUTE");
    m.stats[BEDS_ROUTE] = on_host ? 1 : 0;
    if (N == 0) { m.out.take_host(); return 0; }
    if (N > (size_t)0xffffffffu - 1u) return fail(-1, "[l2r_bed_lines] a batch of %zu records (at most 2^32 - 2)", N);
    if (bed_batch_bound(r, &m.prm) >= BED_BATCH_BYTES)
        return fail(-1, "[l2r_bed_lines] the batch: the summed bounds of its %zu lines reach 2^32 - 64 bytes (cut it with l2r_bed_cut)", N);
    int64_t lines = 0;
    for (size_t i = 0; i < N; ++i) lines += (r->flag[i] & 4u) ? 0 : 1;
    if (on_host) {
        std::string msg;
        if (bed_lines_host(r, &m.prm, m.out.host_text, nullptr, msg)) { m.out.host_text.clear(); return fail(-1, "%s", msg.c_str()); }
        m.out.take_host();
        m.stats[BEDS_LINES] = (double)lines; m.stats[BEDS_BYTES] = (double)m.out.n_bytes;
        *n_lines = lines; *n_bytes = m.out.n_bytes;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.clk.begin(env_on("L2R_BED_TIMING"), c->check_stages))) return rc;
    const int64_t cig_base = r->cig_off[0], name_base = r->name_off[0];
    const size_t n_cig = (size_t)(r->cig_off[N] - cig_base), n_name = (size_t)(r->name_off[N] - name_base);
    const bool wave = wave_form((double)n_cig / (double)N, "L2R_BED_WAVE");
    m.stats[BEDS_WAVE] = wave ? 1 : 0;
    if ((rc = to_dev(c, m.flag, r->flag, N)) || (rc = to_dev(c, m.tid, r->tid, N)) || (rc = to_dev(c, m.pos, r->pos, N)) || (rc = to_dev(c, m.mapq, r->mapq, N)) ||
        (rc = to_dev(c, m.cig_off, r->cig_off, N + 1)) || (rc = to_dev(c, m.cig, n_cig ? r->cig + cig_base : nullptr, n_cig)) ||
        (rc = to_dev(c, m.name_off, r->name_off, N + 1)) || (rc = to_dev(c, m.names, n_name ? r->names + name_base : nullptr, n_name)) ||
        m.off.ensure(N + 1) || m.n_blocks.ensure(N) || m.span.ensure(N) || m.size_len.ensure(N) || m.word.ensure(BEDW_N)) rc = rc ? rc : -2;
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }      // (the columns are the caller's)
    HIP_TRY(hipMemsetAsync(m.word.p, 0, BEDW_N * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(m.word.p + BEDW_BAD, 0xff, sizeof(uint32_t), c->stream));
    BedIn in{};
    in.n = (int64_t)N; in.flag = m.flag.p; in.tid = m.tid.p; in.pos = m.pos.p; in.mapq = m.mapq.p;
    in.cig_off = m.cig_off.p; in.cig = m.cig.p; in.cig_base = cig_base; in.name_off = m.name_off.p; in.names = m.names.p; in.name_base = name_base;
    in.n_ref = m.prm.n_ref; in.ref_off = m.ref.off.p; in.ref_names = m.ref.names.p;
    in.color_len = (uint32_t)m.prm.color_len;
    {   uint32_t w[3] = {0, 0, 0};
        memcpy(w, m.prm.color, 12);
        in.color_w0 = w[0]; in.color_w1 = w[1]; in.color_w2 = w[2]; }
    const BedMeasure meas{m.off.p, m.n_blocks.p, m.span.p, m.size_len.p};
    rc = m.clk.launch(c, &m.stats[BEDS_K_MEASURE], [&] {
        const dim3 grid((unsigned)(((wave ? N * 64 : N) + 255) / 256));
        if (wave) hipLaunchKernelGGL(k_bed_measure<true>, grid, dim3(256), 0, c->stream, in, meas, m.word.p + BEDW_BAD);
        else hipLaunchKernelGGL(k_bed_measure<false>, grid, dim3(256), 0, c->stream, in, meas, m.word.p + BEDW_BAD);
    });
    if (!rc) rc = m.clk.launch(c, &m.stats[BEDS_K_SCAN], [&] { scan_u32(c, m.off.p, (int64_t)N, m.word.p + BEDW_TOTAL); });
    uint32_t w[BEDW_N] = {0, 0, 0};
    if ((rc = download_all(c, rc, {{w, m.word.p, sizeof w}}, "l2r_bed_lines"))) return rc;
    if (w[BEDW_BAD] != 0xffffffffu) {
        std::string msg;
        if ((size_t)w[BEDW_BAD] >= N || bed_record_error(r, &m.prm, (int64_t)w[BEDW_BAD], msg) == BED_OK) return fail(-2, "[l2r_bed_lines] the device names record %u of %zu", w[BEDW_BAD], N);
        return fail(-1, "%s", msg.c_str());
    }
    const size_t B = w[BEDW_TOTAL];
    if ((uint64_t)B >= BED_BATCH_BYTES) return fail(-2, "[l2r_bed_lines] %zu bytes of text behind a bound below 2^32 - 64", B);
    const unsigned n_tiles = (unsigned)((N + BED_TILE - 1) / BED_TILE);
    if (m.out.reserve(B)) return -2;
    uint8_t *text8 = m.out.bytes();
    HIP_TRY(m.out.arm_guard(c, B));
    if (B && (rc = m.clk.launch(c, &m.stats[BEDS_K_WRITE], [&] {
            hipLaunchKernelGGL(k_bed_write, dim3(n_tiles), dim3(BED_TILE), 0, c->stream, in, (const uint32_t *)m.off.p, (const uint32_t *)m.n_blocks.p, (const uint32_t *)m.span.p,
                               (const uint32_t *)m.size_len.p, text8, m.word.p + BEDW_DIRECT);
        }))) { (void)hipStreamSynchronize(c->stream); return rc; }
    uint32_t n_direct = 0;
    HIP_TRY(hipMemcpyAsync(&n_direct, m.word.p + BEDW_DIRECT, sizeof n_direct, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(m.out.fetch_guard(c, B));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!m.out.guard_intact(c)) m.stats[BEDS_GUARD] = 0;
    if (n_direct > n_tiles) return fail(-2, "[l2r_bed_lines] %u direct tiles of %u", n_direct, n_tiles);
    m.stats[BEDS_LINES] = (double)lines; m.stats[BEDS_BYTES] = (double)B;
    m.stats[BEDS_TILES_DIRECT] = (double)n_direct; m.stats[BEDS_TILES_LDS] = (double)(n_tiles - n_direct);
    m.out.take_device(B);
    *n_lines = lines; *n_bytes = (int64_t)B;
    return 0;
}

int l2r_bed_text_out(l2r_ctx *c, uint8_t *text, int64_t cap)
{
    if (!c) return fail(-1, "[l2r_bed_text_out] null argument");
    return text_out(c, c->bed.out, text, cap, "l2r_bed_text_out", "l2r_bed_lines", -1);
}

int l2r_bed_cut(const l2r_bed_records *r, const l2r_bed_params *p, int64_t first, int64_t max_records, int64_t max_bytes, int64_t *n_take)
{
    std::string msg;
    if (bed_cut(r, p, first, max_records, max_bytes, n_take, msg)) return fail(-1, "%s", msg.c_str());
    return 0;
}

int l2r_bed_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->bed.stats : nullptr, BEDS_N, out, n, "l2r_bed_stats"); }

// ---------------------------------------------------------------------------------------------- unique-gtf
static void uniq_on_host(UniqState &m, const l2r_uniq_trans *t, const UniqPrm &p, bool in_order)
{
    uniq_host(t, p, m.host);
    m.on_host = true; m.have = true; m.n_unique = (int64_t)m.host.u_src.size();
    m.stats[UQS_ROUTE] = 1; m.stats[UQS_UNIQUE] = (double)m.n_unique;
    m.stats[UQS_IDENT] = (double)m.host.hits[0]; m.stats[UQS_CONTAINED] = (double)m.host.hits[1]; m.stats[UQS_SINGLE] = (double)m.host.hits[2];
    m.stats[UQS_END_EXT] = (double)m.host.end_ext;
    if (in_order) {
        std::vector<uint8_t> head;
        int64_t n_c = 0, big = 0;
        uniq_clusters(t, head, &n_c, &big);
        m.stats[UQS_CLUSTERS] = (double)n_c; m.stats[UQS_LARGEST] = (double)big;
    }
}

// The device part of merge_trans over N > 0 transcripts whose columns already lie in HBM, in m.tid, m.rev, m.ex_off, m.xs and m.xe
// (l2r_uniq_merge uploads them, l2r_summary_finish gathers them there): the cluster cut, k_uniq_merge, k_uniq_take into m's buffers; the
// counter block comes back in w.  The stage timer m.clk is the caller's to arm; ms_*: where the device milliseconds of the three groups
// are added.  Where w[UQW_UNSORTED] is set -- (tid, start) descends somewhere -- nothing has been merged and the caller takes its exact host
// routine.  The stream has been waited for on every path out.
extern "C++" {
static int uniq_device(l2r_ctx *c, UniqState &m, size_t N, const UniqPrm &p, const char *who, double *ms_cut, double *ms_merge, double *ms_take, uint32_t *w)
{
    const size_t n_tiles = (N + UNIQ_TILE - 1) / UNIQ_TILE;
    int rc = 0;
    if (m.rec.ensure(N) || m.tile_max.ensure(n_tiles) || m.head.ensure(N + 1) || m.first.ensure(N + 1) || m.len.ensure(N + 1) || m.word.ensure(UQW_N) ||
        m.l_src.ensure(N) || m.l_start.ensure(N) || m.l_end.ensure(N) || m.l_cov.ensure(N) || m.uniq_of.ensure(N) || m.merged.ensure(N) ||
        m.u_src.ensure(N) || m.u_start.ensure(N) || m.u_end.ensure(N) || m.u_cov.ensure(N)) rc = -2;
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY_AS(who, hipMemsetAsync(m.word.p, 0, UQW_N * sizeof(uint32_t), c->stream));
    const UniqIn in{(int64_t)N, m.tid.p, m.rev.p, m.ex_off.p, m.xs.p, m.xe.p};
    rc = m.clk.launch(c, ms_cut, [&] {
        hipLaunchKernelGGL(k_uniq_heads, dim3((unsigned)n_tiles), dim3(UNIQ_TILE), 0, c->stream, in, m.rec.p, m.tile_max.p, m.word.p);
        hipLaunchKernelGGL(k_uniq_pmax, dim3(1), dim3(1024), 0, c->stream, m.tile_max.p, (int64_t)n_tiles);
        hipLaunchKernelGGL(k_uniq_cut, dim3((unsigned)n_tiles), dim3(UNIQ_TILE), 0, c->stream, (int64_t)N, (const int32_t *)m.tid.p, (const UniqRec *)m.rec.p,
                           (const uint64_t *)m.tile_max.p, m.head.p);
        scan_u32(c, m.head.p, (int64_t)N, m.word.p + UQW_CLUSTERS);
        hipLaunchKernelGGL(k_uniq_firsts, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (int64_t)N, (const uint32_t *)m.head.p, m.first.p);
    });
    if ((rc = download_all(c, rc, {{w, m.word.p, UQW_N * sizeof(uint32_t)}}, who))) return rc;
    if (w[UQW_UNSORTED]) return 0;
    const uint32_t C = w[UQW_CLUSTERS];
    if (C == 0 || (size_t)C > N) return fail(-2, "[%s] %u clusters of %zu transcripts", who, C, N);
    const UniqList L{m.l_src.p, m.l_start.p, m.l_end.p, m.l_cov.p};
    rc = m.clk.launch(c, ms_merge, [&] {
        hipLaunchKernelGGL(k_uniq_merge, dim3((C + UNIQ_WAVES - 1) / UNIQ_WAVES), dim3(UNIQ_WAVES * 64), 0, c->stream, in, (const UniqRec *)m.rec.p, (const uint32_t *)m.first.p, C, p, L,
                           m.len.p, m.merged.p, m.uniq_of.p, m.word.p);
    });
    if (!rc) rc = m.clk.launch(c, ms_take, [&] {
        scan_u32(c, m.len.p, (int64_t)C, m.word.p + UQW_UNIQUE);
        hipLaunchKernelGGL(k_uniq_take, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (int64_t)N, (const uint32_t *)m.head.p, (const uint32_t *)m.first.p,
                           (const uint32_t *)m.len.p, L, m.uniq_of.p, m.u_src.p, m.u_start.p, m.u_end.p, m.u_cov.p);
    });
    if ((rc = download_all(c, rc, {{w, m.word.p, UQW_N * sizeof(uint32_t)}}, who))) return rc;
    const uint64_t hits = (uint64_t)w[UQW_IDENT] + w[UQW_CONTAINED] + w[UQW_SINGLE];
    if ((size_t)w[UQW_UNIQUE] > N || w[UQW_UNIQUE] < C || hits + w[UQW_UNIQUE] != N) return fail(-2, "[%s] %u entries and %llu hits of %zu offers", who, w[UQW_UNIQUE], (unsigned long long)hits, N);
    return 0;
}
}

int l2r_uniq_merge(l2r_ctx *c, const l2r_params *prm, const l2r_uniq_trans *t, int64_t *n_unique)
{
    if (!c || !prm || !n_unique) return fail(-1, "[l2r_uniq_merge] null argument");
    UniqState &m = c->uniq;
    for (double &v : m.stats) v = 0;
    m.have = false; m.on_host = false; m.n = 0; m.n_unique = 0; m.host = UniqResult();
    {   std::string msg;
        if (uniq_check(t, msg)) return fail(-1, "%s", msg.c_str()); }
    *n_unique = 0;
    const size_t N = (size_t)t->n;
    const UniqPrm p = uniq_prm(prm);
    m.n = t->n; m.stats[UQS_ROWS] = (double)N;
    const bool want_host = route_is_host("L2R_UNIQ_ROUTE");         // (tests, the comparator; the device route is the default: DESIGN section 12)
    if (N == 0) { m.have = true; m.on_host = true; m.stats[UQS_ROUTE] = want_host ? 1 : 0; return 0; }
    if (want_host) { uniq_on_host(m, t, p, uniq_in_order(t)); *n_unique = m.n_unique; return 0; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    const size_t NX = (size_t)t->ex_off[N];
    if ((rc = to_dev(c, m.tid, t->tid, N)) || (rc = to_dev(c, m.rev, t->rev, N)) || (rc = to_dev(c, m.ex_off, t->ex_off, N + 1)) ||
        (rc = to_dev(c, m.xs, t->xs, NX)) || (rc = to_dev(c, m.xe, t->xe, NX))) { (void)hipStreamSynchronize(c->stream); return rc; }      // (the columns are the caller's)
    uint32_t w[UQW_N] = {0};
    if ((rc = uniq_device(c, m, N, p, "l2r_uniq_merge", &m.stats[UQS_K_CUT], &m.stats[UQS_K_MERGE], &m.stats[UQS_K_TAKE], w))) return rc;
    if (w[UQW_UNSORTED]) {                              // (tid, start) descends somewhere: the exact host routine
        for (int k = UQS_K_CUT; k < UQS_N; ++k) m.stats[k] = 0;
        uniq_on_host(m, t, p, false);
        *n_unique = m.n_unique;
        return 0;
    }
    m.n_unique = (int64_t)w[UQW_UNIQUE];
    m.stats[UQS_UNIQUE] = (double)w[UQW_UNIQUE]; m.stats[UQS_CLUSTERS] = (double)w[UQW_CLUSTERS]; m.stats[UQS_LARGEST] = (double)w[UQW_LARGEST]; m.stats[UQS_ROUTE] = 0;
    m.stats[UQS_IDENT] = (double)w[UQW_IDENT]; m.stats[UQS_CONTAINED] = (double)w[UQW_CONTAINED]; m.stats[UQS_SINGLE] = (double)w[UQW_SINGLE]; m.stats[UQS_END_EXT] = (double)w[UQW_END_EXT];
    m.have = true;
    *n_unique = m.n_unique;
    return 0;
}

int l2r_uniq_out(l2r_ctx *c, uint8_t *merged, int32_t *uniq_of, int32_t *u_src, int32_t *u_start, int32_t *u_end, int32_t *u_cov)
{
    if (!c) return fail(-1, "[l2r_uniq_out] null argument");
    const UniqState &m = c->uniq;
    if (!m.have) return fail(-1, "[l2r_uniq_out] no results: the last l2r_uniq_merge failed, or none was made");
    const size_t N = (size_t)m.n, U = (size_t)m.n_unique;
    if (m.on_host) {
        const UniqResult &r = m.host;
        if (merged && N) memcpy(merged, r.merged.data(), N);
        if (uniq_of && N) memcpy(uniq_of, r.uniq_of.data(), N * 4);
        if (u_src && U) memcpy(u_src, r.u_src.data(), U * 4);
        if (u_start && U) memcpy(u_start, r.u_start.data(), U * 4);
        if (u_end && U) memcpy(u_end, r.u_end.data(), U * 4);
        if (u_cov && U) memcpy(u_cov, r.u_cov.data(), U * 4);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return download_all(c, 0, {{merged, m.merged.p, merged ? N : 0}, {uniq_of, m.uniq_of.p, uniq_of ? N * 4 : 0}, {u_src, m.u_src.p, u_src ? U * 4 : 0},
                               {u_start, m.u_start.p, u_start ? U * 4 : 0}, {u_end, m.u_end.p, u_end ? U * 4 : 0}, {u_cov, m.u_cov.p, u_cov ? U * 4 : 0}}, "l2r_uniq_out");
}

int l2r_uniq_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->uniq.stats : nullptr, UQS_N, out, n, "l2r_uniq_stats"); }

// ---------------------------------------------------------------------------------------------- update-gtf -y: read classes and unique counts
int l2r_summary_begin(l2r_ctx *c, const l2r_params *prm)
{
    if (!c || !prm) return fail(-1, "[l2r_summary_begin] null argument");
    SummaryState &m = c->summary;
    m.p = uniq_prm(prm);
    m.on_host = route_is_host("L2R_SUMMARY_ROUTE");      // (tests, the comparator)
    m.n = 0; m.x = 0; m.adds = 0;
    m.tid.clear(); m.info.clear(); m.xs.clear(); m.xe.clear();
    m.h = SummaryState::Host();
    for (double &v : m.stats) v = 0;
    m.stats[SMS_ROUTE] = m.on_host ? 1 : 0;
    m.begun = true;
    return 0;
}

// a buffer could not be had (the text of the failed allocation is in g_err): the stream waited for, -2 under the entry point's name
static int summary_no_room(l2r_ctx *c, const char *who)
{
    const std::string why = g_err;
    (void)hipStreamSynchronize(c->stream);
    return fail(-2, "[%s] %s", who, why.c_str());
}

int l2r_summary_add(l2r_ctx *c, const l2r_summary_reads *r)
{
    if (!c || !r) return fail(-1, "[l2r_summary_add] null argument");
    SummaryState &m = c->summary;
    if (!m.begun) return fail(-1, "[l2r_summary_add] no l2r_summary_begin in front");
    {   std::string msg;
        if (summary_check_result(r->n, r->tid, r->res, msg)) return fail(-1, "%s", msg.c_str()); }
    const size_t N = (size_t)r->n;
    if (N == 0) { ++m.adds; m.stats[SMS_ADDS] = (double)m.adds; return 0; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const bool run_res = !r->res;
    if (run_res) {
        if (!c->ran) return fail(-1, "[l2r_summary_add] no completed run on this context");
        if ((rc = fetch_totals(c))) return rc;
        if (!(c->want & L2R_WANT_RESULTS)) return fail(-1, "[l2r_summary_add] the last run kept no results (l2r_set_outputs without L2R_WANT_RESULTS)");
        if (r->n != c->n_reads) return fail(-1, "[l2r_summary_add] %lld reads, the last run had %lld", (long long)r->n, (long long)c->n_reads);
    }
    const size_t X = run_res ? (size_t)c->h_totals[0] : (size_t)r->res->n_exons;
    {   std::string msg;
        if (summary_check_totals(m.n, m.x, r->n, (int64_t)X, msg)) return fail(-1, "%s", msg.c_str()); }
    const size_t n0 = (size_t)m.n, x0 = (size_t)m.x;
    if (m.on_host) {
        SummaryState::Host &h = m.h;
        try { h.tid.reserve(n0 + N); h.info.reserve(n0 + N); h.xs.reserve(x0 + X); h.xe.reserve(x0 + X); }
        catch (const std::bad_alloc &) { return fail(-2, "[l2r_summary_add] no memory for %zu reads, %zu exons", n0 + N, x0 + X); }
        if (run_res) {
            std::vector<int64_t> off(N + 1); std::vector<uint8_t> f(X ? X : 1); std::vector<int32_t> ref(N);
            h.info.resize(n0 + N); h.xs.resize(x0 + X); h.xe.resize(x0 + X);
            l2r_result res{(int64_t)N, (int64_t)X, 0, off.data(), h.xs.data() + x0, h.xe.data() + x0, f.data(), h.info.data() + n0, ref.data()};
            if ((rc = l2r_download(c, &res))) { h.info.resize(n0); h.xs.resize(x0); h.xe.resize(x0); return rc; }
        } else {
            h.info.insert(h.info.end(), r->res->info, r->res->info + N);
            h.xs.insert(h.xs.end(), r->res->ex_start, r->res->ex_start + X); h.xe.insert(h.xe.end(), r->res->ex_end, r->res->ex_end + X);
        }
        h.tid.insert(h.tid.end(), r->tid, r->tid + N);
    } else {
        // room first: a failed allocation leaves the accumulators as they were
        if (m.tid.reserve(c->stream, n0 + N) || m.info.reserve(c->stream, n0 + N) || m.xs.reserve(c->stream, x0 + X) || m.xe.reserve(c->stream, x0 + X)) return summary_no_room(c, "l2r_summary_add");
        const hipMemcpyKind kind = run_res ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const uint32_t *info = run_res ? c->info.p : r->res->info;
        const int32_t *xs = run_res ? c->ex_start.p : r->res->ex_start, *xe = run_res ? c->ex_end.p : r->res->ex_end;
        hipError_t e = hipMemcpyAsync(m.tid.p + n0, r->tid, N * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(m.info.p + n0, info, N * 4, kind, c->stream);
        if (e == hipSuccess && X) e = hipMemcpyAsync(m.xs.p + x0, xs, X * 4, kind, c->stream);
        if (e == hipSuccess && X) e = hipMemcpyAsync(m.xe.p + x0, xe, X * 4, kind, c->stream);
        const hipError_t sync = hipStreamSynchronize(c->stream);      // (the columns are the caller's)
        if (e == hipSuccess) e = sync;
        if (e != hipSuccess) return fail(-2, "[l2r_summary_add] %s", hipGetErrorString(e));
        m.tid.n = m.info.n = n0 + N; m.xs.n = m.xe.n = x0 + X;
    }
    m.n += (int64_t)N; m.x += (int64_t)X; ++m.adds;
    m.stats[SMS_READS] = (double)m.n; m.stats[SMS_EXONS] = (double)m.x; m.stats[SMS_ADDS] = (double)m.adds;
    return 0;
}

extern "C++" {
// summary_host over the host's copies of the accumulated reads (the checks first: -1 names the read)
static int summary_on_host(SummaryState &m, const SummaryState::Host &h, bool checked, int64_t *counts)
{
    const size_t N = (size_t)m.n;
    std::vector<int64_t> off(N + 1, 0);
    for (size_t i = 0; i < N; ++i) off[i + 1] = off[i] + (int64_t)L2R_INFO_NEXON(h.info[i]);
    if (off[N] != m.x) return fail(-2, "[l2r_summary_finish] the exon counts add up to %lld, %lld exons were added", (long long)off[N], (long long)m.x);
    const SummaryReads r{m.n, h.tid.data(), h.info.data(), off.data(), h.xs.data(), h.xe.data()};
    if (!checked) { std::string msg; if (summary_check(r, msg)) return fail(-1, "%s", msg.c_str()); }
    summary_host(r, m.p, counts);
    m.stats[SMS_ROUTE] = 1;
    return 0;
}

// what a word of k_sum_class / k_sum_gather names: -1 and the text of the host route, or the device's inconsistency
static int summary_bad_read(unsigned long long w, size_t N)
{
    const unsigned long long q = w >> 4; const int kind = (int)(w & 15ull);
    if (q >= N || kind <= 0 || kind >= SUM_E_N) return fail(-2, "[l2r_summary_finish] the device names read %llu of %zu, kind %d", q, N, kind);
    std::string msg; summary_read_fail(msg, (int64_t)q, kind);
    return fail(-1, "%s", msg.c_str());
}
}

int l2r_summary_finish(l2r_ctx *c, int64_t *counts)
{
    if (!c || !counts) return fail(-1, "[l2r_summary_finish] null argument");
    SummaryState &m = c->summary;
    if (!m.begun) return fail(-1, "[l2r_summary_finish] no l2r_summary_begin in front");
    for (int k = 0; k < 2 * SUM_CLASSES; ++k) counts[k] = 0;
    for (int k = SMS_CLUSTERS; k < SMS_N; ++k) m.stats[k] = 0;
    const size_t N = (size_t)m.n, X = (size_t)m.x;
    if (N == 0) return 0;
    if (m.on_host) return summary_on_host(m, m.h, false, counts);
    HIP_TRY(hipSetDevice(c->device));
    UniqState &u = m.u;
    int rc;
    if ((rc = u.clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    const size_t n_tiles = (N + SUM_TILE - 1) / SUM_TILE;
    if (m.cls.ensure(N) || m.src_off.ensure(N + 1) || m.tile_cnt.ensure(SUM_CLASSES * n_tiles + 1) || m.dst_off.ensure(N + 1) || m.src.ensure(N) || m.word.ensure(SUMW_N) || m.bad.ensure(1) ||
        u.tid.ensure(N) || u.rev.ensure(N) || u.ex_off.ensure(N + 1) || u.xs.ensure(X ? X : 1) || u.xe.ensure(X ? X : 1)) return summary_no_room(c, "l2r_summary_finish");
    HIP_TRY(hipMemsetAsync(m.bad.p, 0xff, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(m.word.p, 0, SUMW_N * sizeof(uint32_t), c->stream));
    rc = u.clk.launch(c, &m.stats[SMS_K_CLASS], [&] {
        hipLaunchKernelGGL(k_sum_class, dim3((unsigned)n_tiles), dim3(SUM_TILE), 0, c->stream, (int64_t)N, (const int32_t *)m.tid.p, (const uint32_t *)m.info.p, m.cls.p, m.src_off.p, m.tile_cnt.p,
                           (int64_t)n_tiles, m.bad.p);
        scan_u32(c, m.src_off.p, (int64_t)N, m.word.p + SUMW_EXONS);
        scan_u32(c, m.tile_cnt.p, (int64_t)(SUM_CLASSES * n_tiles), m.word.p + SUMW_TILES);
        hipLaunchKernelGGL(k_sum_place, dim3((unsigned)n_tiles), dim3(SUM_TILE), 0, c->stream, (int64_t)N, (const int32_t *)m.tid.p, (const uint32_t *)m.info.p, (const uint8_t *)m.cls.p,
                           (const uint32_t *)m.tile_cnt.p, (int64_t)n_tiles, u.tid.p, u.rev.p, m.dst_off.p, m.src.p);
        scan_u32(c, m.dst_off.p, (int64_t)N, m.word.p + SUMW_PLACED);
    });
    uint32_t w[SUMW_N] = {0};
    unsigned long long bad = ~0ull;
    // (a read k_sum_class has flagged is not reported yet: k_sum_gather may flag a smaller one, and neither harms it -- a read without
    // exons copies nothing, a tid outside the domain is a key like any other; the totals below are what keeps its copies inside the arrays)
    if ((rc = download_all(c, rc, {{w, m.word.p, sizeof w}}, "l2r_summary_finish"))) return rc;
    if ((size_t)w[SUMW_TILES] != N || (size_t)w[SUMW_EXONS] != X || (size_t)w[SUMW_PLACED] != X)
        return fail(-2, "[l2r_summary_finish] %u reads placed of %zu, %u and %u exons counted of %zu", w[SUMW_TILES], N, w[SUMW_EXONS], w[SUMW_PLACED], X);
    const bool wave = wave_form((double)X / (double)N, "L2R_SUMMARY_WAVE");
    m.stats[SMS_WAVE] = wave ? 1 : 0;
    const SumGather g{(int64_t)N, m.src.p, m.src_off.p, m.dst_off.p, m.xs.p, m.xe.p, (uint32_t)X, u.ex_off.p, u.xs.p, u.xe.p, m.bad.p};
    rc = u.clk.launch(c, &m.stats[SMS_K_GATHER], [&] {
        const dim3 grid((unsigned)(((wave ? N * 64 : N) + 255) / 256));
        if (wave) hipLaunchKernelGGL(k_sum_gather<true>, grid, dim3(256), 0, c->stream, g);
        else hipLaunchKernelGGL(k_sum_gather<false>, grid, dim3(256), 0, c->stream, g);
    });
    if ((rc = download_all(c, rc, {{&bad, m.bad.p, sizeof bad}}, "l2r_summary_finish"))) return rc;
    if (bad != ~0ull) return summary_bad_read(bad, N);
    uint32_t uw[UQW_N] = {0};
    if ((rc = uniq_device(c, u, N, m.p, "l2r_summary_finish", &m.stats[SMS_K_CUT], &m.stats[SMS_K_MERGE], &m.stats[SMS_K_TAKE], uw))) return rc;
    if (uw[UQW_UNSORTED]) {                             // a class's (tid, start) descends somewhere: the accumulated columns fetched, the exact host routine
        for (int k = SMS_K_CLASS; k < SMS_N; ++k) m.stats[k] = 0;
        SummaryState::Host h;
        h.tid.resize(N); h.info.resize(N); h.xs.resize(X ? X : 1); h.xe.resize(X ? X : 1);
        if ((rc = download_all(c, 0, {{h.tid.data(), m.tid.p, N * 4}, {h.info.data(), m.info.p, N * 4}, {h.xs.data(), m.xs.p, X * 4}, {h.xe.data(), m.xe.p, X * 4}}, "l2r_summary_finish"))) return rc;
        return summary_on_host(m, h, true, counts);
    }
    rc = u.clk.launch(c, &m.stats[SMS_K_TAKE], [&] {
        hipLaunchKernelGGL(k_sum_count, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, (int64_t)N, (const int32_t *)u.tid.p, (const uint8_t *)u.merged.p, m.word.p);
    });
    if ((rc = download_all(c, rc, {{w, m.word.p, sizeof w}}, "l2r_summary_finish"))) return rc;
    uint64_t reads = 0, uniq = 0;
    for (int k = 0; k < SUM_CLASSES; ++k) { reads += w[SUMW_READS + k]; uniq += w[SUMW_UNIQUE + k]; }
    if (reads != N || uniq != uw[UQW_UNIQUE]) return fail(-2, "[l2r_summary_finish] %llu reads counted of %zu, %llu pushed offers of %u entries", (unsigned long long)reads, N, (unsigned long long)uniq, uw[UQW_UNIQUE]);
    for (int k = 0; k < SUM_CLASSES; ++k) { counts[k] = (int64_t)w[SUMW_READS + k]; counts[SUM_CLASSES + k] = (int64_t)w[SUMW_UNIQUE + k]; }
    m.stats[SMS_ROUTE] = 0; m.stats[SMS_CLUSTERS] = (double)uw[UQW_CLUSTERS]; m.stats[SMS_LARGEST] = (double)uw[UQW_LARGEST];
    return 0;
}

int l2r_summary_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->summary.stats : nullptr, SMS_N, out, n, "l2r_summary_stats"); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------- what the text commands below share (outside the C linkage block: two take a callable)
// The reads of l2r_detail_rows (noun "rows") and of l2r_gtftext_reads ("reads", which alone has a tid_name) into `rr`: the checks against
// the last run where they came without results, the host route's copies or the uploads.  The uploads are queued (with no reads still a
// names table's) and the columns the caller's: it waits for the stream on every path out; a failure here has waited.  arg_code: of an
// error of arguments or order.
static int take_reads(l2r_ctx *c, ReadRows &rr, const l2r_gtx_reads &r, bool on_host, const char *who, int arg_code, const char *noun)
{
    const size_t N = (size_t)r.n, NL = (size_t)r.names_len;
    rr.n = r.n; rr.names_len = r.names_len; rr.run_res = !r.res; rr.exons_per_read = 0;
    int rc = 0;
    if (rr.run_res) {
        if (!c->ran) return fail(arg_code, "[%s] no completed run on this context", who);
        if ((rc = fetch_totals(c))) return rc;
        if (!(c->want & L2R_WANT_RESULTS)) return fail(arg_code, "[%s] the last run kept no results (l2r_set_outputs without L2R_WANT_RESULTS)", who);
        if (r.n != c->n_reads) return fail(arg_code, "[%s] %lld %s, the last run had %lld reads", who, (long long)r.n, noun, (long long)c->n_reads);
        if (N) rr.exons_per_read = (double)c->h_totals[0] / (double)N;
    } else if (N) rr.exons_per_read = (double)r.res->n_exons / (double)N;
    const l2r_result *s = r.res; const bool two_names = r.tid_name && r.tid_name != r.qname;
    if (on_host) {
        ReadRows::Host &h = rr.h;
        h.tid.assign(r.tid, r.tid + N); h.qname.assign(r.qname, r.qname + N); h.names.assign(r.names, r.names + NL);
        if (two_names) h.tid_name.assign(r.tid_name, r.tid_name + N); else h.tid_name.clear();
        const size_t X = rr.run_res ? (size_t)c->h_totals[0] : (size_t)s->n_exons;
        h.ex_off.assign(N + 1, 0); h.info.assign(N ? N : 1, 0u); h.ref_tx.assign(N ? N : 1, 0); h.xs.assign(X ? X : 1, 0); h.xe.assign(X ? X : 1, 0); h.f.assign(X ? X : 1, 0);
        h.res = l2r_result{(int64_t)N, (int64_t)X, (int64_t)X, h.ex_off.data(), h.xs.data(), h.xe.data(), h.f.data(), h.info.data(), h.ref_tx.data()};
        if (rr.run_res) { if (N && (rc = l2r_download(c, &h.res))) return rc; }
        else if (N) {
            memcpy(h.ex_off.data(), s->ex_off, (N + 1) * 8); memcpy(h.info.data(), s->info, N * 4); memcpy(h.ref_tx.data(), s->ref_tx, N * 4);
            if (X) { memcpy(h.xs.data(), s->ex_start, X * 4); memcpy(h.xe.data(), s->ex_end, X * 4); memcpy(h.f.data(), s->ex_flag, X); }
        }
        return 0;
    }
    if ((rc = to_dev(c, rr.tid, r.tid, N)) || (rc = to_dev(c, rr.qname, r.qname, N)) || (rc = to_dev(c, rr.names, r.names, NL))) {}
    rr.tid_name_p = rr.qname.p;
    if (!rc && two_names) { rc = to_dev(c, rr.tid_name, r.tid_name, N); rr.tid_name_p = rr.tid_name.p; }
    if (!rc && !rr.run_res) {
        const size_t X = (size_t)s->n_exons;
        rr.off32.resize(N);
        for (size_t i = 0; i < N; ++i) rr.off32[i] = (uint32_t)s->ex_off[i];
        if ((rc = put_dev(c, rr.ex_off, rr.off32)) || (rc = to_dev(c, rr.info, (const uint32_t *)s->info, N)) || (rc = to_dev(c, rr.ref_tx, (const int32_t *)s->ref_tx, N)) ||
            (rc = to_dev(c, rr.xs, (const int32_t *)s->ex_start, X)) || (rc = to_dev(c, rr.xe, (const int32_t *)s->ex_end, X)) || (rc = to_dev(c, rr.f, (const uint8_t *)s->ex_flag, X))) {}
    }
    if (rc) (void)hipStreamSynchronize(c->stream);                  // (the columns are the caller's)
    return rc;
}

// The result columns the kernels read: those of the context's last run, or the uploaded ones in the same layout
struct ResultCols { const uint32_t *ex_off, *info; const int32_t *xs, *xe, *ref_tx; const uint8_t *f; };
static ResultCols result_cols(const l2r_ctx *c, const ReadRows &r)
{
    return r.run_res ? ResultCols{c->ex_off.p, c->info.p, c->ex_start.p, c->ex_end.p, c->ref_tx.p, c->ex_flag.p} : ResultCols{r.ex_off.p, r.info.p, r.xs.p, r.xe.p, r.ref_tx.p, r.f.p};
}

// The tail of a measure step (k_gtx_measure, k_rl_measure, k_detail_measure).  The kernels leave the smallest bad item << 4 | the kind of
// its domain error in d_word[0], by atomicMin over a word of ones: the word is armed (the words behind it, n_words in all, are zeroed: the
// GTF measures count their lines in a second one), `launch` runs under the stage timer, the words come back to w with the lengths of
// h_len's items, *bytes is their sum.  A word that names no item or no kind is the device's inconsistency (-2); a domain error is -1 and
// the text of item_fail, as on the host route.  The stream has been waited for in any case.
template <typename Launch>
static int measure_tail(l2r_ctx *c, StageTimer &clk, double *ms, unsigned long long *d_word, unsigned long long *w, size_t n_words, std::vector<uint32_t> &h_len, const uint32_t *d_len,
                        const char *who, const char *item, int n_kinds, int (*item_fail)(std::string &, int64_t, int), uint64_t *bytes, Launch launch)
{
    const size_t M = h_len.size();
    hipError_t e = hipMemsetAsync(d_word, 0xff, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess && n_words > 1) e = hipMemsetAsync(d_word + 1, 0, (n_words - 1) * sizeof(unsigned long long), c->stream);
    int rc = e == hipSuccess ? clk.launch(c, ms, launch) : fail(-2, "[%s] %s", who, hipGetErrorString(e));
    if ((rc = download_all(c, rc, {{w, d_word, n_words * sizeof(unsigned long long)}, {h_len.data(), d_len, M * 4}}, who))) return rc;
    if (w[0] != ~0ull) {
        const unsigned long long q = w[0] >> 4; const int kind = (int)(w[0] & 15ull);
        if (q >= M || kind <= 0 || kind >= n_kinds) return fail(-2, "[%s] the device names %s %llu of %zu, kind %d", who, item, q, M, kind);
        std::string msg; item_fail(msg, (int64_t)q, kind);
        return fail(-1, "%s", msg.c_str());
    }
    for (size_t q = 0; q < M; ++q) *bytes += h_len[q];
    return 0;
}

// slots that l2r_gtftext_stats and l2r_detail_stats have in common: those of a batch
enum { TXS_LINES = 1, TXS_BYTES, TXS_WAVE, TXS_TILES_LDS, TXS_TILES_DIRECT, TXS_ROUTE, TXS_GUARD, TXS_BATCHES, TXS_K_MEASURE, TXS_K_SCAN, TXS_K_WRITE };

// What l2r_gtftext_lines and l2r_detail_lines differ in, beside their write kernels and host routines
struct TextBatch {
    const char *who, *timing, *disagree;    // the entry point; the switch of its stage timer; what a count of `outside` says
    int tile, total, outside, direct;       // items of a workgroup of the write kernel; counter words: the scan's total (behind the kernel's own), what left its place, the direct tiles
};

// One batch of text, behind l2r_gtftext_lines and l2r_detail_lines: the items [first, first + take) of `sum` bytes, as the caller cut them
// from the measured lengths, into `out`.  Host route: compose(host_text, msg) is the exact host routine.  Device route: the batch's
// lengths are scanned into `off`, the guard armed, write(n_tiles, text) launches the write kernel, and its counters come back to
// w[0 .. t.total] with the guard; three of them are checked here, the rest is the caller's.  stats: the TXS_* slots but the lines.
template <typename Compose, typename Write>
static int text_batch(l2r_ctx *c, const TextBatch &t, TextOut &out, StageTimer &clk, const DevBuf<uint32_t> &len, DevBuf<uint32_t> &off, DevBuf<uint32_t> &word, double *stats,
                      bool on_host, int64_t first, int64_t take, int64_t sum, uint32_t *w, Compose compose, Write write)
{
    const size_t B = (size_t)sum, K = (size_t)take, W = (size_t)t.total + 1;
    stats[TXS_LINES] = 0; stats[TXS_BYTES] = 0; stats[TXS_TILES_LDS] = 0; stats[TXS_TILES_DIRECT] = 0;
    if (on_host) {
        std::string msg;
        if (compose(out.host_text, msg)) { out.host_text.clear(); return fail(-1, "%s", msg.c_str()); }
        if (out.host_text.size() != B) return fail(-5, "[%s] %zu bytes of text, measured %zu", t.who, out.host_text.size(), B);
        out.take_host();
        stats[TXS_BYTES] = (double)B; stats[TXS_BATCHES] += 1;
        return 0;
    }
    HIP_TRY_AS(t.who, hipSetDevice(c->device));
    int rc;
    if ((rc = clk.begin(env_on(t.timing), c->check_stages))) return rc;
    if (off.ensure(K + 1) || out.reserve(B) || word.ensure(W)) return -2;
    HIP_TRY_AS(t.who, hipMemcpyAsync(off.p, len.p + first, K * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY_AS(t.who, hipMemsetAsync(word.p, 0, W * sizeof(uint32_t), c->stream));
    if ((rc = clk.launch(c, &stats[TXS_K_SCAN], [&] { scan_u32(c, off.p, (int64_t)K, word.p + t.total); }))) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY_AS(t.who, out.arm_guard(c, B));
    const unsigned n_tiles = (unsigned)((K + (size_t)t.tile - 1) / (size_t)t.tile);
    if ((rc = clk.launch(c, &stats[TXS_K_WRITE], [&] { write(n_tiles, out.bytes()); }))) { (void)hipStreamSynchronize(c->stream); return rc; }
    hipError_t e = hipMemcpyAsync(w, word.p, W * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = out.fetch_guard(c, B);
    const hipError_t sync = hipStreamSynchronize(c->stream);       // (w is the caller's)
    if (e == hipSuccess) e = sync;
    if (e != hipSuccess) return fail(-2, "[%s] %s", t.who, hipGetErrorString(e));
    if (!out.guard_intact(c)) stats[TXS_GUARD] = 0;
    if ((size_t)w[t.total] != B) return fail(-5, "[%s] the scan left %u bytes, the cut %zu", t.who, w[t.total], B);
    if (w[t.outside]) return fail(-5, "[%s] %u %s", t.who, w[t.outside], t.disagree);
    if (w[t.direct] > n_tiles) return fail(-5, "[%s] %u direct tiles of %u", t.who, w[t.direct], n_tiles);
    stats[TXS_BYTES] = (double)B; stats[TXS_BATCHES] += 1;
    stats[TXS_TILES_DIRECT] = (double)w[t.direct]; stats[TXS_TILES_LDS] = (double)(n_tiles - w[t.direct]);
    out.take_device(B);
    return 0;
}

extern "C" {
// ---------------------------------------------------------------------------------------------- the GTF text of bam2gtf / unique-gtf
// slots of l2r_gtftext_stats
enum { GXS_BLOCKS = 0, GXS_LINES, GXS_BYTES, GXS_WAVE, GXS_TILES_LDS, GXS_TILES_DIRECT, GXS_ROUTE, GXS_GUARD, GXS_BATCHES, GXS_K_MEASURE, GXS_K_SCAN, GXS_K_WRITE, GXS_K_SELECT, GXS_PIECES, GXS_N };
static_assert(GXS_N == sizeof(GtxState::stats) / sizeof(double) && GXS_K_MEASURE == 9, "l2r_gtftext_stats: the words of include/lr2rmats_hip.h");
constexpr int GTXC_TOTAL = GTXC_N;                      // GtxState::word: k_gtx_write's counters, then the scan's total
constexpr int GTX_E_ARG = -4;                           // arguments, order of calls: not -1, which is a domain error (the commands fall back on it)

int l2r_gtftext_begin(l2r_ctx *c, const l2r_gtx_params *p)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_begin] null argument");
    GtxState &m = c->gtx;
    m.begun = false; m.have_rows = false; m.have_blocks = false; m.out.have = false;
    m.rl.have_anno = false; m.rl.have_reads = false; m.rl.active = false;
    for (double &v : m.stats) v = 0;
    {   std::string msg;
        if (gtx_check_params(p, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    m.ref.set(p->n_ref, p->ref_off, p->ref_names);
    m.h_src.assign((size_t)p->src_len + 1, 0);
    if (p->src_len) memcpy(m.h_src.data(), p->src, (size_t)p->src_len);
    m.prm = *p;
    m.prm.ref_off = m.ref.h_off.data(); m.prm.ref_names = m.ref.h_names.data(); m.prm.src = m.h_src.data();
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.ref.upload(c)) || (rc = put_dev(c, m.src, m.h_src))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.begun = true;
    return 0;
}

// the exon chains of the last run for the host route: ex_off from the exon counts, xs / xe as they lie
static int gtx_fetch_chains(l2r_ctx *c, GtxState &m)
{
    const size_t N = (size_t)c->n_reads, X = c->h_totals[0];
    std::vector<uint32_t> info(N ? N : 1);
    m.h.xs.assign(X ? X : 1, 0); m.h.xe.assign(X ? X : 1, 0);
    if (N) HIP_TRY(hipMemcpyAsync(info.data(), c->info.p, N * 4, hipMemcpyDeviceToHost, c->stream));
    if (X) {
        HIP_TRY(hipMemcpyAsync(m.h.xs.data(), c->ex_start.p, X * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(m.h.xe.data(), c->ex_end.p, X * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.h.ex_off.assign(N + 1, 0);
    for (size_t i = 0; i < N; ++i) m.h.ex_off[i + 1] = m.h.ex_off[i] + (int64_t)(info[i] >> 8);
    if ((size_t)m.h.ex_off[N] != X) return fail(-5, "[l2r_gtftext_rows] exon counts (%lld) do not add up to the exon total (%zu)", (long long)m.h.ex_off[N], X);
    return 0;
}

int l2r_gtftext_rows(l2r_ctx *c, const l2r_gtx_rows *r)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_rows] null argument");
    GtxState &m = c->gtx;
    m.have_rows = false; m.have_blocks = false; m.out.have = false;
    m.rl.have_reads = false; m.rl.active = false;
    if (!m.begun) return fail(GTX_E_ARG, "[l2r_gtftext_rows] no l2r_gtftext_begin in front");
    {   std::string msg;
        if (gtx_check_rows(r, m.prm.form, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    m.on_host = route_is_host("L2R_GTX_ROUTE");
    m.stats[GXS_ROUTE] = m.on_host ? 1 : 0;
    const size_t N = (size_t)r->n, NL = (size_t)r->names_len;
    const int n_names = m.prm.form == L2R_GTX_READ ? 4 : 2;
    const uint32_t *col[4] = {r->gid, r->tids, r->gname, r->tname};
    m.n = r->n; m.names_len = r->names_len; m.run_chains = N > 0 && !r->xs;
    HIP_TRY(hipSetDevice(c->device));
    int rc = 0;
    if (m.run_chains) {
        if ((rc = fetch_totals(c))) return rc;
        if (!(c->want & L2R_WANT_RESULTS)) return fail(GTX_E_ARG, "[l2r_gtftext_rows] the last run kept no exon chains (l2r_set_outputs without L2R_WANT_RESULTS)");
        if (r->n != c->n_reads) return fail(GTX_E_ARG, "[l2r_gtftext_rows] %lld transcripts, the last run had %lld reads", (long long)r->n, (long long)c->n_reads);
        m.exons_per_row = (double)c->h_totals[0] / (double)N;
        m.h_nex.clear();
    } else {
        m.h_nex.resize(N);
        for (size_t i = 0; i < N; ++i) m.h_nex[i] = (uint32_t)(r->ex_off[i + 1] - r->ex_off[i]);
    }
    if (m.on_host) {
        GtxState::Host &h = m.h;
        h.tid.assign(r->tid, r->tid + N); h.rev.assign(r->rev, r->rev + N);
        h.names.assign(r->names, r->names + NL);
        for (int k = 0; k < 4; ++k) { if (k < n_names && N) h.id[k].assign(col[k], col[k] + N); else h.id[k].clear(); }
        if (m.run_chains) { if ((rc = gtx_fetch_chains(c, m))) return rc; }
        else if (N) { const size_t X = (size_t)r->ex_off[N]; h.ex_off.assign(r->ex_off, r->ex_off + N + 1); h.xs.assign(r->xs, r->xs + X); h.xe.assign(r->xe, r->xe + X); }
        m.have_rows = true;
        return 0;
    }
    if ((rc = to_dev(c, m.tid, r->tid, N)) || (rc = to_dev(c, m.rev, r->rev, N)) || (rc = to_dev(c, m.names, r->names, NL))) { (void)hipStreamSynchronize(c->stream); return rc; }
    for (int k = 0; k < 4 && !rc; ++k) {
        m.id_p[k] = nullptr;
        if (k >= n_names || !N) continue;
        for (int j = 0; j < k; ++j) if (col[j] == col[k]) m.id_p[k] = m.id_p[j];
        if (!m.id_p[k]) { rc = to_dev(c, m.id[k], col[k], N); m.id_p[k] = m.id[k].p; }
    }
    if (!rc && !m.run_chains && N) {
        const size_t X = (size_t)r->ex_off[N];
        if ((rc = to_dev(c, m.ex_off, r->ex_off, N + 1)) || (rc = to_dev(c, m.xs, r->xs, X)) || (rc = to_dev(c, m.xe, r->xe, X))) {}
    }
    const hipError_t sync = hipStreamSynchronize(c->stream);           // (the columns are the caller's)
    if (rc) return rc;
    if (sync != hipSuccess) return fail(-2, "[l2r_gtftext_rows] %s", hipGetErrorString(sync));
    m.have_rows = true;
    return 0;
}

// the kernels' view of the rows and the selection
static GtxIn gtx_in(const l2r_ctx *c, const GtxState &m)
{
    GtxIn in{};
    in.n = m.n; in.m = m.m; in.tid = m.tid.p; in.rev = m.rev.p;
    if (m.run_chains) { in.ex_off32 = c->ex_off.p; in.info = c->info.p; in.xs = c->ex_start.p; in.xe = c->ex_end.p; }
    else { in.ex_off64 = m.ex_off.p; in.xs = m.xs.p; in.xe = m.xe.p; }
    in.names = m.names.p; in.names_len = m.names_len;
    for (int k = 0; k < 4; ++k) in.id[k] = m.id_p[k];
    in.sel = m.has_sel ? m.sel.p : nullptr; in.start = m.has_start ? m.start.p : nullptr; in.end = m.has_end ? m.end.p : nullptr; in.cov = m.has_cov ? m.cov.p : nullptr;
    in.n_ref = m.prm.n_ref; in.ref_off = m.ref.off.p; in.ref_names = m.ref.names.p; in.src = m.src.p; in.src_len = (uint32_t)m.prm.src_len; in.form = m.prm.form;
    return in;
}
// ... and the host route's, over its copies
static void gtx_host_view(const GtxState &m, l2r_gtx_rows &r, GtxChains &cx, l2r_gtx_blocks &b)
{
    const GtxState::Host &h = m.h;
    r = l2r_gtx_rows{m.n, h.tid.data(), h.rev.data(), h.ex_off.data(), h.xs.data(), h.xe.data(), m.names_len, h.names.data(),
                     h.id[0].data(), h.id[1].data(), h.id[2].data(), h.id[3].data()};
    cx = GtxChains{h.ex_off.data(), h.xs.data(), h.xe.data()};
    b = l2r_gtx_blocks{m.m, m.has_sel ? h.sel.data() : nullptr, m.has_start ? h.start.data() : nullptr, m.has_end ? h.end.data() : nullptr, m.has_cov ? h.cov.data() : nullptr};
}

// the kernels' view of the reads and the selection of a list
static RlIn rl_in(const l2r_ctx *c, const GtxState &m)
{
    const GtxState::Lists &l = m.rl;
    RlIn in{};
    const ReadRows &r = l.reads;
    const ResultCols v = result_cols(c, r);
    in.n = r.n; in.m = m.m; in.tid = r.tid.p; in.names = r.names.p; in.names_len = r.names_len; in.qname = r.qname.p; in.tid_name = r.tid_name_p;
    in.ex_off = v.ex_off; in.info = v.info; in.xs = v.xs; in.xe = v.xe; in.ref_tx = v.ref_tx; in.f = v.f;
    in.n_tx = l.anno.n_tx; in.anno_len = l.anno.anno_names_len; in.anno = l.genes.names.p; in.tx_gid = l.genes.gid.p; in.tx_gname = l.genes.gname.p;
    in.b_read = l.b_read.p; in.b_first = l.b_first.p; in.b_count = l.b_count.p; in.b_piece = l.b_piece.p;
    in.n_ref = m.prm.n_ref; in.ref_off = m.ref.off.p; in.ref_names = m.ref.names.p; in.src = m.src.p; in.src_len = (uint32_t)m.prm.src_len;
    in.list = l.list; in.has_sj = l.has_sj; in.split = l.split;
    return in;
}
// ... and the host route's, over its copies
static RlReads rl_host_view(const GtxState &m)
{
    const ReadRows &r = m.rl.reads;
    const ReadRows::Host &h = r.h;
    return RlReads{r.n, h.tid.data(), r.names_len, h.names.data(), h.qname.data(), h.tid_name_or_qname(), h.ex_off.data(), h.info.data(), h.ref_tx.data(),
                   h.xs.data(), h.xe.data(), h.f.data(), m.rl.has_sj, m.rl.split};
}

int l2r_gtftext_blocks(l2r_ctx *c, const l2r_gtx_blocks *b, int64_t *n_lines, int64_t *n_bytes)
{
    if (!c || !n_lines || !n_bytes) return fail(GTX_E_ARG, "[l2r_gtftext_blocks] null argument");
    GtxState &m = c->gtx;
    m.have_blocks = false; m.out.have = false; m.rl.active = false;
    for (int k = 0; k < GXS_N; ++k) if (k != GXS_ROUTE) m.stats[k] = 0;
    m.stats[GXS_GUARD] = 1;
    if (!m.have_rows) return fail(GTX_E_ARG, "[l2r_gtftext_blocks] no l2r_gtftext_rows in front");
    {   std::string msg;
        if (gtx_check_blocks(b, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    *n_lines = 0; *n_bytes = 0;
    const size_t M = (size_t)b->m;
    m.m = b->m; m.has_sel = M && b->sel; m.has_start = M && b->start; m.has_end = M && b->end; m.has_cov = M && b->cov;
    m.stats[GXS_BLOCKS] = (double)M;
    m.h_len.assign(M, 0u);
    if (M == 0) { m.have_blocks = true; return 0; }
    if (m.run_chains && c->n_reads != m.n) return fail(GTX_E_ARG, "[l2r_gtftext_blocks] the rows stand for a run of %lld reads, the context now holds %lld", (long long)m.n, (long long)c->n_reads);
    uint64_t lines = 0, bytes = 0;
    if (m.on_host) {
        GtxState::Host &h = m.h;
        if (m.has_sel) h.sel.assign(b->sel, b->sel + M); if (m.has_start) h.start.assign(b->start, b->start + M);
        if (m.has_end) h.end.assign(b->end, b->end + M); if (m.has_cov) h.cov.assign(b->cov, b->cov + M);
        l2r_gtx_rows hr; GtxChains cx; l2r_gtx_blocks hb;
        gtx_host_view(m, hr, cx, hb);
        for (size_t q = 0; q < M; ++q) {
            uint64_t by = 0, nl = 0;
            const int kind = gtx_block_bytes(&m.prm, &hr, cx, &hb, (int64_t)q, &by, &nl);
            if (kind) { std::string msg; gtx_block_fail(msg, (int64_t)q, kind); return fail(-1, "%s", msg.c_str()); }
            m.h_len[q] = (uint32_t)by; lines += nl; bytes += by;
        }
    } else {
        HIP_TRY(hipSetDevice(c->device));
        int rc;
        if ((rc = m.clk.begin(env_on("L2R_GTX_TIMING"), c->check_stages))) return rc;
        double per_block = m.exons_per_row;
        if (!m.run_chains) {
            uint64_t x = 0;
            for (size_t q = 0; q < M; ++q) { const int64_t t = b->sel ? (int64_t)b->sel[q] : (int64_t)q; if (t >= 0 && t < m.n) x += m.h_nex[(size_t)t]; }
            per_block = (double)x / (double)M;
        }
        const bool wave = wave_form(per_block, "L2R_GTX_WAVE");    // (exons per block of the selection)
        m.stats[GXS_WAVE] = wave ? 1 : 0;
        if ((m.has_sel && (rc = to_dev(c, m.sel, b->sel, M))) || (m.has_start && (rc = to_dev(c, m.start, b->start, M))) || (m.has_end && (rc = to_dev(c, m.end, b->end, M))) ||
            (m.has_cov && (rc = to_dev(c, m.cov, b->cov, M))) || m.len.ensure(M) || m.fix.ensure(M) || m.word64.ensure(2) || m.word.ensure(GTXC_TOTAL + 1)) rc = rc ? rc : -2;
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }  // (the columns are the caller's)
        const GtxIn in = gtx_in(c, m);
        const GtxMeasure meas{m.len.p, m.fix.p, m.word64.p, m.word64.p + 1};
        unsigned long long w[2] = {0, 0};
        if ((rc = measure_tail(c, m.clk, &m.stats[GXS_K_MEASURE], m.word64.p, w, 2, m.h_len, m.len.p, "l2r_gtftext_blocks", "block", GTX_E_N, gtx_block_fail, &bytes, [&] {
                const dim3 grid((unsigned)(((wave ? M * 64 : M) + 255) / 256));
                if (wave) hipLaunchKernelGGL(k_gtx_measure<true>, grid, dim3(256), 0, c->stream, in, meas);
                else hipLaunchKernelGGL(k_gtx_measure<false>, grid, dim3(256), 0, c->stream, in, meas);
            }))) return rc;
        lines = w[1];
    }
    m.have_blocks = true;
    *n_lines = (int64_t)lines; *n_bytes = (int64_t)bytes;
    return 0;
}

int l2r_gtftext_lines(l2r_ctx *c, int64_t first, int64_t max_blocks, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes)
{
    if (!c || !n_taken || !n_bytes) return fail(GTX_E_ARG, "[l2r_gtftext_lines] null argument");
    GtxState &m = c->gtx;
    m.out.reset();
    *n_taken = 0; *n_bytes = 0;
    if (!m.have_blocks) return fail(GTX_E_ARG, "[l2r_gtftext_lines] no l2r_gtftext_blocks or l2r_gtftext_list in front, or it failed");
    const bool list = m.rl.active;                      // the blocks of l2r_gtftext_list: the row source of l2r_readlist.hip.h
    int64_t take = 0, sum = 0;
    {   std::string msg;
        if (gtx_cut(m.h_len.data(), m.m, first, max_blocks, max_bytes, &take, &sum, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    const ReadRows &rr = m.rl.reads;
    if (!m.on_host && !list && m.run_chains && c->n_reads != m.n) return fail(GTX_E_ARG, "[l2r_gtftext_lines] the rows stand for a run of %lld reads, the context now holds %lld", (long long)m.n, (long long)c->n_reads);
    if (!m.on_host && list && rr.run_res && (c->n_reads != rr.n || !c->ran)) return fail(GTX_E_ARG, "[l2r_gtftext_lines] the reads stand for a run of %lld reads, the context now holds %lld", (long long)rr.n, (long long)c->n_reads);
    static const TextBatch batch{"l2r_gtftext_lines", "L2R_GTX_TIMING", "lines would have left their tile's span: k_gtx_measure and k_gtx_write disagree", GTX_TILE, GTXC_TOTAL, GTXC_OUTSIDE, GTXC_DIRECT};
    int64_t host_lines = 0;
    uint32_t w[GTXC_TOTAL + 1] = {0};
    const int rc = text_batch(c, batch, m.out, m.clk, m.len, m.off, m.word, m.stats, m.on_host, first, take, sum, w,
        [&](std::vector<uint8_t> &text, std::string &msg) {
            if (list) return rl_text_host(&m.prm, &m.rl.anno, rl_host_view(m), m.rl.h_sel, first, take, text, &host_lines, msg);
            l2r_gtx_rows hr; GtxChains cx; l2r_gtx_blocks hb;
            gtx_host_view(m, hr, cx, hb);
            return gtx_text_host(&m.prm, &hr, cx, &hb, first, take, text, &host_lines, msg);
        },
        [&](unsigned n_tiles, uint8_t *text) {
            if (list) hipLaunchKernelGGL(k_rl_write, dim3(n_tiles), dim3(GTX_THREADS), 0, c->stream, rl_in(c, m), first, take, (const uint32_t *)m.off.p, (const uint32_t *)m.fix.p, (const uint32_t *)m.rl.hfix.p, text, m.word.p);
            else hipLaunchKernelGGL(k_gtx_write, dim3(n_tiles), dim3(GTX_THREADS), 0, c->stream, gtx_in(c, m), first, take, (const uint32_t *)m.off.p, (const uint32_t *)m.fix.p, text, m.word.p);
        });
    if (rc) return rc;
    m.stats[GXS_LINES] = m.on_host ? (double)host_lines : (double)w[GTXC_LINES];
    *n_taken = take; *n_bytes = sum;
    return 0;
}

int l2r_gtftext_out(l2r_ctx *c, uint8_t *text, int64_t cap)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_out] null argument");
    return text_out(c, c->gtx.out, text, cap, "l2r_gtftext_out", "l2r_gtftext_lines", GTX_E_ARG);
}

int l2r_gtftext_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->gtx.stats : nullptr, GXS_N, out, n, "l2r_gtftext_stats"); }

// ---------------------------------------------------------------------------------------------- the read lists of update-gtf -a / -k / -v / -u
int l2r_gtftext_anno(l2r_ctx *c, const l2r_gtx_anno *a)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_anno] null argument");
    GtxState &m = c->gtx;
    GtxState::Lists &l = m.rl;
    l.have_anno = false; l.have_reads = false; l.active = false; m.have_blocks = false; m.out.have = false;
    if (!m.begun) return fail(GTX_E_ARG, "[l2r_gtftext_anno] no l2r_gtftext_begin in front");
    if (m.prm.form != L2R_GTX_READ) return fail(GTX_E_ARG, "[l2r_gtftext_anno] the read lists are blocks of form READ, l2r_gtftext_begin had form %d", m.prm.form);
    {   std::string msg;
        if (rl_check_anno(a, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    l.genes.set(a->n_tx, a->anno_names_len, a->anno_names, a->tx_gid, a->tx_gname);
    l.anno = l2r_gtx_anno{a->n_tx, a->anno_names_len, l.genes.h_names.data(), l.genes.h_gid.data(), l.genes.h_gname.data()};
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = l.genes.upload(c)) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    l.have_anno = true;
    return 0;
}

int l2r_gtftext_reads(l2r_ctx *c, const l2r_gtx_reads *r)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_reads] null argument");
    GtxState &m = c->gtx;
    GtxState::Lists &l = m.rl;
    l.have_reads = false; l.active = false; m.have_rows = false; m.have_blocks = false; m.out.have = false;
    if (!l.have_anno) return fail(GTX_E_ARG, "[l2r_gtftext_reads] no l2r_gtftext_anno in front");
    {   std::string msg;
        if (rl_check_reads(r, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    m.on_host = route_is_host("L2R_GTX_ROUTE");
    m.stats[GXS_ROUTE] = m.on_host ? 1 : 0;
    l.has_sj = r->has_sj != 0; l.split = r->split != 0;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = take_reads(c, l.reads, *r, m.on_host, "l2r_gtftext_reads", GTX_E_ARG, "reads")) return rc;
    if (!m.on_host) HIP_TRY(hipStreamSynchronize(c->stream));       // (the columns are the caller's)
    l.have_reads = true;
    return 0;
}

int l2r_gtftext_list(l2r_ctx *c, int list, int64_t *n_blocks, int64_t *n_lines, int64_t *n_bytes)
{
    if (!c || !n_blocks || !n_lines || !n_bytes) return fail(GTX_E_ARG, "[l2r_gtftext_list] null argument");
    GtxState &m = c->gtx;
    GtxState::Lists &l = m.rl;
    m.have_blocks = false; m.out.have = false; l.active = false;
    for (int k = 0; k < GXS_N; ++k) if (k != GXS_ROUTE) m.stats[k] = 0;
    m.stats[GXS_GUARD] = 1;
    *n_blocks = 0; *n_lines = 0; *n_bytes = 0;
    if (!l.have_reads) return fail(GTX_E_ARG, "[l2r_gtftext_list] no l2r_gtftext_reads in front");
    {   std::string msg;
        if (rl_check_list(list, msg)) return fail(GTX_E_ARG, "%s", msg.c_str()); }
    l.list = list; l.n_pieces = 0;
    m.m = 0; m.h_len.clear();
    const size_t N = (size_t)l.reads.n;
    uint64_t lines = 0, bytes = 0;
    if (m.on_host) {
        const RlReads hr = rl_host_view(m);
        rl_select(hr, list, l.h_sel);
        const size_t M = (size_t)l.h_sel.m();
        m.m = (int64_t)M; l.n_pieces = l.h_sel.n_pieces;
        m.h_len.assign(M, 0u);
        for (size_t q = 0; q < M; ++q) {
            uint64_t by = 0, nl = 0;
            const int kind = rl_block_bytes(&m.prm, &l.anno, hr, l.h_sel, (int64_t)q, &by, &nl);
            if (kind) { std::string msg; rl_block_fail(msg, (int64_t)q, kind); return fail(-1, "%s", msg.c_str()); }
            m.h_len[q] = (uint32_t)by; lines += nl; bytes += by;
        }
    } else if (N) {
        if (l.reads.run_res && (c->n_reads != l.reads.n || !c->ran)) return fail(GTX_E_ARG, "[l2r_gtftext_list] the reads stand for a run of %lld reads, the context now holds %lld", (long long)l.reads.n, (long long)c->n_reads);
        HIP_TRY(hipSetDevice(c->device));
        int rc;
        if ((rc = m.clk.begin(env_on("L2R_GTX_TIMING"), c->check_stages))) return rc;
        if (l.cnt.ensure(N + 1) || l.word.ensure(2) || m.word64.ensure(2) || m.word.ensure(GTXC_TOTAL + 1)) return -2;
        HIP_TRY(hipMemsetAsync(l.word.p, 0, 2 * sizeof(uint32_t), c->stream));
        RlIn in = rl_in(c, m);
        const dim3 per_read((unsigned)((N + 255) / 256));
        if ((rc = m.clk.launch(c, &m.stats[GXS_K_SELECT], [&] {
                hipLaunchKernelGGL(k_rl_count, per_read, dim3(256), 0, c->stream, in, l.cnt.p, l.word.p + 1);
                scan_u32(c, l.cnt.p, (int64_t)N, l.word.p);
            }))) { (void)hipStreamSynchronize(c->stream); return rc; }
        uint32_t w32[2] = {0, 0};
        if ((rc = download_all(c, 0, {{w32, l.word.p, sizeof w32}}, "l2r_gtftext_list"))) return rc;
        const size_t M = (size_t)w32[0];
        if ((uint64_t)w32[1] > (uint64_t)M) return fail(-5, "[l2r_gtftext_list] %u piece blocks of %zu blocks", w32[1], M);
        m.m = (int64_t)M; l.n_pieces = (int64_t)w32[1];
        m.h_len.assign(M, 0u);
        if (M) {
            if (l.b_read.ensure(M) || l.b_first.ensure(M) || l.b_count.ensure(M) || l.b_piece.ensure(M) || m.len.ensure(M) || m.fix.ensure(M) || l.hfix.ensure(M)) return -2;
            in = rl_in(c, m);
            if ((rc = m.clk.launch(c, &m.stats[GXS_K_SELECT], [&] {
                    hipLaunchKernelGGL(k_rl_take, per_read, dim3(256), 0, c->stream, in, (const uint32_t *)l.cnt.p, l.b_read.p, l.b_first.p, l.b_count.p, l.b_piece.p);
                }))) { (void)hipStreamSynchronize(c->stream); return rc; }
            const bool wave = wave_form(l.reads.exons_per_read, "L2R_GTX_WAVE");       // (exons per read: the lists are not looked at)
            m.stats[GXS_WAVE] = wave ? 1 : 0;
            const RlMeasure meas{m.len.p, m.fix.p, l.hfix.p, m.word64.p, m.word64.p + 1};
            unsigned long long w[2] = {0, 0};
            if ((rc = measure_tail(c, m.clk, &m.stats[GXS_K_MEASURE], m.word64.p, w, 2, m.h_len, m.len.p, "l2r_gtftext_list", "block", RL_E_N, rl_block_fail, &bytes, [&] {
                    const dim3 grid((unsigned)(((wave ? M * 64 : M) + 255) / 256));
                    if (wave) hipLaunchKernelGGL(k_rl_measure<true>, grid, dim3(256), 0, c->stream, in, meas);
                    else hipLaunchKernelGGL(k_rl_measure<false>, grid, dim3(256), 0, c->stream, in, meas);
                }))) return rc;
            lines = w[1];
        }
    }
    m.stats[GXS_BLOCKS] = (double)m.m; m.stats[GXS_PIECES] = (double)l.n_pieces;
    l.active = true; m.have_blocks = true;
    *n_blocks = m.m; *n_lines = (int64_t)lines; *n_bytes = (int64_t)bytes;
    return 0;
}

int l2r_gtftext_list_out(l2r_ctx *c, int32_t *read, int32_t *first, int32_t *count, int32_t *piece)
{
    if (!c) return fail(GTX_E_ARG, "[l2r_gtftext_list_out] null argument");
    GtxState &m = c->gtx;
    const GtxState::Lists &l = m.rl;
    if (!l.active || !m.have_blocks) return fail(GTX_E_ARG, "[l2r_gtftext_list_out] no selection: the last l2r_gtftext_list failed, or none was made");
    const size_t M = (size_t)m.m;
    if (!M) return 0;
    if (m.on_host) {
        const RlSel &s = l.h_sel;
        if (read) memcpy(read, s.read.data(), M * 4); if (first) memcpy(first, s.first.data(), M * 4);
        if (count) memcpy(count, s.count.data(), M * 4); if (piece) memcpy(piece, s.piece.data(), M * 4);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return download_all(c, 0, {{read, l.b_read.p, read ? M * 4 : 0}, {first, l.b_first.p, first ? M * 4 : 0}, {count, l.b_count.p, count ? M * 4 : 0},
                               {piece, l.b_piece.p, piece ? M * 4 : 0}}, "l2r_gtftext_list_out");
}

// ---------------------------------------------------------------------------------------------- the detail table of update-gtf -A
// slots of l2r_detail_stats
enum { DTS_ROWS = 0, DTS_LINES, DTS_BYTES, DTS_WAVE, DTS_TILES_LDS, DTS_TILES_DIRECT, DTS_ROUTE, DTS_GUARD, DTS_BATCHES, DTS_K_MEASURE, DTS_K_SCAN, DTS_K_WRITE, DTS_N };
static_assert(DTS_N == sizeof(DetailState::stats) / sizeof(double) && DTS_K_MEASURE == 9, "l2r_detail_stats: the words of include/lr2rmats_hip.h");
static_assert(DTS_LINES == TXS_LINES && DTS_K_WRITE == TXS_K_WRITE && GXS_LINES == TXS_LINES && GXS_K_WRITE == TXS_K_WRITE, "text_batch: the slots of a batch are the same words in both");
constexpr int DETC_TOTAL = DETC_N;                      // DetailState::word: k_detail_write's counters, then the scan's total
constexpr int DETAIL_E_ARG = -4;                        // arguments, order of calls: not -1, which is a domain error (the command falls back on it)

int l2r_detail_begin(l2r_ctx *c, const l2r_detail_params *p)
{
    if (!c) return fail(DETAIL_E_ARG, "[l2r_detail_begin] null argument");
    DetailState &m = c->detail;
    m.begun = false; m.have_rows = false; m.out.have = false;
    for (double &v : m.stats) v = 0;
    {   std::string msg;
        if (detail_check_params(p, msg)) return fail(DETAIL_E_ARG, "%s", msg.c_str()); }
    m.ref.set(p->n_ref, p->ref_off, p->ref_names);
    m.genes.set(p->n_tx, p->anno_names_len, p->anno_names, p->tx_gid, p->tx_gname);
    m.prm = *p;
    m.prm.ref_off = m.ref.h_off.data(); m.prm.ref_names = m.ref.h_names.data();
    m.prm.anno_names = m.genes.h_names.data(); m.prm.tx_gid = m.genes.h_gid.data(); m.prm.tx_gname = m.genes.h_gname.data();
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.ref.upload(c)) || (rc = m.genes.upload(c))) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.begun = true;
    return 0;
}

// the kernels' view of the rows
static DetailIn detail_in(const l2r_ctx *c, const DetailState &m)
{
    DetailIn in{};
    const ReadRows &r = m.rows;
    const ResultCols v = result_cols(c, r);
    in.n = r.n; in.tid = r.tid.p; in.names = r.names.p; in.names_len = r.names_len; in.qname = r.qname.p;
    in.ex_off = v.ex_off; in.info = v.info; in.xs = v.xs; in.xe = v.xe; in.ref_tx = v.ref_tx; in.f = v.f;
    in.n_ref = m.prm.n_ref; in.ref_off = m.ref.off.p; in.ref_names = m.ref.names.p;
    in.n_tx = m.prm.n_tx; in.anno_names_len = m.prm.anno_names_len; in.anno_names = m.genes.names.p; in.tx_gid = m.genes.gid.p; in.tx_gname = m.genes.gname.p;
    return in;
}
// ... and the host route's, over its copies
static l2r_detail_reads detail_host_view(const DetailState &m)
{
    const ReadRows::Host &h = m.rows.h;
    return l2r_detail_reads{m.rows.n, h.tid.data(), m.rows.names_len, h.names.data(), h.qname.data(), &h.res};
}

int l2r_detail_rows(l2r_ctx *c, const l2r_detail_reads *r, int64_t *n_bytes)
{
    if (!c || !n_bytes) return fail(DETAIL_E_ARG, "[l2r_detail_rows] null argument");
    DetailState &m = c->detail;
    m.have_rows = false; m.out.have = false;
    *n_bytes = 0;
    if (!m.begun) return fail(DETAIL_E_ARG, "[l2r_detail_rows] no l2r_detail_begin in front");
    {   std::string msg;
        if (detail_check_rows(r, msg)) return fail(DETAIL_E_ARG, "%s", msg.c_str()); }
    m.on_host = route_is_host("L2R_DETAIL_ROUTE");
    for (int k = 0; k < DTS_N; ++k) m.stats[k] = 0;
    m.stats[DTS_ROUTE] = m.on_host ? 1 : 0; m.stats[DTS_GUARD] = 1;
    const size_t N = (size_t)r->n;
    m.stats[DTS_ROWS] = (double)N;
    m.h_len.assign(N, 0u);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const l2r_gtx_reads reads{r->n, r->tid, r->names_len, r->names, r->qname, nullptr, r->res, 0, 0};
    if ((rc = take_reads(c, m.rows, reads, m.on_host, "l2r_detail_rows", DETAIL_E_ARG, "rows"))) return rc;
    if (N == 0 && !m.on_host) HIP_TRY(hipStreamSynchronize(c->stream));     // (no rows, but take_reads queues a names table where one came: the caller's)
    if (N == 0) { m.have_rows = true; return 0; }
    uint64_t bytes = 0;
    if (m.on_host) {
        const l2r_detail_reads hr = detail_host_view(m);
        for (size_t i = 0; i < N; ++i) {
            uint64_t by = 0; uint32_t split[DETAIL_SPLIT];
            const int kind = detail_line_bytes(&m.prm, &hr, (int64_t)i, &by, split);
            if (kind) { std::string msg; detail_row_fail(msg, (int64_t)i, kind); return fail(-1, "%s", msg.c_str()); }
            m.h_len[i] = (uint32_t)by; bytes += by;
        }
    } else {
        const bool wave = wave_form(m.rows.exons_per_read, "L2R_DETAIL_WAVE");
        m.stats[DTS_WAVE] = wave ? 1 : 0;
        if ((rc = m.clk.begin(env_on("L2R_DETAIL_TIMING"), c->check_stages)) || m.len.ensure(N) || m.split.ensure(N * DETAIL_SPLIT) || m.word64.ensure(1) || m.word.ensure(DETC_TOTAL + 1)) rc = rc ? rc : -2;
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }  // (the columns are the caller's)
        const DetailIn in = detail_in(c, m);
        const DetailMeasure meas{m.len.p, m.split.p, m.word64.p};
        unsigned long long w = 0;
        if ((rc = measure_tail(c, m.clk, &m.stats[DTS_K_MEASURE], m.word64.p, &w, 1, m.h_len, m.len.p, "l2r_detail_rows", "read", DET_E_N, detail_row_fail, &bytes, [&] {
                const dim3 grid((unsigned)(((wave ? N * 64 : N) + 255) / 256));
                if (wave) hipLaunchKernelGGL(k_detail_measure<true>, grid, dim3(256), 0, c->stream, in, meas);
                else hipLaunchKernelGGL(k_detail_measure<false>, grid, dim3(256), 0, c->stream, in, meas);
            }))) return rc;
    }
    m.have_rows = true;
    *n_bytes = (int64_t)bytes;
    return 0;
}

int l2r_detail_lines(l2r_ctx *c, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes)
{
    if (!c || !n_taken || !n_bytes) return fail(DETAIL_E_ARG, "[l2r_detail_lines] null argument");
    DetailState &m = c->detail;
    m.out.reset();
    *n_taken = 0; *n_bytes = 0;
    if (!m.have_rows) return fail(DETAIL_E_ARG, "[l2r_detail_lines] no l2r_detail_rows in front, or it failed");
    int64_t take = 0, sum = 0;
    {   std::string msg;
        if (detail_cut(m.h_len.data(), m.rows.n, first, max_rows, max_bytes, &take, &sum, msg)) return fail(DETAIL_E_ARG, "%s", msg.c_str()); }
    const ReadRows &rr = m.rows;
    if (!m.on_host && rr.run_res && (c->n_reads != rr.n || !c->ran)) return fail(DETAIL_E_ARG, "[l2r_detail_lines] the rows stand for a run of %lld reads, the context now holds %lld", (long long)rr.n, (long long)c->n_reads);
    static const TextBatch batch{"l2r_detail_lines", "L2R_DETAIL_TIMING", "bytes or segments would have left their place: k_detail_measure and k_detail_write disagree", DETAIL_TILE, DETC_TOTAL, DETC_OUTSIDE, DETC_DIRECT};
    uint32_t w[DETC_TOTAL + 1] = {0};
    const int rc = text_batch(c, batch, m.out, m.clk, m.len, m.off, m.word, m.stats, m.on_host, first, take, sum, w,
        [&](std::vector<uint8_t> &text, std::string &msg) { const l2r_detail_reads hr = detail_host_view(m); return detail_text_host(&m.prm, &hr, first, take, text, msg); },
        [&](unsigned n_tiles, uint8_t *text) {
            hipLaunchKernelGGL(k_detail_write, dim3(n_tiles), dim3(DETAIL_THREADS), 0, c->stream, detail_in(c, m), first, take, (const uint32_t *)m.off.p, (const uint32_t *)m.split.p, text, m.word.p);
        });
    if (rc) return rc;
    m.stats[DTS_LINES] = (double)take;
    *n_taken = take; *n_bytes = sum;
    return 0;
}

int l2r_detail_out(l2r_ctx *c, uint8_t *text, int64_t cap)
{
    if (!c) return fail(DETAIL_E_ARG, "[l2r_detail_out] null argument");
    return text_out(c, c->detail.out, text, cap, "l2r_detail_out", "l2r_detail_lines", DETAIL_E_ARG);
}

int l2r_detail_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->detail.stats : nullptr, DTS_N, out, n, "l2r_detail_stats"); }

// ---------------------------------------------------------------------------------------------- update-gtf: the novel list, its kept items, the BED text
constexpr int NOVC_TOTAL = NOVC_N;                      // NovelState::tword: k_nov_bed_write's counters, then the scan's total
constexpr int NOVEL_E_ARG = -4;                         // arguments and order of calls of the text entry points

int l2r_novel_begin(l2r_ctx *c, const l2r_params *prm, const l2r_novel_params *np)
{
    if (!c || !prm || !np) return fail(-1, "[l2r_novel_begin] null argument");
    NovelState &m = c->novel;
    m.begun = false; m.finished = false; m.text.reset();
    {   std::string msg;
        if (novel_check_begin(prm, np->n_ref, np->ref_off, np->ref_names, np->n_tx, np->tx_gene, msg)) return fail(-1, "%s", msg.c_str()); }
    m.p = uniq_prm(prm);
    m.np = NovelPrm{np->n_ref, np->n_tx, np->na_gene, np->has_sj != 0, prm->split_trans != 0};
    m.ref.set(np->n_ref, np->ref_off, np->ref_names);
    m.h_tx_gene.assign((size_t)np->n_tx + 1, 0u);
    if (np->n_tx) memcpy(m.h_tx_gene.data(), np->tx_gene, (size_t)np->n_tx * 4);
    m.has_gtf = false; m.gtf_ready = false; m.last_which = L2R_NOVEL_BED;
    if (np->src) {
        if (np->src_len < 0 || np->src_len > L2R_GTX_SRC_MAX) return fail(-1, "[l2r_novel_begin] a source string of %d bytes (at most %d)", np->src_len, L2R_GTX_SRC_MAX);
        {   std::string msg;
            if (text_check_genes(np->n_tx, np->anno_names_len, np->anno_names, np->tx_gid, np->tx_gname, msg, "l2r_novel_begin")) return fail(-1, "%s", msg.c_str()); }
        m.h_src.assign(np->src, np->src + np->src_len);
        m.genes.set(np->n_tx, np->anno_names_len, np->anno_names, np->tx_gid, np->tx_gname);
        m.anno_len = np->anno_names_len;
        m.has_gtf = true;
    }
    m.on_host = route_is_host("L2R_NOVEL_ROUTE");       // (tests, the comparator)
    m.n = 0; m.x = 0; m.adds = 0; m.split = 0; m.n_entries = 0;
    m.o_tid.clear(); m.o_ref.clear(); m.o_read.clear(); m.o_rev.clear(); m.o_nex.clear(); m.xs.clear(); m.xe.clear(); m.f.clear(); m.k_tid.clear(); m.k_gene.clear();
    m.h = NovelAcc(); m.out = NovelOut(); m.h_len.clear();
    for (double &v : m.stats) v = 0;
    m.stats[NVS_ROUTE] = m.on_host ? 1 : 0; m.stats[NVS_GUARD] = 1;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = m.ref.upload(c)) || (rc = put_dev(c, m.tx_gene, m.h_tx_gene)) || (m.has_gtf && (rc = m.genes.upload(c))) || m.bad.ensure(1) || m.aword.ensure(NOVW_N) || m.fword.ensure(NOVF_N)) { (void)hipStreamSynchronize(c->stream); return rc ? rc : -2; }
    HIP_TRY(hipMemsetAsync(m.bad.p, 0xff, sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    m.begun = true;
    return 0;
}

int l2r_novel_add(l2r_ctx *c, const l2r_summary_reads *r)
{
    if (!c || !r) return fail(-1, "[l2r_novel_add] null argument");
    NovelState &m = c->novel;
    if (!m.begun) return fail(-1, "[l2r_novel_add] no l2r_novel_begin in front");
    {   std::string msg;
        if (novel_check_result(r->n, r->tid, r->res, msg)) return fail(-1, "%s", msg.c_str()); }
    m.finished = false; m.gtf_ready = false; m.text.reset();
    const size_t N = (size_t)r->n;
    if (N == 0) { ++m.adds; m.stats[NVS_ADDS] = (double)m.adds; return 0; }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const bool run_res = !r->res;
    if (run_res) {
        if (!c->ran) return fail(-1, "[l2r_novel_add] no completed run on this context");
        if ((rc = fetch_totals(c))) return rc;
        if (!(c->want & L2R_WANT_RESULTS)) return fail(-1, "[l2r_novel_add] the last run kept no results (l2r_set_outputs without L2R_WANT_RESULTS)");
        if (r->n != c->n_reads) return fail(-1, "[l2r_novel_add] %lld reads, the last run had %lld", (long long)r->n, (long long)c->n_reads);
    }
    const size_t X = run_res ? (size_t)c->h_totals[0] : (size_t)r->res->n_exons;
    {   std::string msg;
        if (novel_check_totals(m.n, m.x, r->n, (int64_t)X, msg)) return fail(-1, "%s", msg.c_str()); }
    if (m.on_host) {
        NovelAcc &h = m.h;
        const size_t o0 = h.o_tid.size(), x0 = h.xs.size(), k0 = h.k_tid.size();
        const int64_t split0 = h.split, bad0 = h.bad; const int kind0 = h.bad_kind;
        try {
            if (run_res) {
                std::vector<int64_t> off(N + 1); std::vector<int32_t> xs(X ? X : 1), xe(X ? X : 1), ref(N); std::vector<uint8_t> f(X ? X : 1); std::vector<uint32_t> info(N);
                l2r_result res{(int64_t)N, (int64_t)X, 0, off.data(), xs.data(), xe.data(), f.data(), info.data(), ref.data()};
                if ((rc = l2r_download(c, &res))) return rc;
                novel_select(h, m.np, m.h_tx_gene.data(), (int64_t)N, r->tid, &res);
            } else novel_select(h, m.np, m.h_tx_gene.data(), (int64_t)N, r->tid, r->res);
        } catch (const std::bad_alloc &) {              // the accumulators as they were
            h.o_tid.resize(o0); h.o_ref.resize(o0); h.o_read.resize(o0); h.o_rev.resize(o0); h.o_nex.resize(o0); h.xs.resize(x0); h.xe.resize(x0); h.f.resize(x0); h.k_tid.resize(k0); h.k_gene.resize(k0);
            h.reads = m.n; h.split = split0; h.bad = bad0; h.bad_kind = kind0;
            return fail(-2, "[l2r_novel_add] no memory for the offers of %zu reads", N);
        }
        m.split = h.split;
        m.stats[NVS_OFFERS] = (double)h.o_tid.size(); m.stats[NVS_KNOWN] = (double)h.k_tid.size();
    } else {
        StageTimer &clk = m.u.clk;
        if ((rc = clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
        const size_t n_tiles = (N + NOV_TILE - 1) / NOV_TILE;
        if ((rc = to_dev(c, m.a_tid, r->tid, N))) {}
        else if (!run_res) {
            m.off32.resize(N + 1);
            for (size_t i = 0; i <= N; ++i) m.off32[i] = (uint32_t)r->res->ex_off[i];
            if ((rc = put_dev(c, m.a_off, m.off32)) || (rc = to_dev(c, m.a_info, (const uint32_t *)r->res->info, N)) || (rc = to_dev(c, m.a_ref, (const int32_t *)r->res->ref_tx, N)) ||
                (rc = to_dev(c, m.a_xs, (const int32_t *)r->res->ex_start, X)) || (rc = to_dev(c, m.a_xe, (const int32_t *)r->res->ex_end, X)) || (rc = to_dev(c, m.a_f, (const uint8_t *)r->res->ex_flag, X))) {}
        }
        if (!rc && (m.bits.ensure(N) || m.cnt_x.ensure(N + 1) || m.tile_cnt.ensure(2 * n_tiles + 1))) rc = -2;
        if (rc) return summary_no_room(c, "l2r_novel_add");
        HIP_TRY(hipMemsetAsync(m.aword.p, 0, NOVW_N * sizeof(uint32_t), c->stream));
        NovSel s{};
        s.n = (int64_t)N; s.read_base = m.n; s.tid = m.a_tid.p;
        if (run_res) { s.info = c->info.p; s.ex_off = c->ex_off.p; s.ref_tx = c->ref_tx.p; s.xs = c->ex_start.p; s.xe = c->ex_end.p; s.f = c->ex_flag.p; }
        else { s.info = m.a_info.p; s.ex_off = m.a_off.p; s.ref_tx = m.a_ref.p; s.xs = m.a_xs.p; s.xe = m.a_xe.p; s.f = m.a_f.p; }
        s.src_exons = (uint32_t)X;
        s.n_ref = m.np.n_ref; s.n_tx = m.np.n_tx; s.tx_gene = m.tx_gene.p; s.na_gene = m.np.na_gene; s.has_sj = m.np.has_sj; s.split = m.np.split;
        s.bits = m.bits.p; s.cnt_x = m.cnt_x.p; s.tile_cnt = m.tile_cnt.p; s.n_tiles = (int64_t)n_tiles; s.word = m.aword.p; s.bad = m.bad.p;
        rc = clk.launch(c, &m.stats[NVS_K_SELECT], [&] {
            hipLaunchKernelGGL(k_nov_flag, dim3((unsigned)n_tiles), dim3(NOV_TILE), 0, c->stream, s);
            scan_u32(c, m.cnt_x.p, (int64_t)N, m.aword.p + NOVW_EXONS);
            scan_u32(c, m.tile_cnt.p, (int64_t)(2 * n_tiles), m.aword.p + NOVW_TILES);
        });
        uint32_t w[NOVW_N] = {0}, n_off = 0;
        if ((rc = download_all(c, rc, {{w, m.aword.p, sizeof w}, {&n_off, m.tile_cnt.p + n_tiles, sizeof n_off}}, "l2r_novel_add"))) return rc;
        if (n_off > w[NOVW_TILES] || (size_t)w[NOVW_TILES] > 2 * N || (size_t)w[NOVW_EXONS] > X)
            return fail(-2, "[l2r_novel_add] %u offers and %u known reads of %zu reads, %u exons of %zu", n_off, w[NOVW_TILES] - n_off, N, w[NOVW_EXONS], X);
        const size_t O = n_off, K = w[NOVW_TILES] - n_off, XO = w[NOVW_EXONS];
        const size_t o0 = m.o_tid.n, k0 = m.k_tid.n, x0 = m.xs.n;
        // room first: a failed allocation leaves the accumulators as they were
        if (m.o_tid.reserve(c->stream, o0 + O) || m.o_ref.reserve(c->stream, o0 + O) || m.o_read.reserve(c->stream, o0 + O) || m.o_rev.reserve(c->stream, o0 + O) || m.o_nex.reserve(c->stream, o0 + O) ||
            m.xs.reserve(c->stream, x0 + XO) || m.xe.reserve(c->stream, x0 + XO) || m.f.reserve(c->stream, x0 + XO) || m.k_tid.reserve(c->stream, k0 + K) || m.k_gene.reserve(c->stream, k0 + K))
            return summary_no_room(c, "l2r_novel_add");
        s.n_off = (uint32_t)O; s.n_known = (uint32_t)K; s.o0 = o0; s.k0 = k0; s.x0 = x0; s.o_room = o0 + O; s.k_room = k0 + K; s.x_room = x0 + XO;
        s.o_tid = m.o_tid.p; s.o_ref = m.o_ref.p; s.o_read = m.o_read.p; s.o_rev = m.o_rev.p; s.o_nex = m.o_nex.p; s.a_xs = m.xs.p; s.a_xe = m.xe.p; s.a_f = m.f.p; s.k_tid = m.k_tid.p; s.k_gene = m.k_gene.p;
        const bool wave = wave_form(O ? (double)XO / (double)O : 0.0, "L2R_NOVEL_WAVE");       // (exons per offer)
        m.stats[NVS_WAVE] = wave ? 1 : 0;
        rc = clk.launch(c, &m.stats[NVS_K_SELECT], [&] {
            if (O + K) hipLaunchKernelGGL(k_nov_place, dim3((unsigned)n_tiles), dim3(NOV_TILE), 0, c->stream, s);
            const dim3 grid((unsigned)(((wave ? N * 64 : N) + 255) / 256));
            if (O && wave) hipLaunchKernelGGL(k_nov_chain<true>, grid, dim3(256), 0, c->stream, s);
            else if (O) hipLaunchKernelGGL(k_nov_chain<false>, grid, dim3(256), 0, c->stream, s);
        });
        if ((rc = download_all(c, rc, {}, "l2r_novel_add"))) return rc;      // (the columns are the caller's)
        m.o_tid.n = m.o_ref.n = m.o_read.n = m.o_rev.n = m.o_nex.n = o0 + O; m.xs.n = m.xe.n = m.f.n = x0 + XO; m.k_tid.n = m.k_gene.n = k0 + K;
        m.split += (int64_t)w[NOVW_SPLIT];
        m.stats[NVS_OFFERS] = (double)(o0 + O); m.stats[NVS_KNOWN] = (double)(k0 + K);
    }
    m.n += (int64_t)N; m.x += (int64_t)X; ++m.adds;
    m.stats[NVS_READS] = (double)m.n; m.stats[NVS_SPLIT] = (double)m.split; m.stats[NVS_ADDS] = (double)m.adds;
    return 0;
}

extern "C++" {
// the lengths of the BED lines, the counts and the stats that both routes leave alike, from m.kept and m.out / the device's rows
static void novel_done(NovelState &m, int64_t *counts)
{
    novel_counts(m.kept, m.n_entries, counts);
    m.stats[NVS_ENTRIES] = (double)m.n_entries;
    for (int l = 0; l < NOV_LISTS; ++l) m.stats[NVS_KEPT + l] = (double)m.kept[l];
    m.finished = true;
}

// novel_host over the host's copy of the accumulators (the refusals first: -1 names the read, -3 counts the split-route reads)
static int novel_on_host(NovelState &m, const NovelAcc &a, int64_t *counts)
{
    if (a.bad >= 0) { std::string msg; novel_read_fail(msg, a.bad, a.bad_kind); return fail(-1, "%s", msg.c_str()); }
    if (a.split) return fail(-3, "[l2r_novel_finish] %lld split-route reads: their pieces enter the list without a place, the host tail merges it", (long long)a.split);
    novel_host(a, m.p, m.h_tx_gene.data(), m.np.na_gene, m.out);
    const NovelOut &o = m.out;
    m.n_entries = (int64_t)o.e_src.size();
    m.row0[0] = 0;
    for (int l = 0; l < NOV_LISTS; ++l) { m.kept[l] = (int64_t)o.rows[l].tid.size(); m.row0[l + 1] = m.row0[l] + m.kept[l]; m.stats[NVS_ITEMS + l] = (double)o.items[l]; }
    const NovelRows &E = o.rows[NOV_EXON];
    m.h_len.resize(E.tid.size());
    for (size_t q = 0; q < E.tid.size(); ++q) m.h_len[q] = novel_bed_bytes(m.ref.h_off.data(), E.tid[q], E.a[q], E.b[q], E.score[q]);
    m.rows_on_host = true;
    m.stats[NVS_ROUTE] = 1; m.stats[NVS_CLUSTERS] = (double)o.clusters; m.stats[NVS_LARGEST] = (double)o.largest;
    m.stats[NVS_HITS] = (double)(o.u.hits[0] + o.u.hits[1] + o.u.hits[2]); m.stats[NVS_WIDENED] = (double)o.widened;
    novel_done(m, counts);
    return 0;
}

// the device's accumulators fetched, then novel_host (input that is not in order)
static int novel_fetch_host(l2r_ctx *c, NovelState &m, int64_t *counts)
{
    for (int k = NVS_K_MERGE; k <= NVS_K_KEEP; ++k) m.stats[k] = 0;
    m.h = NovelAcc();                                   // (kept: the updated GTF reads the chains from it)
    NovelAcc &a = m.h;
    const size_t O = m.o_tid.n, K = m.k_tid.n, X = m.xs.n;
    try {
        a.o_tid.resize(O); a.o_ref.resize(O); a.o_read.resize(O); a.o_rev.resize(O); a.o_nex.resize(O); a.xs.resize(X); a.xe.resize(X); a.f.resize(X); a.k_tid.resize(K); a.k_gene.resize(K);
    } catch (const std::bad_alloc &) { return fail(-2, "[l2r_novel_finish] no memory for %zu offers", O); }
    a.reads = m.n;
    if (int rc = download_all(c, 0, {{a.o_tid.data(), m.o_tid.p, O * 4}, {a.o_ref.data(), m.o_ref.p, O * 4}, {a.o_read.data(), m.o_read.p, O * 4}, {a.o_rev.data(), m.o_rev.p, O}, {a.o_nex.data(), m.o_nex.p, O * 4},
                                     {a.xs.data(), m.xs.p, X * 4}, {a.xe.data(), m.xe.p, X * 4}, {a.f.data(), m.f.p, X}, {a.k_tid.data(), m.k_tid.p, K * 4}, {a.k_gene.data(), m.k_gene.p, K * 4}}, "l2r_novel_finish")) return rc;
    return novel_on_host(m, a, counts);
}
}

int l2r_novel_finish(l2r_ctx *c, int64_t *counts)
{
    if (!c || !counts) return fail(-1, "[l2r_novel_finish] null argument");
    NovelState &m = c->novel;
    if (!m.begun) return fail(-1, "[l2r_novel_finish] no l2r_novel_begin in front");
    for (int k = 0; k < 8; ++k) counts[k] = 0;
    for (int k = NVS_CLUSTERS; k < NVS_WAVE; ++k) m.stats[k] = 0;
    for (int k = NVS_K_MERGE; k < NVS_N; ++k) m.stats[k] = 0;
    m.finished = false; m.gtf_ready = false; m.rows_on_host = false; m.text.reset(); m.out = NovelOut(); m.h_len.clear(); m.n_entries = 0;
    for (int l = 0; l < NOV_LISTS; ++l) { m.kept[l] = 0; m.row0[l] = 0; }
    m.row0[NOV_LISTS] = 0;
    if (m.on_host) return novel_on_host(m, m.h, counts);
    HIP_TRY(hipSetDevice(c->device));
    int rc = 0;
    StageTimer &clk = m.u.clk;
    if ((rc = clk.begin(env_on("L2R_SORT_TIMING"), c->check_stages))) return rc;
    {   unsigned long long bad = ~0ull;
        if ((rc = download_all(c, 0, {{&bad, m.bad.p, sizeof bad}}, "l2r_novel_finish"))) return rc;
        if (bad != ~0ull) {
            const unsigned long long q = bad >> 4; const int kind = (int)(bad & 15ull);
            if (q >= (unsigned long long)m.n || kind <= 0 || kind >= NOV_E_N) return fail(-2, "[l2r_novel_finish] the device names read %llu of %lld, kind %d", q, (long long)m.n, kind);
            std::string msg; novel_read_fail(msg, (int64_t)q, kind);
            return fail(-1, "%s", msg.c_str());
        } }
    if (m.split) return fail(-3, "[l2r_novel_finish] %lld split-route reads: their pieces enter the list without a place, the host tail merges it", (long long)m.split);
    const size_t O = m.o_tid.n, K = m.k_tid.n, XO = m.xs.n;
    UniqState &u = m.u;
    uint32_t w[NOVF_N] = {0};
    HIP_TRY(hipMemsetAsync(m.fword.p, 0, NOVF_N * sizeof(uint32_t), c->stream));
    // ---- the merge
    if (O) {
        if (m.o_off.ensure(O + 1) || u.tid.ensure(O) || u.rev.ensure(O) || u.ex_off.ensure(O + 1) || u.xs.ensure(XO ? XO : 1) || u.xe.ensure(XO ? XO : 1)) return summary_no_room(c, "l2r_novel_finish");
        HIP_TRY(hipMemcpyAsync(m.o_off.p, m.o_nex.p, O * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(u.tid.p, m.o_tid.p, O * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(u.rev.p, m.o_rev.p, O, hipMemcpyDeviceToDevice, c->stream));
        if (XO) { HIP_TRY(hipMemcpyAsync(u.xs.p, m.xs.p, XO * 4, hipMemcpyDeviceToDevice, c->stream)); HIP_TRY(hipMemcpyAsync(u.xe.p, m.xe.p, XO * 4, hipMemcpyDeviceToDevice, c->stream)); }
    }
    rc = clk.launch(c, &m.stats[NVS_K_MERGE], [&] {
        if (O) {
            scan_u32(c, m.o_off.p, (int64_t)O, m.fword.p + NOVF_EXONS);
            hipLaunchKernelGGL(k_nov_widen, dim3((unsigned)((O + 1 + 255) / 256)), dim3(256), 0, c->stream, (int64_t)O, (const uint32_t *)m.o_off.p, u.ex_off.p);
        }
        if (K > 1) hipLaunchKernelGGL(k_nov_descends, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, (int64_t)K, (const int32_t *)m.k_tid.p, m.fword.p);
    });
    if ((rc = download_all(c, rc, {{w, m.fword.p, sizeof w}}, "l2r_novel_finish"))) return rc;
    if (O && (size_t)w[NOVF_EXONS] != XO) return fail(-2, "[l2r_novel_finish] the exon counts of the offers add up to %u, %zu exons were appended", w[NOVF_EXONS], XO);
    if (w[NOVF_DESCENDS]) return novel_fetch_host(c, m, counts);
    uint32_t uw[UQW_N] = {0};
    if (O) {
        if ((rc = uniq_device(c, u, O, m.p, "l2r_novel_finish", &m.stats[NVS_K_MERGE], &m.stats[NVS_K_MERGE], &m.stats[NVS_K_MERGE], uw))) return rc;
        if (uw[UQW_UNSORTED]) return novel_fetch_host(c, m, counts);
    }
    const size_t U = uw[UQW_UNIQUE];
    m.n_entries = (int64_t)U;
    m.stats[NVS_ROUTE] = 0; m.stats[NVS_CLUSTERS] = (double)uw[UQW_CLUSTERS]; m.stats[NVS_LARGEST] = (double)uw[UQW_LARGEST];
    m.stats[NVS_HITS] = (double)((uint64_t)uw[UQW_IDENT] + uw[UQW_CONTAINED] + uw[UQW_SINGLE]);
    // ---- the items
    NovItems t{};
    t.n_entries = (uint32_t)U; t.n_offers = (uint32_t)O; t.n_exons = (uint32_t)XO; t.n_known = (uint32_t)K;
    t.u_src = u.u_src.p; t.u_start = u.u_start.p; t.u_end = u.u_end.p; t.u_cov = u.u_cov.p;
    t.o_tid = m.o_tid.p; t.o_ref = m.o_ref.p; t.o_read = m.o_read.p; t.o_rev = m.o_rev.p; t.o_nex = m.o_nex.p; t.o_off = m.o_off.p;
    t.xs = m.xs.p; t.xe = m.xe.p; t.f = m.f.p; t.k_tid = m.k_tid.p; t.k_gene = m.k_gene.p; t.tx_gene = m.tx_gene.p; t.na_gene = m.np.na_gene; t.word = m.fword.p;
    uint32_t start[NOV_LISTS + 1] = {0};                // where every list's items begin
    if (U) {
        const size_t n_cnt = (size_t)(NOV_GENE + 1) * U;
        if (m.cnt.ensure(n_cnt + 1) || m.e_src.ensure(U)) return summary_no_room(c, "l2r_novel_finish");
        t.cnt = m.cnt.p; t.e_src = m.e_src.p;
        rc = clk.launch(c, &m.stats[NVS_K_ITEMS], [&] {
            hipLaunchKernelGGL(k_nov_count, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, c->stream, t);
            scan_u32(c, m.cnt.p, (int64_t)n_cnt, m.fword.p + NOVF_ITEMS);
        });
        hipError_t e = hipSuccess;
        for (int l = 1; l <= NOV_GENE && !rc && e == hipSuccess; ++l) e = hipMemcpyAsync(&start[l], m.cnt.p + (size_t)l * U, 4, hipMemcpyDeviceToHost, c->stream);
        if (!rc && e != hipSuccess) rc = fail(-2, "[l2r_novel_finish] %s", hipGetErrorString(e));
        if ((rc = download_all(c, rc, {{w, m.fword.p, sizeof w}}, "l2r_novel_finish"))) return rc;
    }
    const uint64_t n_items64 = (uint64_t)w[NOVF_ITEMS] + K;
    if (n_items64 >= (uint64_t)NOV_MAX_ITEMS) return fail(-1, "[l2r_novel_finish] %llu items in the six lists (below 2^32 - 64)", (unsigned long long)n_items64);
    const uint32_t n_items = (uint32_t)n_items64;
    start[NOV_KNOWN_GENE] = w[NOVF_ITEMS]; start[NOV_LISTS] = n_items;
    for (int l = 0; l < NOV_LISTS; ++l) {
        if (start[l + 1] < start[l]) return fail(-2, "[l2r_novel_finish] the items of list %d begin at %u, those behind at %u", l, start[l], start[l + 1]);
        m.stats[NVS_ITEMS + l] = (double)(start[l + 1] - start[l]);
    }
    m.stats[NVS_WIDENED] = (double)w[NOVF_WIDENED];
    if (n_items == 0) { novel_done(m, counts); return 0; }
    const size_t NI = n_items;
    t.n_items = n_items; t.base_known = w[NOVF_ITEMS];
    if (m.hi.ensure(NI) || m.ia.ensure(NI) || m.ib.ensure(NI) || m.icov.ensure(NI) || m.imeta.ensure(NI) || m.order1.ensure(NI) || m.order.ensure(NI) || m.head.ensure(NI + 1) || m.first.ensure(NI + 1) ||
        m.grp.ensure(NI) || m.sum.ensure(NI)) return summary_no_room(c, "l2r_novel_finish");
    t.hi = m.hi.p; t.a = m.ia.p; t.b = m.ib.p; t.cov = m.icov.p; t.meta = m.imeta.p;
    HIP_TRY(hipMemsetAsync(m.hi.p, 0, NI * 4, c->stream)); HIP_TRY(hipMemsetAsync(m.ia.p, 0, NI * 4, c->stream)); HIP_TRY(hipMemsetAsync(m.ib.p, 0, NI * 4, c->stream));
    HIP_TRY(hipMemsetAsync(m.icov.p, 0, NI * 4, c->stream)); HIP_TRY(hipMemsetAsync(m.imeta.p, 0, NI, c->stream));
    HIP_TRY(hipMemsetAsync(m.first.p, 0, (NI + 1) * 4, c->stream)); HIP_TRY(hipMemsetAsync(m.sum.p, 0, NI * 4, c->stream));
    if ((rc = clk.launch(c, &m.stats[NVS_K_ITEMS], [&] {
            if (U) hipLaunchKernelGGL(k_nov_emit, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, c->stream, t);
            if (K) hipLaunchKernelGGL(k_nov_emit_known, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, t);
        }))) { (void)hipStreamSynchronize(c->stream); return rc; }
    // ---- the stable order by (list, tid, a, b): on b, then on the upper 64 bits read through the first order
    {   double *const ms[3] = {&m.stats[NVS_K_SORT], &m.stats[NVS_K_SORT], &m.stats[NVS_K_SORT]};
        const uint32_t *order1 = nullptr, *perm2 = nullptr;
        int n_pass = 0;
        if ((rc = order_by_keys(c, clk, NovLowKeyOf{m.ib.p}, n_items, ms[0], ms, &n_pass, nullptr, &order1))) { (void)hipStreamSynchronize(c->stream); return rc; }
        if (order1) {                                   // (stage 2 runs in the same index columns)
            HIP_TRY(hipMemcpyAsync(m.order1.p, order1, NI * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            order1 = m.order1.p;
        }
        if ((rc = order_by_keys(c, clk, NovHighKeyOf{m.hi.p, m.ia.p, order1, n_items}, n_items, ms[0], ms, &n_pass, nullptr, &perm2))) { (void)hipStreamSynchronize(c->stream); return rc; }
        if ((rc = clk.launch(c, &m.stats[NVS_K_SORT], [&] {
                hipLaunchKernelGGL(k_gtf_compose, dim3((unsigned)((NI + GTF_THREADS - 1) / GTF_THREADS)), dim3(GTF_THREADS), 0, c->stream, order1, perm2, n_items, m.order.p);
            }))) { (void)hipStreamSynchronize(c->stream); return rc; } }
    // ---- the first item of every key, in item order
    const NovKeys keys{n_items, m.order.p, m.hi.p, m.ia.p, m.ib.p};
    const unsigned grid_i = (unsigned)((NI + 255) / 256);
    rc = clk.launch(c, &m.stats[NVS_K_KEEP], [&] {
        hipLaunchKernelGGL(k_nov_heads, dim3(grid_i), dim3(256), 0, c->stream, keys, m.head.p);
        scan_u32(c, m.head.p, (int64_t)NI, m.fword.p + NOVF_GROUPS);
        hipLaunchKernelGGL(k_nov_groups, dim3(grid_i), dim3(256), 0, c->stream, keys, (const uint32_t *)m.head.p, (const uint32_t *)m.icov.p, m.first.p, m.grp.p, m.sum.p);
        scan_u32(c, m.first.p, (int64_t)NI, m.fword.p + NOVF_ROWS);
    });
    uint32_t row0[NOV_LISTS + 1] = {0};
    {   hipError_t e = hipSuccess;
        for (int l = 1; l < NOV_LISTS && !rc && e == hipSuccess; ++l) e = hipMemcpyAsync(&row0[l], m.first.p + start[l], 4, hipMemcpyDeviceToHost, c->stream);
        if (!rc && e != hipSuccess) rc = fail(-2, "[l2r_novel_finish] %s", hipGetErrorString(e)); }
    if ((rc = download_all(c, rc, {{w, m.fword.p, sizeof w}}, "l2r_novel_finish"))) return rc;
    const size_t R = w[NOVF_ROWS];
    row0[NOV_LISTS] = (uint32_t)R;
    if (R == 0 || R > NI || w[NOVF_GROUPS] != R) return fail(-2, "[l2r_novel_finish] %u keys and %zu first items of %zu items", w[NOVF_GROUPS], R, NI);
    for (int l = 0; l < NOV_LISTS; ++l) if (row0[l + 1] < row0[l]) return fail(-2, "[l2r_novel_finish] the rows of list %d begin at %u, those behind at %u", l, row0[l], row0[l + 1]);
    if (m.r_tid.ensure(R) || m.r_a.ensure(R) || m.r_b.ensure(R) || m.r_score.ensure(R) || m.r_meta.ensure(R)) return summary_no_room(c, "l2r_novel_finish");
    const size_t E = row0[NOV_EXON + 1] - row0[NOV_EXON], G0 = row0[NOV_GENE], NG = R - G0;
    if (m.len.ensure(E ? E : 1)) return summary_no_room(c, "l2r_novel_finish");
    const NovBed bed{(uint32_t)E, m.r_tid.p, m.r_a.p, m.r_b.p, m.r_score.p, m.r_meta.p, m.np.n_ref, m.ref.off.p, m.ref.names.p};
    rc = clk.launch(c, &m.stats[NVS_K_KEEP], [&] {
        hipLaunchKernelGGL(k_nov_keep, dim3(grid_i), dim3(256), 0, c->stream, keys, (const uint32_t *)m.first.p, (const uint32_t *)m.grp.p, (const uint32_t *)m.sum.p, (const uint8_t *)m.imeta.p, (uint32_t)R,
                           NovRows{m.r_tid.p, m.r_a.p, m.r_b.p, m.r_score.p, m.r_meta.p});
    });
    if (!rc && E) rc = clk.launch(c, &m.stats[NVS_K_MEASURE], [&] { hipLaunchKernelGGL(k_nov_bed_measure, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, c->stream, bed, m.len.p); });
    // the gene rows come to the host, where add_gene's last test is made (novel_gene_rows); the lines' lengths for the cut
    std::vector<int32_t> g_tid(NG ? NG : 1), g_a(NG ? NG : 1);
    m.h_len.assign(E, 0u);
    if ((rc = download_all(c, rc, {{g_tid.data(), m.r_tid.p + G0, NG * 4}, {g_a.data(), m.r_a.p + G0, NG * 4}, {m.h_len.data(), m.len.p, E * 4}}, "l2r_novel_finish"))) return rc;
    for (int l = NOV_GENE; l < NOV_LISTS; ++l) {
        NovelRows &g = m.out.rows[l];
        const size_t lo = row0[l] - G0, hi = row0[l + 1] - G0;
        g.tid.assign(g_tid.begin() + lo, g_tid.begin() + hi); g.a.assign(g_a.begin() + lo, g_a.begin() + hi);
        g.b.assign(hi - lo, 0); g.score.assign(hi - lo, 0); g.meta.assign(hi - lo, 0);
        novel_gene_rows(g);
    }
    for (int l = 0; l <= NOV_LISTS; ++l) m.row0[l] = (int64_t)row0[l];
    for (int l = 0; l < NOV_GENE; ++l) m.kept[l] = (int64_t)(row0[l + 1] - row0[l]);
    for (int l = NOV_GENE; l < NOV_LISTS; ++l) m.kept[l] = (int64_t)m.out.rows[l].tid.size();
    novel_done(m, counts);
    return 0;
}

int l2r_novel_entries_out(l2r_ctx *c, int32_t *src, int32_t *start, int32_t *end, int32_t *cov)
{
    if (!c) return fail(-1, "[l2r_novel_entries_out] null argument");
    const NovelState &m = c->novel;
    if (!m.finished) return fail(-1, "[l2r_novel_entries_out] no results: the last l2r_novel_finish failed, or none was made");
    const size_t U = (size_t)m.n_entries;
    if (U == 0) return 0;
    if (m.rows_on_host) {
        const NovelOut &o = m.out;
        if (src) memcpy(src, o.e_src.data(), U * 4);
        if (start) memcpy(start, o.e_start.data(), U * 4);
        if (end) memcpy(end, o.e_end.data(), U * 4);
        if (cov) memcpy(cov, o.e_cov.data(), U * 4);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return download_all(c, 0, {{src, m.e_src.p, src ? U * 4 : 0}, {start, m.u.u_start.p, start ? U * 4 : 0}, {end, m.u.u_end.p, end ? U * 4 : 0}, {cov, m.u.u_cov.p, cov ? U * 4 : 0}}, "l2r_novel_entries_out");
}

int l2r_novel_rows_out(l2r_ctx *c, int list, int32_t *tid, int32_t *a, int32_t *b, int32_t *score, uint8_t *meta)
{
    if (!c) return fail(-1, "[l2r_novel_rows_out] null argument");
    const NovelState &m = c->novel;
    if (!m.finished) return fail(-1, "[l2r_novel_rows_out] no results: the last l2r_novel_finish failed, or none was made");
    if (list < 0 || list >= NOV_LISTS) return fail(-1, "[l2r_novel_rows_out] list %d (0 .. %d)", list, NOV_LISTS - 1);
    const size_t R = (size_t)m.kept[list];
    if (R == 0) return 0;
    if (m.rows_on_host || list >= NOV_GENE) {
        const NovelRows &r = m.out.rows[list];
        if (tid) memcpy(tid, r.tid.data(), R * 4);
        if (a) memcpy(a, r.a.data(), R * 4);
        if (b) memcpy(b, r.b.data(), R * 4);
        if (score) memcpy(score, r.score.data(), R * 4);
        if (meta) memcpy(meta, r.meta.data(), R);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t r0 = (size_t)m.row0[list];
    return download_all(c, 0, {{tid, m.r_tid.p + r0, tid ? R * 4 : 0}, {a, m.r_a.p + r0, a ? R * 4 : 0}, {b, m.r_b.p + r0, b ? R * 4 : 0}, {score, m.r_score.p + r0, score ? R * 4 : 0},
                               {meta, m.r_meta.p + r0, meta ? R : 0}}, "l2r_novel_rows_out");
}

int l2r_novel_lines(l2r_ctx *c, int which, int64_t first, int64_t max_rows, int64_t max_bytes, int64_t *n_taken, int64_t *n_bytes)
{
    if (!c || !n_taken || !n_bytes) return fail(NOVEL_E_ARG, "[l2r_novel_lines] null argument");
    NovelState &m = c->novel;
    m.text.reset();
    *n_taken = 0; *n_bytes = 0;
    if (!m.finished) return fail(NOVEL_E_ARG, "[l2r_novel_lines] no l2r_novel_finish in front, or it failed");
    if (which == L2R_NOVEL_GTF) {
        if (!m.gtf_ready) return fail(NOVEL_E_ARG, "[l2r_novel_lines] no l2r_novel_names in front, or it failed");
        m.last_which = L2R_NOVEL_GTF;
        return l2r_gtftext_lines(c, first, max_rows, max_bytes, n_taken, n_bytes);
    }
    m.last_which = L2R_NOVEL_BED;
    if (which != L2R_NOVEL_BED) return fail(NOVEL_E_ARG, "[l2r_novel_lines] which = %d", which);
    int64_t take = 0, sum = 0;
    {   std::string msg;
        if (novel_cut(m.h_len.data(), m.kept[NOV_EXON], first, max_rows, max_bytes, &take, &sum, msg)) return fail(NOVEL_E_ARG, "%s", msg.c_str()); }
    static const TextBatch batch{"l2r_novel_lines", "L2R_SORT_TIMING", "lines would have left their place: k_nov_bed_measure and k_nov_bed_write disagree", NOV_BED_TILE, NOVC_TOTAL, NOVC_OUTSIDE, NOVC_DIRECT};
    uint32_t w[NOVC_TOTAL + 1] = {0};
    m.tstats[TXS_GUARD] = 1; m.tstats[TXS_K_SCAN] = 0; m.tstats[TXS_K_WRITE] = 0;
    const NovBed bed{(uint32_t)m.kept[NOV_EXON], m.r_tid.p, m.r_a.p, m.r_b.p, m.r_score.p, m.r_meta.p, m.np.n_ref, m.ref.off.p, m.ref.names.p};
    const int rc = text_batch(c, batch, m.text, m.u.clk, m.len, m.off, m.tword, m.tstats, m.rows_on_host, first, take, sum, w,
        [&](std::vector<uint8_t> &text, std::string &) { novel_bed_host(m.out.rows[NOV_EXON], m.ref.h_off.data(), m.ref.h_names.data(), first, take, text); return 0; },
        [&](unsigned n_tiles, uint8_t *text) {
            hipLaunchKernelGGL(k_nov_bed_write, dim3(n_tiles), dim3(NOV_BED_TILE), 0, c->stream, bed, first, take, (const uint32_t *)m.off.p, text, m.tword.p);
        });
    m.stats[NVS_K_SCAN] += m.tstats[TXS_K_SCAN]; m.stats[NVS_K_WRITE] += m.tstats[TXS_K_WRITE];
    if (m.tstats[TXS_GUARD] == 0) m.stats[NVS_GUARD] = 0;
    if (rc) return rc;
    *n_taken = take; *n_bytes = sum;
    return 0;
}

// The updated GTF of the entries through the GTF-text unit (l2r_gtftext_*): the rows are the OFFERS -- the accumulators' columns and chains,
// copied inside HBM -- the blocks the entries (sel = the entry's offer, with k_uniq_take's start, end and cov), and the names one table:
// the annotation's, `NA`, the caller's.  g / G of an offer are those of its ref, t / T the entry's tid_name / qname.
int l2r_novel_names(l2r_ctx *c, const l2r_novel_name_table *t, int64_t *n_lines, int64_t *n_bytes)
{
    if (!c || !t || !n_lines || !n_bytes) return fail(NOVEL_E_ARG, "[l2r_novel_names] null argument");
    NovelState &m = c->novel;
    m.gtf_ready = false;
    *n_lines = 0; *n_bytes = 0;
    if (!m.finished) return fail(NOVEL_E_ARG, "[l2r_novel_names] no l2r_novel_finish in front, or it failed");
    if (!m.has_gtf) return fail(NOVEL_E_ARG, "[l2r_novel_names] l2r_novel_begin came without a source string and gene tables");
    const size_t U = (size_t)m.n_entries, A = (size_t)m.anno_len, NL = (size_t)(t->names_len > 0 ? t->names_len : 0);
    if (t->names_len < 0 || (uint64_t)A + 3 + NL > 0xffffffffull) return fail(NOVEL_E_ARG, "[l2r_novel_names] a names table of %lld bytes", (long long)t->names_len);
    if (U && (!t->qname || (NL && !t->names))) return fail(NOVEL_E_ARG, "[l2r_novel_names] null column");
    const uint32_t na = (uint32_t)A, base = (uint32_t)A + 3u;
    const uint32_t *tid_name = t->tid_name ? t->tid_name : t->qname;
    for (size_t e = 0; e < U; ++e)                      // (added to base below: an offset beyond the table would name another string, or wrap)
        if ((size_t)t->qname[e] >= NL || (size_t)tid_name[e] >= NL) return fail(NOVEL_E_ARG, "[l2r_novel_names] entry %zu: a name id at or beyond names_len", e);
    const l2r_gtx_params gp{m.np.n_ref, m.ref.h_off.data(), m.ref.h_names.data(), L2R_GTX_READ, (int32_t)m.h_src.size(), m.h_src.data()};
    int rc;
    if ((rc = l2r_gtftext_begin(c, &gp))) return rc;
    std::vector<uint8_t> names(A + 3 + NL);
    if (A) memcpy(names.data(), m.genes.h_names.data(), A);
    names[A] = 'N'; names[A + 1] = 'A'; names[A + 2] = 0;
    if (NL) memcpy(names.data() + base, t->names, NL);
    std::vector<int32_t> sel(U ? U : 1), start(U ? U : 1), end(U ? U : 1), cov(U ? U : 1);
    GtxState &g = c->gtx;
    if (m.rows_on_host) {
        const NovelAcc &a = m.h;
        const size_t O = a.o_tid.size();
        std::vector<int64_t> off;
        (void)novel_trans(a, off);
        std::vector<uint32_t> id[4];
        for (auto &v : id) v.assign(O ? O : 1, na);
        for (size_t e = 0; e < U; ++e) {
            const size_t o = (size_t)m.out.u.u_src[e];
            const int32_t ref = a.o_ref[o];
            if (ref >= 0) { id[0][o] = m.genes.h_gid[(size_t)ref]; id[2][o] = m.genes.h_gname[(size_t)ref]; }
            id[1][o] = base + tid_name[e]; id[3][o] = base + t->qname[e];
            sel[e] = (int32_t)o; start[e] = m.out.e_start[e]; end[e] = m.out.e_end[e]; cov[e] = m.out.e_cov[e];
        }
        const l2r_gtx_rows rows{(int64_t)O, a.o_tid.data(), a.o_rev.data(), off.data(), a.xs.data(), a.xe.data(), (int64_t)names.size(), names.data(), id[0].data(), id[1].data(), id[2].data(), id[3].data()};
        if (O && (rc = l2r_gtftext_rows(c, &rows))) return rc;
        if (!O) { g.n = 0; g.names_len = 0; g.on_host = true; g.run_chains = false; g.have_rows = true; }
    } else {
        HIP_TRY(hipSetDevice(c->device));
        const size_t O = m.o_tid.n, X = m.xs.n;
        g.on_host = false; g.stats[GXS_ROUTE] = 0; g.run_chains = false;
        g.n = (int64_t)O; g.names_len = (int64_t)names.size();
        g.h_nex.assign(O, 0u);
        if (g.tid.ensure(O ? O : 1) || g.rev.ensure(O ? O : 1) || g.ex_off.ensure(O + 1) || g.xs.ensure(X ? X : 1) || g.xe.ensure(X ? X : 1) || g.id[0].ensure(O ? O : 1) || g.id[1].ensure(O ? O : 1) ||
            g.id[2].ensure(O ? O : 1) || g.id[3].ensure(O ? O : 1) || (rc = put_dev(c, g.names, names)) || (rc = to_dev(c, m.e_qname, t->qname, U)) || (rc = to_dev(c, m.e_tidname, tid_name, U)))
            return summary_no_room(c, "l2r_novel_names");
        hipError_t e = hipSuccess;
        if (O) {
            e = hipMemcpyAsync(g.tid.p, m.o_tid.p, O * 4, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(g.rev.p, m.o_rev.p, O, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(g.ex_off.p, m.u.ex_off.p, (O + 1) * 8, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess && X) e = hipMemcpyAsync(g.xs.p, m.xs.p, X * 4, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess && X) e = hipMemcpyAsync(g.xe.p, m.xe.p, X * 4, hipMemcpyDeviceToDevice, c->stream);
            for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemsetAsync(g.id[k].p, 0, O * 4, c->stream);
        }
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); return fail(-2, "[l2r_novel_names] %s", hipGetErrorString(e)); }
        if (U) hipLaunchKernelGGL(k_nov_gtf_ids, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, c->stream, (uint32_t)U, (uint32_t)O, (const int32_t *)m.u.u_src.p, (const int32_t *)m.o_ref.p,
                                  (const uint32_t *)m.genes.gid.p, (const uint32_t *)m.genes.gname.p, m.np.n_tx, na, base, (const uint32_t *)m.e_qname.p, (const uint32_t *)m.e_tidname.p,
                                  g.id[0].p, g.id[1].p, g.id[2].p, g.id[3].p);
        if ((rc = download_all(c, 0, {{g.h_nex.data(), m.o_nex.p, O * 4}, {sel.data(), m.u.u_src.p, U * 4}, {start.data(), m.u.u_start.p, U * 4}, {end.data(), m.u.u_end.p, U * 4}, {cov.data(), m.u.u_cov.p, U * 4}},
                               "l2r_novel_names"))) return rc;
        for (int k = 0; k < 4; ++k) g.id_p[k] = g.id[k].p;
        g.have_rows = true;
    }
    const l2r_gtx_blocks blk{(int64_t)U, sel.data(), start.data(), end.data(), cov.data()};
    if ((rc = l2r_gtftext_blocks(c, &blk, n_lines, n_bytes))) return rc;
    m.gtf_ready = true;
    return 0;
}

int l2r_novel_out(l2r_ctx *c, uint8_t *text, int64_t cap)
{
    if (!c) return fail(NOVEL_E_ARG, "[l2r_novel_out] null argument");
    if (c->novel.last_which == L2R_NOVEL_GTF) return l2r_gtftext_out(c, text, cap);
    return text_out(c, c->novel.text, text, cap, "l2r_novel_out", "l2r_novel_lines", NOVEL_E_ARG);
}

int l2r_novel_stats(l2r_ctx *c, double *out, int n) { return stats_out(c ? c->novel.stats : nullptr, NVS_N, out, n, "l2r_novel_stats"); }

}  // extern "C"

static_assert(sizeof(AccRec) == sizeof(l2r_accepted_read), "accepted record layout");
static_assert(sizeof(TxHdr) == 48, "TxHdr must be three int4");
static_assert(sizeof(SiteEnt) == 32 && sizeof(TileDesc) == 48, "dictionary entry / tile descriptor layout");

#include "l2r_xchg.hip.h"
