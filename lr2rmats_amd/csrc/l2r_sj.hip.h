// l2r_sj.hip.h -- the kernels of `bam2sj` (reference src/parse_bam.c:402-442 gen_sj, :339-380 sj_sch_group / sj_update_group,
// :319-337 intr_deri_str): junction rows from alignment records, ordered and counted on the device.
//
//   k_sj_count / k_sj_fill   one thread per record: the record filter and one walk over its CIGAR words; count -> k_scan_u32 ->
//                            fill writes the rows {tid, don, acc, uniq_c, multi_c} in record order (a compaction: most short reads
//                            carry no N operation)
//   k_sj_hist12              one pass over the keys: the histograms of all twelve key bytes (a byte that is equal in every key is
//                            a radix pass that is not run)
//   SjRows<OVER>             the rows of a radix pass of l2r_radix.hip.h: k_radix_digit_hist<SjRows<false>> reads the one column
//                            the pass's byte lives in, k_radix_scatter<SjRows<OVER>> moves the five (OVER: six) columns
//   k_sj_heads / k_sj_reduce head flags where the key changes -> k_scan_u32 -> per run the sums of the two count COLUMNS (so the same
//                            sort + reduce merges tables that were reduced before); a wave sums its part of a run by shuffles and
//                            adds it with one integer atomic, so a run may cross waves and workgroups and be of any length
//   k_sj_motif               per reduced row: four bases -> motif and strand; the first row on a sequence the genome lacks
//
// `sjtab` adds a sixth column, the overhang (the shorter of the two aligned blocks beside the junction), reduced by MAXIMUM: k_sj_fill,
// k_radix_scatter<SjRows> and k_sj_reduce have an OVER instance each that carries it (24 bytes per row and pass); the plain instances are the
// code above, unchanged.  Behind the reduction:
//   k_sj_introns             per annotation exon that is not the last of its transcript: the intron behind it as a row (sorted and made
//                            unique by the same passes, in a state of their own)
//   k_sj_annotate            per table row: binary search in the sorted intron keys -> anno 0 / 1
//   k_sj_keep / k_sj_take    the filter by category (annotated, or by motif) -> k_scan_u32 -> the nine columns of the kept rows, in order
//
// The second filter stage of `sjtab` (l2r_sj_filter_rows2; the rule is in include/lr2rmats_hip.h).  k_sj_keep has an INTRON instance that
// applies the intron-size rule as well; the plain instance is the code above, unchanged.  Over the rows that instance left:
//   SjAccKeyOf               k_radix_keys<SjAccKeyOf>: per row one 64-bit key (tid, acc) for the passes `sort` runs over SortRows
//                            (l2r_sort.hip.h), the histograms of its eight bytes and the descent word (no key below its predecessor: no pass runs)
//   k_sj_near_acc            per position of the acceptor order: the distance to the nearest other acceptor on the reference, from
//                            the two neighbours in that order (adjacent lanes by shuffles), written to the row's own slot
//   k_sj_keep_near           per row in table order: the distance to the nearest other donor from rows i - 1 and i + 1 (the table is in
//                            donor order inside a reference), the acceptor distance from the column above -> the keep words
//
// LSD radix with 8-bit digits over the 12-byte key (tid, don, acc), least significant byte of acc first; signed order (the top byte of
// every column is compared with its sign bit flipped).  HBM-bound integer work: a pass reads and writes 20 bytes per row.  No kernel
// waits for another workgroup.
#pragma once
#include "l2r_radix.hip.h"

namespace l2r {

constexpr int SJ_THREADS = RADIX_THREADS;
constexpr int SJ_KEY_BYTES = 12;

struct SjCols { int32_t *tid, *don, *acc, *uq, *mc, *ov; };      // ov: only the OVER instances touch it (null in a plain table)
struct SjPrm { int32_t min_intron, pair_only; };
struct SjRecs { int64_t n; const uint16_t *flag; const int32_t *tid, *pos; const uint8_t *uniq; const int64_t *cig_off; const uint32_t *cig; };

// src/parse_bam.c:909-914: unmapped records and, with read_type PAIR_T, records that are not properly paired are skipped
__device__ __forceinline__ bool sj_record_kept(uint32_t flag, const SjPrm &p) { return !(flag & 4u) && (!p.pair_only || (flag & 2u)); }

// gen_sj: `end` = last reference base so far (1-based); M = X D N grow it, an N of at least min_intron bases is a junction first
template <typename Emit>
__device__ __forceinline__ uint32_t sj_walk(const uint32_t *__restrict__ cig, int64_t c0, int64_t c1, int32_t pos, int32_t min_intron, Emit emit)
{
    int32_t end = pos;
    uint32_t k = 0;
    for (int64_t j = c0; j < c1; ++j) {
        const uint32_t w = cig[j], op = w & 0xfu; const int32_t len = (int32_t)(w >> 4);
        if (op == 3u && len >= min_intron) { emit(k, end + 1, end + len); ++k; }
        if ((0x18du >> op) & 1u) end += len;
    }
    return k;
}

__global__ __launch_bounds__(SJ_THREADS)
void k_sj_count(SjRecs r, SjPrm p, uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    uint32_t k = 0;
    if (sj_record_kept(r.flag[i], p)) k = sj_walk(r.cig, r.cig_off[i], r.cig_off[i + 1], r.pos[i], p.min_intron, [](uint32_t, int32_t, int32_t) {});
    cnt[i] = k;
}

// The overhang rule of `sjtab`: the junction operations cut the CIGAR into blocks, a block's length is the sum of its M = X lengths (I D
// S H P B and an N below min_intron add nothing and cut nothing), and a record's overhang at a junction is the shorter of the blocks on its
// two sides.  The right block is complete only at the next junction or at the end of the CIGAR: done(k, overhang) follows emit(k, ...)
// late.  An N that is the first or the last operation has an empty block beside it: overhang 0.
template <typename Emit, typename Done>
__device__ __forceinline__ uint32_t sj_walk_over(const uint32_t *__restrict__ cig, int64_t c0, int64_t c1, int32_t pos, int32_t min_intron, Emit emit, Done done)
{
    int32_t end = pos;
    uint32_t k = 0;
    int64_t blk = 0, left = 0;
    for (int64_t j = c0; j < c1; ++j) {
        const uint32_t w = cig[j], op = w & 0xfu; const int32_t len = (int32_t)(w >> 4);
        if (op == 3u && len >= min_intron) {
            if (k) done(k - 1, (int32_t)(left < blk ? left : blk));
            emit(k, end + 1, end + len); ++k;
            left = blk; blk = 0;
        } else if ((0x181u >> op) & 1u) blk = blk + len < 0x7fffffff ? blk + len : 0x7fffffff;
        if ((0x18du >> op) & 1u) end += len;
    }
    if (k) done(k - 1, (int32_t)(left < blk ? left : blk));
    return k;
}

// at[]: the scanned counts (n + 1 words); rows go to out[base + at[i] ...), never beyond `cap`.  OVER: the sixth column as well.
template <bool OVER>
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_fill(SjRecs r, SjPrm p, const uint32_t *__restrict__ at, SjCols out, int64_t base, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= r.n) return;
    const uint32_t a = at[i];
    if (at[i + 1] == a) return;
    const int32_t t = r.tid[i], u = r.uniq[i] ? 1 : 0;
    auto row = [&](uint32_t k, int32_t don, int32_t acc) {
        const int64_t o = base + a + k;
        if (o < cap) { out.tid[o] = t; out.don[o] = don; out.acc[o] = acc; out.uq[o] = u; out.mc[o] = 1 - u; }
    };
    if constexpr (OVER)
        sj_walk_over(r.cig, r.cig_off[i], r.cig_off[i + 1], r.pos[i], p.min_intron, row, [&](uint32_t k, int32_t over) {
            const int64_t o = base + a + k;
            if (o < cap) out.ov[o] = over;
        });
    else
        sj_walk(r.cig, r.cig_off[i], r.cig_off[i + 1], r.pos[i], p.min_intron, row);
}

// byte b (0 = least significant of acc ... 11 = most significant of tid) of a key, in unsigned order
__device__ __forceinline__ uint32_t sj_digit(int32_t tid, int32_t don, int32_t acc, int b)
{
    const uint32_t col = b < 4 ? (uint32_t)acc : b < 8 ? (uint32_t)don : (uint32_t)tid;
    return ((col ^ 0x80000000u) >> (8 * (b & 3))) & 0xffu;
}

// hist: 12 x 256 words, cleared by the caller
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_hist12(SjCols in, uint32_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[SJ_KEY_BYTES * 256];
    for (int k = threadIdx.x; k < SJ_KEY_BYTES * 256; k += SJ_THREADS) s_h[k] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x; i < n; i += gridDim.x * SJ_THREADS) {
        const int32_t t = in.tid[i], d = in.don[i], a = in.acc[i];
#pragma unroll
        for (int b = 0; b < SJ_KEY_BYTES; ++b) atomicAdd(&s_h[b * 256 + sj_digit(t, d, a, b)], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < SJ_KEY_BYTES * 256; k += SJ_THREADS) { const uint32_t v = s_h[k]; if (v) atomicAdd(&hist[k], v); }
}

// The rows of a pass (l2r_radix.hip.h).  OVER: the sixth column moves too.
template <bool OVER>
struct SjRows {
    SjCols in, out;
    struct Row { int32_t t, d, a, u, m, v; };
    static constexpr int HIST_UNROLL = RADIX_ROUNDS;
    __device__ __forceinline__ Row blank(uint32_t) const { return Row{0, 0, 0, 0, 0, 0}; }
    __device__ __forceinline__ Row load(uint32_t i) const
    {
        Row r{in.tid[i], in.don[i], in.acc[i], in.uq[i], in.mc[i], 0};
        if constexpr (OVER) r.v = in.ov[i];
        return r;
    }
    __device__ __forceinline__ uint32_t digit(const Row &r, int b) const { return sj_digit(r.t, r.d, r.a, b); }
    __device__ __forceinline__ uint32_t digit_at(uint32_t i, int b) const
    {
        const int32_t *__restrict__ col = b < 4 ? in.acc : b < 8 ? in.don : in.tid;
        return (((uint32_t)col[i] ^ 0x80000000u) >> (8 * (b & 3))) & 0xffu;
    }
    __device__ __forceinline__ void store(uint32_t o, const Row &r) const
    {
        out.tid[o] = r.t; out.don[o] = r.d; out.acc[o] = r.a; out.uq[o] = r.u; out.mc[o] = r.m;
        if constexpr (OVER) out.ov[o] = r.v;
    }
};

// head[i] = 1 where row i starts a run of equal keys (head has n + 1 words for the scan)
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_heads(SjCols in, uint32_t n, uint32_t *__restrict__ head)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0u || in.tid[i] != in.tid[i - 1] || in.don[i] != in.don[i - 1] || in.acc[i] != in.acc[i - 1]) ? 1u : 0u;
}

// before[]: head[] after its exclusive scan (before[n] = runs).  Row i belongs to run before[i + 1] - 1.  out.uq / out.mc are cleared by
// the caller; a wave adds up its rows of a run (segmented inclusive scan by shuffles) and the last lane of every such piece adds it.
// OVER: out.ov is cleared to 0 too (an overhang is never negative); the same scan takes the maximum of the sixth column and the piece's
// last lane hands it over with one atomicMax.
template <bool OVER>
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_reduce(SjCols in, uint32_t n, const uint32_t *__restrict__ before, SjCols out, uint32_t n_runs)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = i < n;
    uint32_t run = 0xffffffffu; int32_t u = 0, m = 0, v = 0;
    if (active) {
        run = before[i + 1] - 1u;
        u = in.uq[i]; m = in.mc[i]; if constexpr (OVER) v = in.ov[i];
        if (before[i] != before[i + 1] && run < n_runs) { out.tid[run] = in.tid[i]; out.don[run] = in.don[i]; out.acc[run] = in.acc[i]; }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t pr = (uint32_t)__shfl_up((int)run, s, 64);
        const int32_t pu = __shfl_up(u, s, 64), pm = __shfl_up(m, s, 64);
        if constexpr (OVER) {
            const int32_t pv = __shfl_up(v, s, 64);
            if (lane >= s && pr == run) { u += pu; m += pm; v = pv > v ? pv : v; }
        } else {
            if (lane >= s && pr == run) { u += pu; m += pm; }
        }
    }
    const uint32_t next = (uint32_t)__shfl_down((int)run, 1, 64);
    if (active && (lane == 63 || next != run) && run < n_runs) {
        if (u) atomicAdd(&out.uq[run], u);
        if (m) atomicAdd(&out.mc[run], m);
        if constexpr (OVER) { if (v > 0) atomicMax(&out.ov[run], v); }
    }
}

struct SjGenome { int32_t n_seq; const int64_t *seq_off; const uint8_t *bases; };

// src/parse_bam.c:319-337 with the table of src/parse_bam.c's intron_motif / intron_motif_strand.  A base outside its sequence matches
// nothing.  bad_row: the smallest row index on a sequence the genome does not have (cleared to 0xffffffff by the caller).
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_motif(const int32_t *__restrict__ tid, const int32_t *__restrict__ don, const int32_t *__restrict__ acc, uint32_t n, SjGenome g,
                uint8_t *__restrict__ strand, uint8_t *__restrict__ motif, uint32_t *__restrict__ bad_row)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    uint8_t mo = 0, st = 0;
    if (g.n_seq > 0) {
        const int32_t t = tid[i];
        if (t >= g.n_seq) atomicMin(bad_row, i);
        else if (t >= 0) {
            const int64_t s0 = g.seq_off[t], len = g.seq_off[t + 1] - s0;
            const int64_t at[4] = {(int64_t)don[i] - 1, (int64_t)don[i], (int64_t)acc[i] - 2, (int64_t)acc[i] - 1};
            uint32_t word = 0; bool inside = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t c = 0;
                if (at[k] >= 0 && at[k] < len) c = g.bases[s0 + at[k]]; else inside = false;
                if (c >= 'a' && c <= 'z') c -= 32u;
                word = (word << 8) | c;
            }
#define SJ_M4(a, b, c, d) (((uint32_t)(a) << 24) | ((uint32_t)(b) << 16) | ((uint32_t)(c) << 8) | (uint32_t)(d))
            if (inside) {
                switch (word) {
                case SJ_M4('G', 'T', 'A', 'G'): mo = 1; st = 1; break;
                case SJ_M4('C', 'T', 'A', 'C'): mo = 2; st = 2; break;
                case SJ_M4('G', 'C', 'A', 'G'): mo = 3; st = 1; break;
                case SJ_M4('C', 'T', 'G', 'C'): mo = 4; st = 2; break;
                case SJ_M4('A', 'T', 'A', 'C'): mo = 5; st = 1; break;
                case SJ_M4('G', 'T', 'A', 'T'): mo = 6; st = 2; break;
                default: break;
                }
            }
#undef SJ_M4
        }
    }
    strand[i] = st; motif[i] = mo;
}

// ---- `sjtab`: annotated flag, filter

struct SjAnno { int64_t n_tx, n_exon; const int32_t *tx_tid; const int64_t *tx_ex_off; const int32_t *ex_start, *ex_end; };

// One thread per exon.  Its transcript: the last t with tx_ex_off[t] <= e (transcripts without exons share an offset with their
// successor and are stepped over by the search).  Not the last exon of a transcript with tid >= 0 -> the interval up to the next exon, where
// it is not empty, as a row {tid, first base, last base, 1, 0} at a slot taken from *count (any order: the rows are sorted next).
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_introns(SjAnno a, SjCols out, uint32_t *__restrict__ count, uint32_t cap)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_exon) return;
    int64_t lo = 0, hi = a.n_tx;                                  // tx_ex_off[lo] <= e < tx_ex_off[hi]
    while (hi - lo > 1) { const int64_t mid = lo + (hi - lo) / 2; if (a.tx_ex_off[mid] <= e) lo = mid; else hi = mid; }
    if (e + 1 >= a.tx_ex_off[lo + 1]) return;
    const int32_t t = a.tx_tid[lo];
    if (t < 0) return;
    const int64_t first = (int64_t)a.ex_end[e] + 1, last = (int64_t)a.ex_start[e + 1] - 1;
    if (last < first) return;
    const uint32_t o = atomicAdd(count, 1u);
    if (o < cap) { out.tid[o] = t; out.don[o] = (int32_t)first; out.acc[o] = (int32_t)last; out.uq[o] = 1; out.mc[o] = 0; }
}

// in: the sorted, distinct intron keys
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_annotate(const int32_t *__restrict__ tid, const int32_t *__restrict__ don, const int32_t *__restrict__ acc, uint32_t n,
                   SjCols in, uint32_t n_in, uint8_t *__restrict__ anno)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t t = tid[i], d = don[i], a = acc[i];
    uint32_t lo = 0, hi = n_in;                                   // the first key that is not below (t, d, a)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int32_t mt = in.tid[mid], md = in.don[mid], ma = in.acc[mid];
        const bool below = mt != t ? mt < t : md != d ? md < d : ma < a;
        if (below) lo = mid + 1; else hi = mid;
    }
    anno[i] = (lo < n_in && in.tid[lo] == t && in.don[lo] == d && in.acc[lo] == a) ? 1 : 0;
}

struct SjFilter { int32_t anchor_min[5], uniq_min[5], all_min[5]; };
struct SjFilter2 { int32_t dist_min[5], n_intron_max, intron_max[8]; };

// category: annotated 0; else by motif: 0 -> 1, 1 2 -> 2, 3 4 -> 3, 5 6 -> 4.  keep has n + 1 words for the scan.
// INTRON: a row of category 1..4 seen by reads = max(1, uniq_c + multi_c) <= n_intron_max records stays only where its intron is no
// longer than intron_max[reads - 1]; *n_long counts the rows that this rule alone drops (one atomic per wave).
template <bool INTRON>
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_keep(SjCols in, const uint8_t *__restrict__ motif, const uint8_t *__restrict__ anno, uint32_t n, SjFilter f, SjFilter2 g, uint32_t *__restrict__ keep,
               uint32_t *__restrict__ n_long)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if constexpr (!INTRON) {
        if (i >= n) return;
        const uint32_t mo = motif[i];
        const int c = anno[i] ? 0 : mo == 0u ? 1 : mo > 6u ? 1 : (int)((mo + 1u) / 2u) + 1;
        const int64_t u = in.uq[i], all = (int64_t)in.uq[i] + in.mc[i];
        keep[i] = (in.ov[i] >= f.anchor_min[c] && (u >= f.uniq_min[c] || all >= f.all_min[c])) ? 1u : 0u;
    } else {
        bool stays = false, too_long = false;
        if (i < n) {
            const uint32_t mo = motif[i];
            const int c = anno[i] ? 0 : mo == 0u ? 1 : mo > 6u ? 1 : (int)((mo + 1u) / 2u) + 1;
            const int64_t u = in.uq[i], all = (int64_t)in.uq[i] + in.mc[i];
            stays = in.ov[i] >= f.anchor_min[c] && (u >= f.uniq_min[c] || all >= f.all_min[c]);
            const int64_t reads = all > 1 ? all : 1, len = (int64_t)in.acc[i] - in.don[i] + 1;
            if (c != 0 && reads <= g.n_intron_max) {
                int64_t lim = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) if (reads == k + 1) lim = g.intron_max[k];        // (constant indices: the list stays in scalar registers)
                too_long = len > lim;
            }
            keep[i] = (stays && !too_long) ? 1u : 0u;
        }
        const unsigned long long hit = __ballot(stays && too_long);
        if (hit && (threadIdx.x & 63) == 0) atomicAdd(n_long, (uint32_t)__popcll(hit));
    }
}

// the (tid, acc) key of the acceptor order: each column with its sign bit flipped, as sj_digit has it
__device__ __forceinline__ uint64_t sj_acc_key(int32_t tid, int32_t acc)
{
    return ((uint64_t)((uint32_t)tid ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)acc ^ 0x80000000u);
}

struct SjAccKeyOf {
    const int32_t *tid, *acc;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return sj_acc_key(tid[i], acc[i]); }
};

constexpr int32_t SJ_FAR = 0x7fffffff;                   // no other row on the reference

__device__ __forceinline__ int32_t sj_gap(int32_t a, int32_t b)
{
    const int64_t d = (int64_t)a - (int64_t)b, m = d < 0 ? -d : d;
    return m < (int64_t)SJ_FAR ? (int32_t)m : SJ_FAR;
}

// idx: the acceptor order (idx[j] = row at rank j), or null where the rows are in that order as they stand.  Thread j holds the row at
// rank j; its neighbours at ranks j - 1 and j + 1 sit in the adjacent lanes, and only the first and the last lane of a wave load theirs.
// The last radix pass writes the index column alone, so there is no sorted key column to read the neighbours from.
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_near_acc(const int32_t *__restrict__ tid, const int32_t *__restrict__ acc, const uint32_t *__restrict__ idx, uint32_t n, int32_t *__restrict__ da)
{
    const uint32_t j = blockIdx.x * SJ_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = j < n;
    uint32_t r = 0; int32_t t = 0, a = 0;
    if (active) { r = idx ? idx[j] : j; if (r >= n) r = n - 1u; t = tid[r]; a = acc[r]; }
    int32_t pt = __shfl_up(t, 1, 64), pa = __shfl_up(a, 1, 64), nt = __shfl_down(t, 1, 64), na = __shfl_down(a, 1, 64);
    if (!active) return;
    const bool has_prev = j > 0u, has_next = j + 1u < n;
    if (lane == 0 && has_prev) { uint32_t q = idx ? idx[j - 1u] : j - 1u; if (q >= n) q = n - 1u; pt = tid[q]; pa = acc[q]; }
    if (lane == 63 && has_next) { uint32_t q = idx ? idx[j + 1u] : j + 1u; if (q >= n) q = n - 1u; nt = tid[q]; na = acc[q]; }
    int32_t d = SJ_FAR;
    if (has_prev && pt == t) d = sj_gap(a, pa);
    if (has_next && nt == t) { const int32_t e = sj_gap(na, a); d = e < d ? e : d; }
    da[r] = d;
}

// A row of category c stays iff both distances are at least dist_min[c].  Rows i - 1 and i + 1 hold the nearest other donors of the
// reference: the table is sorted by (tid, don, acc).  keep has n + 1 words for the scan.
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_keep_near(const int32_t *__restrict__ tid, const int32_t *__restrict__ don, const int32_t *__restrict__ da, const uint8_t *__restrict__ motif,
                    const uint8_t *__restrict__ anno, uint32_t n, SjFilter2 g, uint32_t *__restrict__ keep)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t mo = motif[i];
    const int c = anno[i] ? 0 : mo == 0u ? 1 : mo > 6u ? 1 : (int)((mo + 1u) / 2u) + 1;
    int32_t lim = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) if (c == k) lim = g.dist_min[k];
    const int32_t t = tid[i], d = don[i];
    int32_t dd = SJ_FAR;
    if (i > 0u && tid[i - 1u] == t) dd = sj_gap(d, don[i - 1u]);
    if (i + 1u < n && tid[i + 1u] == t) { const int32_t e = sj_gap(don[i + 1u], d); dd = e < dd ? e : dd; }
    keep[i] = (dd >= lim && da[i] >= lim) ? 1u : 0u;
}

struct SjBytes { uint8_t *strand, *motif, *anno; };

// at[]: keep[] after its exclusive scan
__global__ __launch_bounds__(SJ_THREADS)
void k_sj_take(SjCols in, SjBytes bin, uint32_t n, const uint32_t *__restrict__ at, SjCols out, SjBytes bout, uint32_t n_out)
{
    const uint32_t i = blockIdx.x * SJ_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = at[i];
    if (at[i + 1] == o || o >= n_out) return;
    out.tid[o] = in.tid[i]; out.don[o] = in.don[i]; out.acc[o] = in.acc[i]; out.uq[o] = in.uq[i]; out.mc[o] = in.mc[i]; out.ov[o] = in.ov[i];
    bout.strand[o] = bin.strand[i]; bout.motif[o] = bin.motif[i]; bout.anno[o] = bin.anno[i];
}

}  // namespace l2r
