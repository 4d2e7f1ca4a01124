// l2r_novel.hip.h -- the kernels of l2r_novel_add / _finish / _lines (the novel list of `update-gtf`, include/lr2rmats_hip.h): the offers
// and known reads of every shard selected where its results lie, the offers merged as one merge_trans list by the kernels of
// l2r_uniq.hip.h, the items of the six lists made from the entries' widened chains, the first item of every key kept in the order of first
// appearance, and the BED text of the kept exon rows.  The rule: l2r_novelplan.hip.h.
//
// The selection, per add:
//   k_nov_flag       one thread per read: its bits (offer, known, split-route), the exons an offer brings (0 otherwise); per tile of 256
//                    reads the offers and the known reads (cnt[tile], cnt[n_tiles + tile]: ONE exclusive scan gives every tile its first
//                    rank of both); the split-route reads counted; the smallest read with a tid outside the table, no exon, or a ref
//                    beyond the annotation
//   (k_scan_u32 over the exons of the offers: where every chain goes; over the tile counts)
//   k_nov_place      the rank of every offer and known read: the tile's base + the like in front of it in the tile (ballots inside the
//                    wave, the waves in front through LDS) -- input order.  At the rank, behind what the accumulators hold: tid, strand,
//                    ref, global read index, exon count; (tid, gene) of a known read
//   k_nov_chain      an offer's chain and flags copied behind the accumulated ones; the smallest offer with a negative coordinate.
//                    Thread form: one thread per read.  Wave form: one wave per read, lanes over exons, coalesced
// The finish:
//   k_nov_widen      the scanned exon counts as the 64-bit offsets UniqIn takes
//   (k_uniq_heads .. k_uniq_take of l2r_uniq.hip.h, unchanged, over the accumulated columns)
//   k_nov_descends   whether tid descends anywhere over the known reads
//   k_nov_count      one thread per entry: its items of the lists exon, donor, acceptor, junction, gene (cnt[list * U + entry]: one scan
//                    gives every list its items one behind the other, in entry order); the entries a hit has widened
//   k_nov_emit       one thread per entry: its items' keys (list << 29 | tid, a, b) at their ordinals, from the chain with the first
//                    start and the last end as the hits left them; an exon item carries the entry's coverage, its type and strand
//   k_nov_emit_known the known reads' (tid, gene) behind them
//   (order_by_keys on b, then on (list << 29 | tid) << 32 | a read through the first order, k_gtf_compose: stable, so equal keys stand
//    in item order)
//   k_nov_heads      row r of the order is a head where its key differs from row r - 1's
//   k_nov_groups     behind the scan of the heads: a head's item -- the first of its key in ITEM order -- is flagged at its own ordinal
//                    and told its group; every exon item adds its coverage to its group's sum (integer atomics: exact in any order)
//   k_nov_keep       behind the scan of the flags in item order: the flagged items compacted -- the kept rows of the six lists one
//                    behind the other, each in the order of first appearance, with no second sort
// The text:
//   k_nov_bed_measure  one thread per kept exon row: the bytes of its line
//   k_nov_bed_write    one workgroup per NOV_BED_TILE rows composes their lines in an LDS image and streams it out (l2r_text.hip.h); a
//                      tile with more text than the image holds writes its lines straight to the text
// wave64, 256-thread workgroups, plain stores; no kernel waits for another workgroup.  Every index that comes out of a column is checked
// against its bound before it is used as an address.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l2r_kernels.hip.h"
#include "l2r_novelplan.hip.h"
#include "l2r_text.hip.h"

namespace l2r {

constexpr int NOV_TILE = 256;                           // reads, and threads, of one tile of the selection
static_assert(NOV_TILE == 4 * WAVE, "k_nov_flag / k_nov_place: four waves per tile");
constexpr int NOV_BED_TILE = 256;                       // rows, and threads, of one workgroup of k_nov_bed_write
constexpr uint32_t NOV_BED_LDS = 32768;                 // bytes of a tile's text the LDS image holds

enum { NOV_BIT_OFFER = 1, NOV_BIT_KNOWN = 2, NOV_BIT_SPLIT = 4 };
// words of the counter block of an add ...
enum { NOVW_SPLIT = 0, NOVW_EXONS, NOVW_TILES, NOVW_N };
// ... of the finish ...
enum { NOVF_EXONS = 0, NOVF_DESCENDS, NOVF_WIDENED, NOVF_ITEMS, NOVF_GROUPS, NOVF_ROWS, NOVF_N };
// ... and of k_nov_bed_write, with the scan's total behind them
enum { NOVC_OUTSIDE = 0, NOVC_DIRECT, NOVC_N };

__device__ __forceinline__ void nov_flag_bad(unsigned long long *bad, int64_t read, int kind)
{
    atomicMin(bad, (unsigned long long)read << 4 | (unsigned long long)kind);
}

// The reads of one add and where their selection goes.  o0, k0, x0: what the accumulators hold; o_room, k_room, x_room: what they have
// room for.  n_off / n_known: the add's offers and known reads (k_nov_place, k_nov_chain: from the scan of the tile counts)
struct NovSel {
    int64_t n, read_base;
    const int32_t *tid; const uint32_t *info, *ex_off; const int32_t *ref_tx, *xs, *xe; const uint8_t *f;
    uint32_t src_exons;
    int32_t n_ref; int64_t n_tx; const uint32_t *tx_gene; uint32_t na_gene; int32_t has_sj, split;
    uint8_t *bits; uint32_t *cnt_x, *tile_cnt; int64_t n_tiles;
    uint32_t n_off, n_known;
    uint64_t o0, k0, x0, o_room, k_room, x_room;
    int32_t *o_tid, *o_ref, *o_read; uint8_t *o_rev; uint32_t *o_nex;
    int32_t *a_xs, *a_xe; uint8_t *a_f;
    int32_t *k_tid; uint32_t *k_gene;
    uint32_t *word; unsigned long long *bad;
};

__global__ __launch_bounds__(NOV_TILE)
void k_nov_flag(NovSel s)
{
    __shared__ uint32_t s_cnt[NOV_TILE / WAVE][2];
    const int64_t i = (int64_t)blockIdx.x * NOV_TILE + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1)), w = (int)(threadIdx.x >> 6);
    uint32_t b = 0u;
    if (i < s.n) {
        const uint32_t info = s.info[i];
        const int kind = novel_read_kind(s.tid[i], info, s.ref_tx[i], s.n_ref, s.n_tx);
        if (kind) nov_flag_bad(s.bad, s.read_base + i, kind);
        else b = (novel_offer(info, s.has_sj) ? NOV_BIT_OFFER : 0u) | (novel_known(info) ? NOV_BIT_KNOWN : 0u) | (novel_split(info, s.has_sj, s.split) ? NOV_BIT_SPLIT : 0u);
        s.bits[i] = (uint8_t)b;
        s.cnt_x[i] = (b & NOV_BIT_OFFER) ? L2R_INFO_NEXON(info) : 0u;
    }
    const uint32_t n_o = (uint32_t)__popcll(__ballot((b & NOV_BIT_OFFER) != 0u)), n_k = (uint32_t)__popcll(__ballot((b & NOV_BIT_KNOWN) != 0u));
    const uint32_t n_s = (uint32_t)__popcll(__ballot((b & NOV_BIT_SPLIT) != 0u));
    if (lane == 0) { s_cnt[w][0] = n_o; s_cnt[w][1] = n_k; if (n_s) atomicAdd(s.word + NOVW_SPLIT, n_s); }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t sum = 0;
        for (int q = 0; q < NOV_TILE / WAVE; ++q) sum += s_cnt[q][threadIdx.x];
        s.tile_cnt[(int64_t)threadIdx.x * s.n_tiles + blockIdx.x] = sum;
    }
}

// tile_cnt: scanned.  The known reads' ranks start behind the n_off offers of the scan
__global__ __launch_bounds__(NOV_TILE)
void k_nov_place(NovSel s)
{
    __shared__ uint32_t s_cnt[NOV_TILE / WAVE][2];
    const int64_t i = (int64_t)blockIdx.x * NOV_TILE + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1)), w = (int)(threadIdx.x >> 6);
    const uint32_t b = i < s.n ? (uint32_t)s.bits[i] : 0u;
    const unsigned long long m_o = __ballot((b & NOV_BIT_OFFER) != 0u), m_k = __ballot((b & NOV_BIT_KNOWN) != 0u);
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t before_o = (uint32_t)__popcll(m_o & below), before_k = (uint32_t)__popcll(m_k & below);
    if (lane == 0) { s_cnt[w][0] = (uint32_t)__popcll(m_o); s_cnt[w][1] = (uint32_t)__popcll(m_k); }
    __syncthreads();
    if (i >= s.n) return;
    for (int q = 0; q < w; ++q) { before_o += s_cnt[q][0]; before_k += s_cnt[q][1]; }
    if (b & NOV_BIT_OFFER) {
        const uint32_t r = s.tile_cnt[blockIdx.x] + before_o;
        if (r < s.n_off && s.o0 + r < s.o_room) {           // (cannot fail: the counts add up to n_off, the host has made the room)
            const uint64_t at = s.o0 + r;
            const uint32_t info = s.info[i];
            s.o_tid[at] = s.tid[i]; s.o_ref[at] = s.ref_tx[i]; s.o_read[at] = (int32_t)(s.read_base + i); s.o_rev[at] = (info & L2R_INFO_REV) ? 1 : 0; s.o_nex[at] = L2R_INFO_NEXON(info);
        }
    }
    if (b & NOV_BIT_KNOWN) {
        const uint32_t r = s.tile_cnt[s.n_tiles + blockIdx.x] - s.n_off + before_k;
        if (r < s.n_known && s.k0 + r < s.k_room) {
            const uint64_t at = s.k0 + r;
            s.k_tid[at] = s.tid[i]; s.k_gene[at] = novel_gene(s.ref_tx[i], s.tx_gene, s.na_gene);      // (ref < n_tx: k_nov_flag has looked)
        }
    }
}

// cnt_x: scanned
template <bool BY_WAVE>
__global__ __launch_bounds__(256)
void k_nov_chain(NovSel s)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = BY_WAVE ? t >> 6 : t;
    if (i >= s.n) return;                               // (BY_WAVE: the whole wave)
    if (!(s.bits[i] & NOV_BIT_OFFER)) return;
    const int lane = BY_WAVE ? (int)(threadIdx.x & (WAVE - 1)) : 0;
    const uint32_t k = L2R_INFO_NEXON(s.info[i]), s0 = s.ex_off[i];
    const uint64_t d0 = s.x0 + s.cnt_x[i];
    if ((uint64_t)s0 + k > (uint64_t)s.src_exons || d0 + k > s.x_room) return;      // (cannot be: the host has compared the totals and made the room)
    int32_t sign = 0;
    for (uint32_t j = (uint32_t)lane; j < k; j += BY_WAVE ? WAVE : 1) {
        const int32_t a = s.xs[s0 + j], e = s.xe[s0 + j];
        s.a_xs[d0 + j] = a; s.a_xe[d0 + j] = e; s.a_f[d0 + j] = s.f[s0 + j];
        sign |= a | e;
    }
    if (sign < 0) nov_flag_bad(s.bad, s.read_base + i, NOV_E_NEGATIVE);
}

__global__ __launch_bounds__(256)
void k_nov_widen(int64_t n, const uint32_t *__restrict__ off32, int64_t *__restrict__ off64)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) off64[i] = (int64_t)off32[i];
}

__global__ __launch_bounds__(256)
void k_nov_descends(int64_t n, const int32_t *__restrict__ k_tid, uint32_t *__restrict__ word)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > 0 && i < n && k_tid[i] < k_tid[i - 1]) word[NOVF_DESCENDS] = 1u;
}

// The entries and the offers behind them, and where the items go
struct NovItems {
    uint32_t n_entries, n_offers, n_exons, n_known, n_items, base_known;
    const int32_t *u_src, *u_start, *u_end, *u_cov;     // per entry (k_uniq_take)
    const int32_t *o_tid, *o_ref, *o_read; const uint8_t *o_rev; const uint32_t *o_nex, *o_off;      // per offer; o_off: n_offers + 1
    const int32_t *xs, *xe; const uint8_t *f;
    const int32_t *k_tid; const uint32_t *k_gene;
    const uint32_t *tx_gene; uint32_t na_gene;
    uint32_t *cnt;                                      // NOV_GENE + 1 lists x n_entries (+ 1), scanned in place
    uint32_t *hi, *a, *b, *cov; uint8_t *meta;          // per item
    int32_t *e_src;                                     // per entry: the read that created it
    uint32_t *word;
};

// the chain of entry e: false where a column names what does not exist (cannot be)
__device__ __forceinline__ bool nov_entry(const NovItems &t, uint32_t e, uint32_t &o, uint32_t &x0, uint32_t &n)
{
    o = (uint32_t)t.u_src[e];
    if (o >= t.n_offers) return false;
    x0 = t.o_off[o]; n = t.o_nex[o];
    return n > 0u && (uint64_t)x0 + n <= (uint64_t)t.n_exons;
}

__global__ __launch_bounds__(256)
void k_nov_count(NovItems t)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    bool wide = false;
    if (e < t.n_entries) {
        uint32_t o, x0, n, c[4] = {0u, 0u, 0u, 0u};
        if (nov_entry(t, e, o, x0, n)) {
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t f = t.f[x0 + j];
                c[NOV_EXON] += (f & L2R_EXF_NOVEL_EXON) ? 1u : 0u;
                if (j + 1u < n) { c[NOV_DON] += (f & L2R_EXF_NOVEL_DON) ? 1u : 0u; c[NOV_ACC] += (f & L2R_EXF_NOVEL_ACC) ? 1u : 0u; c[NOV_JUNC] += (f & L2R_EXF_NOVEL_JUNC) ? 1u : 0u; }
            }
            wide = t.xs[x0] != t.u_start[e] || t.xe[x0 + n - 1u] != t.u_end[e];
            t.e_src[e] = t.o_read[o];
        } else t.e_src[e] = -1;
#pragma unroll
        for (int l = 0; l < 4; ++l) t.cnt[(uint64_t)l * t.n_entries + e] = c[l];
        t.cnt[(uint64_t)NOV_GENE * t.n_entries + e] = 1u;
    }
    const uint32_t n_wide = (uint32_t)__popcll(__ballot(wide));
    if (lane == 0 && n_wide) atomicAdd(t.word + NOVF_WIDENED, n_wide);
}

__device__ __forceinline__ void nov_put(const NovItems &t, uint32_t p, int list, int32_t tid, int32_t a, int32_t b, uint32_t cov, uint32_t meta)
{
    if (p >= t.n_items) return;                         // (cannot be: the ordinals come from the scan of the counts)
    t.hi[p] = (uint32_t)list << NOV_TID_BITS | (uint32_t)tid; t.a[p] = (uint32_t)a; t.b[p] = (uint32_t)b; t.cov[p] = cov; t.meta[p] = (uint8_t)meta;
}

// cnt: scanned
__global__ __launch_bounds__(256)
void k_nov_emit(NovItems t)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= t.n_entries) return;
    uint32_t o, x0, n;
    if (!nov_entry(t, e, o, x0, n)) return;
    uint32_t p[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) p[l] = t.cnt[(uint64_t)l * t.n_entries + e];
    const int32_t tid = t.o_tid[o], first = t.u_start[e], last = t.u_end[e];
    const uint32_t cov = (uint32_t)t.u_cov[e], rev = t.o_rev[o];
    nov_put(t, t.cnt[(uint64_t)NOV_GENE * t.n_entries + e], NOV_GENE, tid, (int32_t)novel_gene(t.o_ref[o], t.tx_gene, t.na_gene), 0, 0u, 0u);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t f = t.f[x0 + j];
        const int32_t s = j == 0u ? first : t.xs[x0 + j], en = j == n - 1u ? last : t.xe[x0 + j];
        if (f & L2R_EXF_NOVEL_EXON) nov_put(t, p[NOV_EXON]++, NOV_EXON, tid, s, en, cov, (uint32_t)novel_exon_type(j, n) | rev << 2);
        if (j + 1u < n) {
            const int32_t next = t.xs[x0 + j + 1u];       // (j + 1 >= 1: never the widened start)
            if (f & L2R_EXF_NOVEL_DON) nov_put(t, p[NOV_DON]++, NOV_DON, tid, en, 0, 0u, 0u);
            if (f & L2R_EXF_NOVEL_ACC) nov_put(t, p[NOV_ACC]++, NOV_ACC, tid, next, 0, 0u, 0u);
            if (f & L2R_EXF_NOVEL_JUNC) nov_put(t, p[NOV_JUNC]++, NOV_JUNC, tid, en, next, 0u, 0u);
        }
    }
}

__global__ __launch_bounds__(256)
void k_nov_emit_known(NovItems t)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < t.n_known) nov_put(t, t.base_known + i, NOV_KNOWN_GENE, t.k_tid[i], (int32_t)t.k_gene[i], 0, 0u, 0u);
}

// the keys of the two stable stages: b, then (list << 29 | tid) << 32 | a read through the first stage's order (null: the identity)
struct NovLowKeyOf {
    const uint32_t *__restrict__ b;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return (uint64_t)b[i]; }
};
struct NovHighKeyOf {
    const uint32_t *__restrict__ hi, *__restrict__ a, *__restrict__ order1; uint32_t n;
    __device__ __forceinline__ uint64_t key(int64_t i) const
    {
        uint32_t r = order1 ? order1[i] : (uint32_t)i;
        if (r >= n) r = n - 1u;
        return (uint64_t)hi[r] << 32 | (uint64_t)a[r];
    }
};

struct NovKeys { uint32_t n; const uint32_t *order, *hi, *a, *b; };

// head[r] (n + 1 words, scanned next)
__global__ __launch_bounds__(256)
void k_nov_heads(NovKeys k, uint32_t *__restrict__ head)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= k.n) return;
    uint32_t i = k.order[r], j = r ? k.order[r - 1u] : 0u;
    if (i >= k.n) i = k.n - 1u;
    if (j >= k.n) j = k.n - 1u;
    head[r] = (r == 0u || k.hi[i] != k.hi[j] || k.a[i] != k.a[j] || k.b[i] != k.b[j]) ? 1u : 0u;
}

// before: the scanned heads.  first (n + 1 words) and sum (n words) are zeroed
__global__ __launch_bounds__(256)
void k_nov_groups(NovKeys k, const uint32_t *__restrict__ before, const uint32_t *__restrict__ cov, uint32_t *__restrict__ first, uint32_t *__restrict__ grp, uint32_t *__restrict__ sum)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= k.n) return;
    const uint32_t i = k.order[r], g = before[r + 1u] - 1u;
    if (i >= k.n || g >= k.n) return;
    if (before[r + 1u] != before[r]) { first[i] = 1u; grp[i] = g; }
    if ((k.hi[i] >> NOV_TID_BITS) == (uint32_t)NOV_EXON) atomicAdd(sum + g, cov[i]);
}

struct NovRows { int32_t *tid, *a, *b, *score; uint8_t *meta; };

// rank: the scanned flags, in item order
__global__ __launch_bounds__(256)
void k_nov_keep(NovKeys k, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ grp, const uint32_t *__restrict__ sum, const uint8_t *__restrict__ meta, uint32_t n_rows, NovRows out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.n) return;
    const uint32_t q = rank[i];
    if (rank[i + 1u] == q || q >= n_rows) return;
    const uint32_t hi = k.hi[i], g = grp[i];
    out.tid[q] = (int32_t)(hi & ((1u << NOV_TID_BITS) - 1u)); out.a[q] = (int32_t)k.a[i]; out.b[q] = (int32_t)k.b[i];
    out.score[q] = (hi >> NOV_TID_BITS) == (uint32_t)NOV_EXON && g < k.n ? (int32_t)sum[g] : 0;
    out.meta[q] = meta[i];
}

// The name ids of the GTF-text unit's rows (the offers) from the entries: id0 / id2 the gene id / gene name of the offer's ref in the
// annotation's part of the table (na: the `NA` behind it), id1 / id3 the entry's tid_name / qname in the caller's part (from base on)
__global__ __launch_bounds__(256)
void k_nov_gtf_ids(uint32_t n_entries, uint32_t n_offers, const int32_t *__restrict__ u_src, const int32_t *__restrict__ o_ref, const uint32_t *__restrict__ tx_gid,
                   const uint32_t *__restrict__ tx_gname, int64_t n_tx, uint32_t na, uint32_t base, const uint32_t *__restrict__ qname, const uint32_t *__restrict__ tid_name,
                   uint32_t *__restrict__ id0, uint32_t *__restrict__ id1, uint32_t *__restrict__ id2, uint32_t *__restrict__ id3)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n_entries) return;
    const uint32_t o = (uint32_t)u_src[e];
    if (o >= n_offers) return;                          // (cannot be)
    const int32_t ref = o_ref[o];
    const bool has = ref >= 0 && (int64_t)ref < n_tx;
    id0[o] = has ? tx_gid[ref] : na; id2[o] = has ? tx_gname[ref] : na;
    id1[o] = base + tid_name[e]; id3[o] = base + qname[e];
}

// ---- the BED text of the kept exon rows
struct NovBed { uint32_t n; const int32_t *tid, *start, *end, *score; const uint8_t *meta; int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names; };

__device__ __forceinline__ uint32_t nov_digits(int32_t v) { return v < 0 ? 1u + text_digits(0u - (uint32_t)v) : text_digits((uint32_t)v); }
__device__ __forceinline__ uint8_t *nov_put_int(uint8_t *p, int32_t v)
{
    if (v < 0) { *p++ = '-'; return text_put_num(p, 0u - (uint32_t)v); }
    return text_put_num(p, (uint32_t)v);
}
__device__ __forceinline__ uint32_t nov_bed_len(const NovBed &in, uint32_t q)
{
    const int32_t tid = in.tid[q];
    if (tid < 0 || tid >= in.n_ref) return 0u;          // (cannot be: the selection has looked)
    return (uint32_t)(in.ref_off[tid + 1] - in.ref_off[tid]) + nov_digits(in.start[q] - 1) + nov_digits(in.end[q]) + nov_digits(in.score[q]) + 13u;
}

__global__ __launch_bounds__(256)
void k_nov_bed_measure(NovBed in, uint32_t *__restrict__ len)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < in.n) len[q] = nov_bed_len(in, q);
}

// the line of row q at dst: exactly the bytes nov_bed_len counted; returns the byte behind it
__device__ __forceinline__ uint8_t *nov_bed_line(uint8_t *dst, const NovBed &in, uint32_t q)
{
    const int32_t tid = in.tid[q];
    const uint32_t m = in.meta[q];
    uint8_t *p = dst;
    for (int64_t k = in.ref_off[tid]; k < in.ref_off[tid + 1]; ++k) *p++ = in.ref_names[k];
    *p++ = '\t'; p = nov_put_int(p, in.start[q] - 1); *p++ = '\t'; p = nov_put_int(p, in.end[q]); *p++ = '\t';
    *p++ = (m & 3u) == (uint32_t)NOV_TYPE_T ? 'T' : (m & 3u) == (uint32_t)NOV_TYPE_I ? 'I' : 'S';
    p = text_put_lit(p, "_exon\t");
    p = nov_put_int(p, in.score[q]); *p++ = '\t'; *p++ = (m & 4u) ? '-' : '+'; *p++ = '\n';
    return p;
}

// rows [first, first + take); off: their scanned lengths (take + 1 words)
__global__ __launch_bounds__(NOV_BED_TILE)
void k_nov_bed_write(NovBed in, int64_t first, int64_t take, const uint32_t *__restrict__ off, uint8_t *__restrict__ text, uint32_t *__restrict__ word)
{
    __shared__ uint4 s_img[NOV_BED_LDS / 16 + 1];       // the image of the tile's span (l2r_text.hip.h)
    const int64_t i0 = (int64_t)blockIdx.x * NOV_BED_TILE, i1 = i0 + NOV_BED_TILE < take ? i0 + NOV_BED_TILE : take;
    const uint32_t b0 = off[i0], b1 = off[i1], bytes = b1 - b0;
    if (bytes == 0u) return;
    const bool direct = bytes > NOV_BED_LDS;            // (workgroup-uniform)
    const uint32_t head = text_head(b0);
    const int64_t i = i0 + threadIdx.x;
    if (i < i1 && first + i < (int64_t)in.n) {
        const uint32_t o = off[i], l = off[i + 1] - o, q = (uint32_t)(first + i);
        if (l != nov_bed_len(in, q) || l == 0u) atomicAdd(word + NOVC_OUTSIDE, 1u);      // (the row is not written: its bytes would leave their place)
        else if (direct) (void)nov_bed_line(text + o, in, q);
        else (void)nov_bed_line(text_image(s_img, head) + (o - b0), in, q);
    }
    if (direct) { if (threadIdx.x == 0) atomicAdd(word + NOVC_DIRECT, 1u); return; }
    __syncthreads();
    text_stream_out<NOV_BED_TILE>(s_img, b0, bytes, text);
}

}  // namespace l2r
