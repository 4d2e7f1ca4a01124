// l2r_summary.hip.h -- the kernels of l2r_summary_finish (`update-gtf -y`, include/lr2rmats_hip.h): the reads accumulated in HBM put in
// class-major order with the merge key tid' = class << 29 | tid, so that the kernels of l2r_uniq.hip.h merge the four classes' lists as
// one.  The rule and why one list gives the verdicts of four: l2r_summaryplan.hip.h.
//
//   k_sum_class      one thread per read: class and exon count; per tile of 256 reads the four read counts, class-major
//                    (cnt[class * n_tiles + tile]), so that ONE exclusive scan over them gives the rank of every tile's first read of
//                    every class; the smallest read with a tid outside [0, 2^29) or without an exon
//   (k_scan_u32 over the exon counts: where every read's chain lies in the accumulated exon arrays; over the tile counts)
//   k_sum_place      the rank of every read: the tile's base of its class + the reads of its class in front of it in the tile (ballots
//                    inside the wave, the waves in front through LDS) -- input order inside a class, the partition is stable.  At the
//                    rank: tid', strand, exon count, the read itself
//   (k_scan_u32 over the exon counts in rank order: the compact place of every chain)
//   k_sum_gather     the chains copied to their compact place, the offsets widened to what UniqIn takes; the smallest read with a
//                    negative coordinate.  Thread form: one thread per read.  Wave form: one wave per read, lanes over exons, coalesced
//   (k_uniq_heads .. k_uniq_take of l2r_uniq.hip.h, unchanged, over the permuted columns)
//   k_sum_count      per class the reads and the offers that were pushed: ballots, one atomic per wave and class
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l2r_kernels.hip.h"
#include "l2r_summaryplan.hip.h"

namespace l2r {

constexpr int SUM_TILE = 256;                           // reads, and threads, of one tile of the partition
static_assert(SUM_TILE == 4 * WAVE, "k_sum_class / k_sum_place: four waves per tile");

// words of the counter block: the reads of every class, its pushed offers, the scans' totals
enum { SUMW_READS = 0, SUMW_UNIQUE = 4, SUMW_EXONS = 8, SUMW_TILES, SUMW_PLACED, SUMW_N };

__device__ __forceinline__ void sum_flag(unsigned long long *bad, int64_t read, int kind)
{
    atomicMin(bad, (unsigned long long)read << 4 | (unsigned long long)kind);
}

// cls[i], nex[i]; cnt[class * n_tiles + tile]
__global__ __launch_bounds__(SUM_TILE)
void k_sum_class(int64_t n, const int32_t *__restrict__ tid, const uint32_t *__restrict__ info, uint8_t *__restrict__ cls, uint32_t *__restrict__ nex,
                 uint32_t *__restrict__ cnt, int64_t n_tiles, unsigned long long *__restrict__ bad)
{
    __shared__ uint32_t s_cnt[SUM_TILE / WAVE][SUM_CLASSES];
    const int64_t i = (int64_t)blockIdx.x * SUM_TILE + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1)), w = (int)(threadIdx.x >> 6);
    int c = -1;
    if (i < n) {
        const uint32_t f = info[i];
        c = summary_class(f);
        cls[i] = (uint8_t)c; nex[i] = L2R_INFO_NEXON(f);
        if (!summary_tid_ok(tid[i])) sum_flag(bad, i, SUM_E_TID);
        else if (L2R_INFO_NEXON(f) == 0) sum_flag(bad, i, SUM_E_NO_EXON);
    }
#pragma unroll
    for (int k = 0; k < SUM_CLASSES; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (lane == 0) s_cnt[w][k] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < SUM_CLASSES) {
        uint32_t s = 0;
        for (int q = 0; q < SUM_TILE / WAVE; ++q) s += s_cnt[q][threadIdx.x];
        cnt[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = s;
    }
}

// base: the exclusive scan of cnt.  At the rank of read i: key, rev, nex (n + 1 words: scanned next), src
__global__ __launch_bounds__(SUM_TILE)
void k_sum_place(int64_t n, const int32_t *__restrict__ tid, const uint32_t *__restrict__ info, const uint8_t *__restrict__ cls, const uint32_t *__restrict__ base, int64_t n_tiles,
                 int32_t *__restrict__ key, uint8_t *__restrict__ rev, uint32_t *__restrict__ nex, uint32_t *__restrict__ src)
{
    __shared__ uint32_t s_cnt[SUM_TILE / WAVE][SUM_CLASSES];
    const int64_t i = (int64_t)blockIdx.x * SUM_TILE + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1)), w = (int)(threadIdx.x >> 6);
    const int c = i < n ? (int)cls[i] : -1;
    uint32_t before = 0;                                // reads of my class in front of me in my wave
#pragma unroll
    for (int k = 0; k < SUM_CLASSES; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (lane == 0) s_cnt[w][k] = (uint32_t)__popcll(m);
        if (c == k) before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (i >= n) return;
    for (int q = 0; q < w; ++q) before += s_cnt[q][c];
    const uint32_t r = base[(int64_t)c * n_tiles + blockIdx.x] + before;
    if ((int64_t)r >= n) return;                        // (cannot be: the counts add up to n)
    const uint32_t f = info[i];
    key[r] = summary_key(c, tid[i]); rev[r] = (f & L2R_INFO_REV) ? 1 : 0; nex[r] = L2R_INFO_NEXON(f); src[r] = (uint32_t)i;
}

struct SumGather {
    int64_t n;
    const uint32_t *src, *src_off, *dst_off;            // the read at rank r; its chain's place in the accumulated arrays (by read); the compact place (by rank, n + 1)
    const int32_t *xs, *xe;                             // accumulated, src_exons of them
    uint32_t src_exons;
    int64_t *ex_off; int32_t *out_s, *out_e;            // n + 1; the compact chains
    unsigned long long *bad;
};

template <bool BY_WAVE>
__global__ __launch_bounds__(256)
void k_sum_gather(SumGather g)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = BY_WAVE ? t >> 6 : t;
    if (r >= g.n) return;                               // (BY_WAVE: the whole wave)
    const int lane = BY_WAVE ? (int)(threadIdx.x & (WAVE - 1)) : 0;
    const uint32_t i = g.src[r], d0 = g.dst_off[r], d1 = g.dst_off[r + 1], k = d1 - d0;
    if ((int64_t)i >= g.n) return;                      // (cannot be: every rank has its read)
    const uint32_t s0 = g.src_off[i];
    if (lane == 0) { g.ex_off[r] = (int64_t)d0; if (r == g.n - 1) g.ex_off[g.n] = (int64_t)d1; }
    if ((uint64_t)s0 + k > (uint64_t)g.src_exons) return;       // (cannot be: the caller has compared the scans' totals)
    int32_t sign = 0;
    for (uint32_t j = (uint32_t)lane; j < k; j += BY_WAVE ? WAVE : 1) {
        const int32_t s = g.xs[s0 + j], e = g.xe[s0 + j];
        g.out_s[d0 + j] = s; g.out_e[d0 + j] = e;
        sign |= s | e;
    }
    if (sign < 0) sum_flag(g.bad, (int64_t)i, SUM_E_NEGATIVE);
}

// word[SUMW_READS + c] += the reads of class c, word[SUMW_UNIQUE + c] += those of them with merged == 0
__global__ __launch_bounds__(256)
void k_sum_count(int64_t n, const int32_t *__restrict__ key, const uint8_t *__restrict__ merged, uint32_t *__restrict__ word)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & (WAVE - 1));
    int c = -1; bool pushed = false;
    if (r < n) { c = (int)((uint32_t)key[r] >> SUM_TID_BITS); pushed = merged[r] == 0; }
#pragma unroll
    for (int k = 0; k < SUM_CLASSES; ++k) {
        const uint32_t reads = (uint32_t)__popcll(__ballot(c == k)), uniq = (uint32_t)__popcll(__ballot(c == k && pushed));
        if (lane == 0 && reads) atomicAdd(word + SUMW_READS + k, reads);
        if (lane == 0 && uniq) atomicAdd(word + SUMW_UNIQUE + k, uniq);
    }
}

}  // namespace l2r
