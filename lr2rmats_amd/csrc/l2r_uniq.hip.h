// l2r_uniq.hip.h -- the kernels of l2r_uniq_merge (`unique-gtf`, include/lr2rmats_hip.h): merge_trans over a list of transcripts whose
// (tid, start) does not descend, exact to the host loop.  The rule and the argument why clusters are independent: l2r_uniqplan.hip.h.
//
//   k_uniq_heads     one thread per transcript: start, end, exon count and strand into one packed record; a flag where (tid, start)
//                    falls below the predecessor's (the route test); the maximum of the tile's end keys (tid + 1) << 32 | end
//   k_uniq_pmax      one workgroup: the exclusive prefix maximum over the tile maxima, in place
//   k_uniq_cut       per tile the exclusive prefix maximum of the end keys behind the tile's prefix: transcript i heads a cluster where
//                    (tid + 1) << 32 | start exceeds it (and where i = 0)
//   (k_scan_u32 over the head flags numbers the clusters)
//   k_uniq_firsts    the first transcript of every cluster, n behind the last
//   k_uniq_merge     one wave per cluster, UNIQ_WAVES waves per workgroup.  The wave takes the cluster's offers in input order.  For one
//                    offer its lanes judge the cluster's list entries newest first, 64 per round: lane l the entry l behind the newest
//                    of the round; a ballot of the verdicts other than skip and its lowest lane give the deciding entry.  Stop, or no
//                    entry left, pushes the offer; a hit lets that one lane apply the mutation.  An entry is four words -- the offer that
//                    created it, first start, last end, coverage -- at cluster_first + k of arrays of n words (a cluster of m offers
//                    holds at most m entries: no arena).  Its chain is read from the input exon arrays, first start and last end from
//                    the mutable words
//   (k_scan_u32 over the clusters' list lengths: the rank of every cluster's first entry and the number of entries)
//   k_uniq_take      cluster order, then push order, is the host's list order: entries gathered into it, uniq_of made global
//
// Ordering inside k_uniq_merge.  An entry's words are written by one lane (the push by lane 0, a mutation by the deciding lane) and read
// by other lanes of the SAME wave in a later round; no other wave ever touches them.  The words are accessed with relaxed atomics of
// wavefront scope (plain global loads and stores), with a release fence of wavefront scope behind the writes of a round and an acquire
// fence of wavefront scope in front of the reads of the next.  That suffices: a wave's vector memory instructions are issued and
// performed in program order, so inside one wave nothing but the compiler could reorder or keep a word in a register -- the fences of
// wavefront scope forbid exactly that and cost no instruction.  No LDS copy, so a cluster's list has no size limit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l2r_kernels.hip.h"
#define L2R_UNIQ_KERNELS 1
#include "l2r_uniqplan.hip.h"

namespace l2r {

constexpr int UNIQ_TILE = L2R_UNIQ_PMAX_TILE;           // transcripts, and threads, of one tile of the prefix maximum
constexpr int UNIQ_WAVES = 4;                           // clusters of one workgroup of k_uniq_merge
static_assert(UNIQ_TILE == 256, "k_uniq_heads / k_uniq_cut: four waves per tile");

// words of the counter block
enum { UQW_UNSORTED = 0, UQW_CLUSTERS, UQW_UNIQUE, UQW_LARGEST, UQW_IDENT, UQW_CONTAINED, UQW_SINGLE, UQW_END_EXT, UQW_N };

struct UniqIn { int64_t n; const int32_t *tid; const uint8_t *rev; const int64_t *ex_off; const int32_t *xs, *xe; };
struct UniqRec { int32_t start, end; uint32_t n_rev; };  // n_rev: exon count, strand in bit 31

__device__ __forceinline__ uint64_t uniq_shfl_up64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t uniq_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// inclusive prefix maximum over the wave
__device__ __forceinline__ uint64_t uniq_wave_pmax(uint64_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t o = uniq_shfl_up64(v, d); if (lane >= d) v = uniq_max64(v, o); }
    return v;
}
// EXCLUSIVE prefix maximum over the workgroup's threads (blockDim.x / 64 waves, at most 16; 0 in front of the first); total: the
// workgroup's maximum.  Every thread of the workgroup calls it.
__device__ __forceinline__ uint64_t uniq_block_pmax(uint64_t v, uint64_t *s_wave, uint64_t &total)
{
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    const uint64_t inc = uniq_wave_pmax(v, lane);
    const uint64_t up = uniq_shfl_up64(inc, 1);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (int k = 0; k < nw; ++k) { const uint64_t m = s_wave[k]; if (k < w) before = uniq_max64(before, m); total = uniq_max64(total, m); }
    __syncthreads();
    return lane ? uniq_max64(up, before) : before;
}

__global__ __launch_bounds__(UNIQ_TILE)
void k_uniq_heads(UniqIn in, UniqRec *__restrict__ rec, uint64_t *__restrict__ tile_max, uint32_t *__restrict__ word)
{
    __shared__ uint64_t s_wave[UNIQ_TILE / 64];
    const int64_t i = (int64_t)blockIdx.x * UNIQ_TILE + threadIdx.x;
    uint64_t key_end = 0;
    if (i < in.n) {
        const int64_t o0 = in.ex_off[i], o1 = in.ex_off[i + 1];
        const int32_t tid = in.tid[i], start = in.xs[o0], end = in.xe[o1 - 1];
        rec[i] = UniqRec{start, end, (uint32_t)(o1 - o0) | (in.rev[i] ? 0x80000000u : 0u)};
        key_end = uniq_key(tid, end);
        if (i > 0 && uniq_key(tid, start) < uniq_key(in.tid[i - 1], in.xs[in.ex_off[i - 1]])) word[UQW_UNSORTED] = 1u;
    }
    uint64_t total;
    (void)uniq_block_pmax(key_end, s_wave, total);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = total;
}

// tile_max[0, n_tiles) <- its exclusive prefix maximum: one workgroup, 1024 tiles a round
__global__ __launch_bounds__(1024)
void k_uniq_pmax(uint64_t *__restrict__ tile_max, int64_t n_tiles)
{
    __shared__ uint64_t s_wave[16];
    uint64_t carry = 0;                                  // (the same in every thread)
    for (int64_t base = 0; base < n_tiles; base += 1024) {
        const int64_t k = base + threadIdx.x;
        uint64_t total;
        const uint64_t ex = uniq_block_pmax(k < n_tiles ? tile_max[k] : 0, s_wave, total);
        if (k < n_tiles) tile_max[k] = uniq_max64(carry, ex);
        carry = uniq_max64(carry, total);
    }
}

// head[i] <- 1 where transcript i heads a cluster, else 0 (tile_pre: the tiles' exclusive prefix maxima)
__global__ __launch_bounds__(UNIQ_TILE)
void k_uniq_cut(int64_t n, const int32_t *__restrict__ tid, const UniqRec *__restrict__ rec, const uint64_t *__restrict__ tile_pre, uint32_t *__restrict__ head)
{
    __shared__ uint64_t s_wave[UNIQ_TILE / 64];
    const int64_t i = (int64_t)blockIdx.x * UNIQ_TILE + threadIdx.x;
    uint64_t key_end = 0, key_start = 0;
    if (i < n) { const UniqRec r = rec[i]; const int32_t t = tid[i]; key_end = uniq_key(t, r.end); key_start = uniq_key(t, r.start); }
    uint64_t total;
    const uint64_t reach = uniq_max64(tile_pre[blockIdx.x], uniq_block_pmax(key_end, s_wave, total));
    if (i < n) head[i] = (i == 0 || key_start > reach) ? 1u : 0u;
}

// before: the exclusive scan of the head flags (n + 1 words).  first[c] <- the first transcript of cluster c, first[clusters] <- n.
__global__ __launch_bounds__(256)
void k_uniq_firsts(int64_t n, const uint32_t *__restrict__ before, uint32_t *__restrict__ first)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = before[i], a = before[i + 1];
    if (a != b) first[b] = (uint32_t)i;
    if (i == n - 1) first[a] = (uint32_t)n;
}

struct UniqList { int32_t *src, *start, *end, *cov; };   // n words each: cluster c's entries from first[c] on, in push order

__device__ __forceinline__ int32_t uniq_ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void uniq_st(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

__device__ __forceinline__ UniqChain uniq_chain_of(const UniqIn &in, const UniqRec &r, int64_t i)
{
    const int64_t off = in.ex_off[i];
    return UniqChain{in.xs + off, in.xe + off, (int32_t)(r.n_rev & 0x7fffffffu), r.start, r.end, in.tid[i], r.n_rev >> 31};
}

// len[c] <- entries of cluster c's list; merged[i], and uniq_of[i] = the entry of offer i counted inside its cluster
__global__ __launch_bounds__(UNIQ_WAVES * 64)
void k_uniq_merge(UniqIn in, const UniqRec *__restrict__ rec, const uint32_t *__restrict__ first, uint32_t n_clusters, UniqPrm p,
                  UniqList L, uint32_t *__restrict__ len, uint8_t *__restrict__ merged, int32_t *__restrict__ uniq_of, uint32_t *__restrict__ word)
{
    const uint32_t c = blockIdx.x * (uint32_t)UNIQ_WAVES + (threadIdx.x >> 6);
    if (c >= n_clusters) return;                       // (the whole wave)
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t f0 = first[c], f1 = first[c + 1];
    int64_t n_list = 0;
    uint32_t hits_i = 0, hits_c = 0, hits_s = 0, ext = 0;   // of this lane
    for (int64_t i = f0; i < f1; ++i) {
        const UniqChain t = uniq_chain_of(in, rec[i], i);
        int verdict = UNIQ_STOP;
        int64_t hit = -1;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int64_t top = n_list; top > 0; top -= 64) {
            const int64_t k = top - 1 - lane;
            int v = UNIQ_SKIP;
            UniqChain T = t;
            int32_t cov = 0;
            if (k >= 0) {
                const int64_t src = uniq_ld(L.src + f0 + k);
                T = uniq_chain_of(in, rec[src], src);
                T.first = uniq_ld(L.start + f0 + k); T.last = uniq_ld(L.end + f0 + k); cov = uniq_ld(L.cov + f0 + k);
                v = uniq_judge(t, T, p);
            }
            const unsigned long long m = __ballot(v != UNIQ_SKIP);
            if (m) {
                const int d = __ffsll((long long)m) - 1;
                verdict = __shfl(v, d, 64);
                hit = top - 1 - d;
                if (lane == d && verdict != UNIQ_STOP) {
                    int32_t s = T.first, e = T.last;
                    ext += (uint32_t)uniq_apply(verdict, t, s, e, cov);
                    if (verdict != UNIQ_CONTAINED) { uniq_st(L.start + f0 + k, s); uniq_st(L.end + f0 + k, e); uniq_st(L.cov + f0 + k, cov); }
                    hits_i += verdict == UNIQ_IDENT; hits_c += verdict == UNIQ_CONTAINED; hits_s += verdict == UNIQ_SINGLE;
                }
                break;
            }
        }
        const bool push = hit < 0 || verdict == UNIQ_STOP;
        if (lane == 0) {
            if (push) { uniq_st(L.src + f0 + n_list, (int32_t)i); uniq_st(L.start + f0 + n_list, t.first); uniq_st(L.end + f0 + n_list, t.last); uniq_st(L.cov + f0 + n_list, 1); }
            merged[i] = push ? 0 : 1;
            uniq_of[i] = (int32_t)(push ? n_list : hit);
        }
        if (push) ++n_list;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
    hits_i = wave_sum(hits_i); hits_c = wave_sum(hits_c); hits_s = wave_sum(hits_s); ext = wave_sum(ext);
    if (lane == 0) {
        len[c] = (uint32_t)n_list;
        atomicMax(word + UQW_LARGEST, (uint32_t)(f1 - f0));
        if (hits_i) atomicAdd(word + UQW_IDENT, hits_i);
        if (hits_c) atomicAdd(word + UQW_CONTAINED, hits_c);
        if (hits_s) atomicAdd(word + UQW_SINGLE, hits_s);
        if (ext) atomicAdd(word + UQW_END_EXT, ext);
    }
}

// before: the scan of the head flags; base: the exclusive scan of len (n_clusters + 1 words).  uniq_of made global, the entries gathered
// into list order.
__global__ __launch_bounds__(256)
void k_uniq_take(int64_t n, const uint32_t *__restrict__ before, const uint32_t *__restrict__ first, const uint32_t *__restrict__ base, UniqList L,
                 int32_t *__restrict__ uniq_of, int32_t *__restrict__ u_src, int32_t *__restrict__ u_start, int32_t *__restrict__ u_end, int32_t *__restrict__ u_cov)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t c = before[j + 1] - 1u, b = base[c], k = (uint32_t)j - first[c];
    uniq_of[j] += (int32_t)b;
    if (k < base[c + 1] - b) {
        const uint32_t r = b + k;
        u_src[r] = L.src[j]; u_start[r] = L.start[j]; u_end[r] = L.end[j]; u_cov[r] = L.cov[j];
    }
}

}  // namespace l2r
