// l2r_radix.hip.h -- one pass of a stable LSD radix sort with 8-bit digits, written once: `sort` / `filter -S` (l2r_sort.hip.h) and
// `bam2sj` / `sjtab` (l2r_sj.hip.h) say what a row is and where a digit comes from, the kernels here do the rest.
//
//   k_radix_keys<KeyOf>       one thread per row: its 64-bit key; the histograms of all eight key bytes (a byte that is equal in every key
//                             is a pass that is not run); one word that says whether any key is below its predecessor (none: the rows are
//                             in order and no pass runs at all)
//   k_radix_digit_hist<Rows>  per pass: the digit histogram of every tile of RADIX_TILE rows, digit-major (one k_scan_u32 over it gives
//                             every (digit, tile) its first slot)
//   k_radix_scatter<Rows>     per pass: stable scatter, one workgroup per tile, 256 rows per round in row order: the rank of a row among the
//                             rows of its digit = rows of earlier rounds + rows of earlier waves + lanes in front of it
//
// KeyOf, passed by value, holds the input columns:   uint64_t key(int64_t i)
// Rows, passed by value, holds the columns of both sides of a pass:
//     Row                       what a lane carries from load to store
//     Row blank(uint32_t i)     the row of a lane behind the last row
//     Row load(uint32_t i)
//     uint32_t digit(const Row &, int b)
//     uint32_t digit_at(uint32_t i, int b)      the digit alone, from the one column byte b lives in (the histogram)
//     void store(uint32_t o, const Row &)
//     HIST_UNROLL               rounds of a tile the histogram issues together
// The host side is in l2r_engine.hip: radix_passes is the pass loop (digit hist -> scan -> scatter over the bytes it is given), and
// order_by_keys is k_radix_keys and the passes over SortRows that follow it (sort_passes: which bytes run), for every command that wants
// rows in the order of 64-bit keys.  No kernel waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l2r {

constexpr int RADIX_THREADS = 256;
constexpr int RADIX_TILE = 4096;                         // rows of one workgroup of a pass
constexpr int RADIX_ROUNDS = RADIX_TILE / RADIX_THREADS;
constexpr int RADIX_KEY_BYTES = 8;                       // of a k_radix_keys key
static_assert(RADIX_TILE % RADIX_THREADS == 0, "a tile is a whole number of rounds");
static_assert(L2R_SORT_TILE == RADIX_TILE && L2R_SJ_SORT_TILE == RADIX_TILE, "include/lr2rmats_hip.h names the tile of a pass");

// hist: 8 x 256 words and *descends, cleared by the caller.  A wave whose 64 keys share a byte -- the upper bytes of nearly every
// wave of coordinate-sorted input -- adds 64 to one word instead of 64 times 1.
template <typename KeyOf>
__global__ __launch_bounds__(RADIX_THREADS)
void k_radix_keys(KeyOf in, int64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ hist, uint32_t *__restrict__ descends)
{
    __shared__ uint32_t s_h[RADIX_KEY_BYTES * 256];
    for (int k = threadIdx.x; k < RADIX_KEY_BYTES * 256; k += RADIX_THREADS) s_h[k] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    bool down = false;
    for (int64_t base = (int64_t)blockIdx.x * RADIX_THREADS; base < n; base += (int64_t)gridDim.x * RADIX_THREADS) {      // (uniform)
        const int64_t i = base + threadIdx.x;
        const bool active = i < n;
        uint64_t k = 0;
        if (active) { k = in.key(i); key[i] = k; }
        uint64_t prev = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
        if (lane == 0 && active && i > 0) prev = in.key(i - 1);
        down |= active && i > 0 && k < prev;
        const bool whole = __ballot(active) == ~0ull;
#pragma unroll
        for (int b = 0; b < RADIX_KEY_BYTES; ++b) {
            const uint32_t d = (uint32_t)(k >> (8 * b)) & 0xffu;
            if (whole && __all(d == (uint32_t)__builtin_amdgcn_readfirstlane((int)d))) { if (lane == 0) atomicAdd(&s_h[b * 256 + d], 64u); }
            else if (active) atomicAdd(&s_h[b * 256 + d], 1u);
        }
    }
    if (__any(down) && lane == 0) atomicOr(descends, 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < RADIX_KEY_BYTES * 256; k += RADIX_THREADS) { const uint32_t v = s_h[k]; if (v) atomicAdd(&hist[k], v); }
}

// tile_hist[d * n_tiles + tile] = rows of the tile whose byte b is d
template <typename Rows>
__global__ __launch_bounds__(RADIX_THREADS)
void k_radix_digit_hist(Rows rows, uint32_t n, int b, uint32_t n_tiles, uint32_t *__restrict__ tile_hist)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t t0 = blockIdx.x * (uint32_t)RADIX_TILE;
#pragma unroll Rows::HIST_UNROLL
    for (int r = 0; r < RADIX_ROUNDS; ++r) {
        const uint32_t i = t0 + (uint32_t)r * RADIX_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&s_h[rows.digit_at(i, b)], 1u);
    }
    __syncthreads();
    tile_hist[threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

// The lanes of this wave that are active and hold the digit of the calling lane: eight ballots, one per digit bit.
__device__ __forceinline__ unsigned long long radix_same_digit(uint32_t dg, bool active)
{
    unsigned long long same = __ballot(active);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool bit = (dg >> q) & 1u;
        const unsigned long long bal = __ballot(active && bit);
        same &= bit ? bal : ~bal;
    }
    return same;
}

// first[]: tile_hist after its exclusive scan: the first slot of the tile's rows of every digit
template <typename Rows>
__global__ __launch_bounds__(RADIX_THREADS)
void k_radix_scatter(Rows rows, uint32_t n, int b, uint32_t n_tiles, const uint32_t *__restrict__ first)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wcnt[RADIX_THREADS / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s_base[threadIdx.x] = first[threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < RADIX_THREADS / 64; ++k) s_wcnt[k][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t t0 = blockIdx.x * (uint32_t)RADIX_TILE;
    for (int r = 0; r < RADIX_ROUNDS; ++r) {
        const uint32_t r0 = t0 + (uint32_t)r * RADIX_THREADS;
        if (r0 >= n) break;                                            // (uniform)
        const uint32_t i = r0 + threadIdx.x;
        const bool active = i < n;
        typename Rows::Row row = rows.blank(i);
        if (active) row = rows.load(i);
        const uint32_t dg = rows.digit(row, b);
        const unsigned long long same = radix_same_digit(dg, active);
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (active && rank == 0u) s_wcnt[w][dg] = (uint32_t)__popcll(same);
        __syncthreads();
        if (active) {
            uint32_t o = s_base[dg] + rank;
            for (int q = 0; q < w; ++q) o += s_wcnt[q][dg];
            if (o < n) rows.store(o, row);
        }
        __syncthreads();
        {
            uint32_t s = 0;
#pragma unroll
            for (int q = 0; q < RADIX_THREADS / 64; ++q) { s += s_wcnt[q][threadIdx.x]; s_wcnt[q][threadIdx.x] = 0u; }
            s_base[threadIdx.x] += s;
        }
        __syncthreads();
    }
}

}  // namespace l2r
