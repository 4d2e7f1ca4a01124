// l2r_sort.hip.h -- the kernels of `sort` and `filter -S`: the coordinate order of alignment records, as a permutation.
//
// One 64-bit key per record, the comparison `samtools sort` makes by coordinate:
//     key = (tid < 0 ? 0x7fffffff : tid) << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
// (records without a reference last; pos = -1 gives 0; the reverse strand behind the forward one at one position).  Equal keys keep
// their input order: LSD radix with 8-bit digits, every pass stable.  The payload is the 32-bit record index; the record bytes never
// come to the device.
//
//   k_sort_keys        one thread per record: the key; the histograms of all eight key bytes (a byte that is equal in every key is a
//                      pass that is not run); one word that says whether any key is below its predecessor (none: the order is the
//                      identity and no pass runs at all)
//   k_sort_digit_hist  per pass: the digit histogram of every tile of SORT_TILE rows, digit-major (one k_scan_u32 over it gives every
//                      (digit, tile) its first slot)
//   k_sort_scatter     per pass: stable scatter, one workgroup per tile, 256 rows per round in row order: the rank of a row among the
//                      rows of its digit = rows of earlier rounds + rows of earlier waves + lanes in front of it.  FIRST: the index
//                      is the row number, no index column is read; LAST: only the index column is written
//
// HBM-bound integer work: a scatter reads and writes 12 bytes per row (8 without an index column on one side, 4 without a key column
// on the other), the digit histogram reads 8.  No kernel waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l2r {

constexpr int SORT_THREADS = 256;
constexpr int SORT_TILE = L2R_SORT_TILE;                // rows of one workgroup of a radix pass (include/lr2rmats_hip.h)
constexpr int SORT_ROUNDS = SORT_TILE / SORT_THREADS;
constexpr int SORT_KEY_BYTES = 8;
static_assert(SORT_TILE % SORT_THREADS == 0, "a tile is a whole number of rounds");

struct SortRecs { int64_t n; const uint16_t *flag; const int32_t *tid, *pos; };

__device__ __forceinline__ uint64_t sort_key(int32_t tid, int32_t pos, uint32_t flag)
{
    const uint64_t t = tid < 0 ? 0x7fffffffull : (uint64_t)(uint32_t)tid;
    return (t << 33) | ((uint64_t)((uint32_t)pos + 1u) << 1) | (uint64_t)((flag >> 4) & 1u);
}

// hist: 8 x 256 words and *descends, cleared by the caller.  A wave whose 64 keys share a byte -- the upper bytes of nearly every
// wave of coordinate-sorted input -- adds 64 to one word instead of 64 times 1.
__global__ __launch_bounds__(SORT_THREADS)
void k_sort_keys(SortRecs r, uint64_t *__restrict__ key, uint32_t *__restrict__ hist, uint32_t *__restrict__ descends)
{
    __shared__ uint32_t s_h[SORT_KEY_BYTES * 256];
    for (int k = threadIdx.x; k < SORT_KEY_BYTES * 256; k += SORT_THREADS) s_h[k] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    bool down = false;
    for (int64_t base = (int64_t)blockIdx.x * SORT_THREADS; base < r.n; base += (int64_t)gridDim.x * SORT_THREADS) {      // (uniform)
        const int64_t i = base + threadIdx.x;
        const bool active = i < r.n;
        uint64_t k = 0;
        if (active) { k = sort_key(r.tid[i], r.pos[i], r.flag[i]); key[i] = k; }
        uint64_t prev = (uint64_t)__shfl_up((unsigned long long)k, 1, 64);
        if (lane == 0 && active && i > 0) prev = sort_key(r.tid[i - 1], r.pos[i - 1], r.flag[i - 1]);
        down |= active && i > 0 && k < prev;
        const bool whole = __ballot(active) == ~0ull;
#pragma unroll
        for (int b = 0; b < SORT_KEY_BYTES; ++b) {
            const uint32_t d = (uint32_t)(k >> (8 * b)) & 0xffu;
            if (whole && __all(d == (uint32_t)__builtin_amdgcn_readfirstlane((int)d))) { if (lane == 0) atomicAdd(&s_h[b * 256 + d], 64u); }
            else if (active) atomicAdd(&s_h[b * 256 + d], 1u);
        }
    }
    if (__any(down) && lane == 0) atomicOr(descends, 1u);
    __syncthreads();
    for (int k = threadIdx.x; k < SORT_KEY_BYTES * 256; k += SORT_THREADS) { const uint32_t v = s_h[k]; if (v) atomicAdd(&hist[k], v); }
}

// tile_hist[d * n_tiles + tile] = rows of the tile whose byte b is d
__global__ __launch_bounds__(SORT_THREADS)
void k_sort_digit_hist(const uint64_t *__restrict__ key, uint32_t n, int b, uint32_t n_tiles, uint32_t *__restrict__ tile_hist)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t t0 = blockIdx.x * (uint32_t)SORT_TILE;
#pragma unroll 4
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const uint32_t i = t0 + (uint32_t)r * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(uint32_t)(key[i] >> (8 * b)) & 0xffu], 1u);
    }
    __syncthreads();
    tile_hist[threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

// The lanes of this wave that are active and hold the digit of the calling lane: eight ballots, one per digit bit.
__device__ __forceinline__ unsigned long long sort_same_digit(uint32_t dg, bool active)
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
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(SORT_THREADS)
void k_sort_scatter(const uint64_t *__restrict__ key_in, const uint32_t *__restrict__ idx_in, uint64_t *__restrict__ key_out,
                    uint32_t *__restrict__ idx_out, uint32_t n, int b, uint32_t n_tiles, const uint32_t *__restrict__ first)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wcnt[SORT_THREADS / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s_base[threadIdx.x] = first[threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < SORT_THREADS / 64; ++k) s_wcnt[k][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t t0 = blockIdx.x * (uint32_t)SORT_TILE;
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const uint32_t r0 = t0 + (uint32_t)r * SORT_THREADS;
        if (r0 >= n) break;                                            // (uniform)
        const uint32_t i = r0 + threadIdx.x;
        const bool active = i < n;
        uint64_t k = 0; uint32_t x = i;
        if (active) { k = key_in[i]; if constexpr (!FIRST) x = idx_in[i]; }
        const uint32_t dg = (uint32_t)(k >> (8 * b)) & 0xffu;
        const unsigned long long same = sort_same_digit(dg, active);
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (active && rank == 0u) s_wcnt[w][dg] = (uint32_t)__popcll(same);
        __syncthreads();
        if (active) {
            uint32_t o = s_base[dg] + rank;
            for (int q = 0; q < w; ++q) o += s_wcnt[q][dg];
            if (o < n) { if constexpr (!LAST) key_out[o] = k; idx_out[o] = x; }
        }
        __syncthreads();
        {
            uint32_t s = 0;
#pragma unroll
            for (int q = 0; q < SORT_THREADS / 64; ++q) { s += s_wcnt[q][threadIdx.x]; s_wcnt[q][threadIdx.x] = 0u; }
            s_base[threadIdx.x] += s;
        }
        __syncthreads();
    }
}

}  // namespace l2r
