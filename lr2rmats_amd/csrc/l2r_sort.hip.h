// l2r_sort.hip.h -- `sort` and `filter -S`: the coordinate order of alignment records, as a permutation.
//
// One 64-bit key per record, the comparison `samtools sort` makes by coordinate:
//     key = (tid < 0 ? 0x7fffffff : tid) << 33 | (uint32)(pos + 1) << 1 | (flag >> 4 & 1)
// (records without a reference last; pos = -1 gives 0; the reverse strand behind the forward one at one position).  Equal keys keep
// their input order: LSD radix with 8-bit digits, every pass stable.  The payload is the 32-bit record index; the record bytes never
// come to the device.
//
// The kernels are those of l2r_radix.hip.h; this header says what they sort:
//   SortKeyOf              k_radix_keys<SortKeyOf>: the key of a record from its three columns
//   SortRows<FIRST, LAST>  k_radix_digit_hist<SortRows<false, false>> and the four k_radix_scatter<SortRows<FIRST, LAST>>: a row is
//                          {key, index}.  FIRST: the index is the row number, no index column is read; LAST: only the index column is
//                          written
//
// HBM-bound integer work: a scatter reads and writes 12 bytes per row (8 without an index column on one side, 4 without a key column
// on the other), the digit histogram reads 8.
#pragma once
#include "l2r_radix.hip.h"

namespace l2r {

constexpr int SORT_THREADS = RADIX_THREADS;
constexpr int SORT_KEY_BYTES = RADIX_KEY_BYTES;

__device__ __forceinline__ uint64_t sort_key(int32_t tid, int32_t pos, uint32_t flag)
{
    const uint64_t t = tid < 0 ? 0x7fffffffull : (uint64_t)(uint32_t)tid;
    return (t << 33) | ((uint64_t)((uint32_t)pos + 1u) << 1) | (uint64_t)((flag >> 4) & 1u);
}

struct SortKeyOf {
    const uint16_t *flag; const int32_t *tid, *pos;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return sort_key(tid[i], pos[i], flag[i]); }
};

template <bool FIRST, bool LAST>
struct SortRows {
    const uint64_t *__restrict__ key_in; const uint32_t *__restrict__ idx_in; uint64_t *__restrict__ key_out; uint32_t *__restrict__ idx_out;
    struct Row { uint64_t k; uint32_t x; };
    static constexpr int HIST_UNROLL = 4;
    __device__ __forceinline__ Row blank(uint32_t i) const { return Row{0, i}; }
    __device__ __forceinline__ Row load(uint32_t i) const { Row r{key_in[i], i}; if constexpr (!FIRST) r.x = idx_in[i]; return r; }
    __device__ __forceinline__ uint32_t digit(const Row &r, int b) const { return (uint32_t)(r.k >> (8 * b)) & 0xffu; }
    __device__ __forceinline__ uint32_t digit_at(uint32_t i, int b) const { return (uint32_t)(key_in[i] >> (8 * b)) & 0xffu; }
    __device__ __forceinline__ void store(uint32_t o, const Row &r) const { if constexpr (!LAST) key_out[o] = r.k; idx_out[o] = r.x; }
};

}  // namespace l2r
