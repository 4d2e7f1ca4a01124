// l2r_names.hip.h -- `sort -n`, `filter -N`, `fusion -N`: the name order of alignment records, as a permutation (gfx950).
//
// The order (include/lr2rmats_hip.h): records with one name are consecutive, the groups follow each other by the input index of their
// first record, the records of a group keep their input order; input that is grouped already gives the identity.  That is the whole
// definition: no equality with the output of any samtools release is claimed.  The names come as one packed byte blob and n + 1 offsets;
// the record bytes never come to the device.
//
//   NameHashOf      k_radix_keys<NameHashOf> (l2r_radix.hip.h): a seeded 64-bit hash of a record's name bytes and length, one thread per
//                   record; the kernel also leaves the byte histograms and the descent word, and the passes are those of `sort`
//                   (sort_passes, SortRows) over the hashes, with the record index as the payload
//   k_name_heads    over the rows in hash order: row k is a head iff k == 0, or its hash differs from row k - 1's, or its name does
//                   (length and bytes, through the index column); a pair with one hash and two names adds 1 to the mismatch word.
//                   The passes are stable, so a head carries the smallest input index of its run
//   k_name_firsts   behind the exclusive k_scan_u32 of the head flags (row k is of group before[k + 1] - 1): head_pos[g], first_idx[g]
//   k_name_sizes    group g's size into a zeroed n-word array at slot first_idx[g]; one exclusive k_scan_u32 over that array gives every
//                   group its base in the order of first appearance
//   k_name_place    order[base[first_idx[g]] + (k - head_pos[g])] = idx[k]; one word says whether any record moved
//
// With no mismatch the runs of one hash are exactly the groups: equal names give equal hashes, and a run whose neighbouring pairs are all
// equal holds one name.  With a mismatch the engine runs once more with a second seed and then orders on the host (l2r_nameorder.hip.h).
//
// Name bytes are read as ALIGNED 8-byte words, two of them shifted into one word of the name: a name starts at any byte, and neighbouring
// threads read neighbouring words of the blob.  The words that hold a name's first and last byte may reach in front of and behind it, so
// the blob starts on an 8-byte boundary and has 8 bytes of room behind its last name; what lies outside the name is masked away.
// No kernel waits for another workgroup.
#pragma once
#include "l2r_radix.hip.h"

namespace l2r {

constexpr int NAME_THREADS = RADIX_THREADS;
constexpr uint32_t NAME_MAX_LEN = L2R_NAME_MAX;             // include/lr2rmats_hip.h
constexpr size_t NAME_BLOB_ROOM = 16;                    // bytes behind the last name a load may touch (8), rounded up

// words: the blob, names[off0 ...] at its byte 0; off: the caller's n + 1 offsets
struct NameCols { const uint64_t *__restrict__ words; const int64_t *__restrict__ off; int64_t off0; };

// The 8-byte words of one name, little endian, the bytes behind the name zero: next() while left() > 0.
struct NameWords {
    const uint64_t *p, *end;
    uint64_t cur;
    uint32_t s, len, done;
    __device__ __forceinline__ NameWords(const NameCols &c, uint32_t i)
    {
        const int64_t o = c.off[i], b = o - c.off0;
        const int64_t l = c.off[(size_t)i + 1] - o;
        len = l < 0 ? 0u : l > (int64_t)NAME_MAX_LEN ? NAME_MAX_LEN : (uint32_t)l;      // (the engine has checked the offsets)
        done = 0u;
        s = 8u * (uint32_t)(b & 7);
        p = c.words + (b >> 3);
        end = c.words + ((b + (int64_t)len + 7) >> 3);
        cur = len ? *p : 0ull;
    }
    __device__ __forceinline__ bool left() const { return done < len; }
    __device__ __forceinline__ uint64_t next()
    {
        ++p;
        const uint64_t nxt = p < end ? *p : 0ull;
        uint64_t w = s ? (cur >> s) | (nxt << (64u - s)) : cur;
        const uint32_t rem = len - done;
        if (rem < 8u) w &= (1ull << (8u * rem)) - 1ull;
        cur = nxt; done += 8u;
        return w;
    }
};

__device__ __forceinline__ uint64_t name_mix(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h;
}

// The length goes in first, so a name and the same name with zero bytes behind it differ.
__device__ __forceinline__ uint64_t name_hash(const NameCols &c, uint32_t i, uint64_t seed)
{
    NameWords w(c, i);
    uint64_t h = seed ^ ((uint64_t)(w.len + 1u) * 0x9e3779b97f4a7c15ull);
    while (w.left()) { h = (h ^ w.next()) * 0x9fb21c651e98df25ull; h ^= h >> 29; }
    return name_mix(h);
}

__device__ __forceinline__ bool name_equal(const NameCols &c, uint32_t a, uint32_t b)
{
    NameWords x(c, a), y(c, b);
    if (x.len != y.len) return false;
    while (x.left()) if (x.next() != y.next()) return false;
    return true;
}

// mask: L2R_NAME_HASH_BITS (tests) keeps the low bits only
struct NameHashOf {
    NameCols c; uint64_t seed, mask;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return name_hash(c, (uint32_t)i, seed) & mask; }
};

// hkey: the hashes in RECORD order; idx: the index column the passes left (null: no pass ran, row k is record k).  head has n words.
__global__ __launch_bounds__(NAME_THREADS)
void k_name_heads(NameCols c, const uint64_t *__restrict__ hkey, const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ head, uint32_t *__restrict__ mismatch)
{
    const uint32_t k = blockIdx.x * NAME_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = k < n;
    uint32_t r = 0; uint64_t h = 0;
    if (active) { r = idx ? idx[k] : k; if (r >= n) r = n - 1u; h = hkey[r]; }
    uint64_t ph = (uint64_t)__shfl_up((unsigned long long)h, 1, 64);
    uint32_t pr = (uint32_t)__shfl_up((int)r, 1, 64);
    if (lane == 0 && active && k > 0u) { pr = idx ? idx[k - 1u] : k - 1u; if (pr >= n) pr = n - 1u; ph = hkey[pr]; }
    bool is_head = true, mis = false;
    if (active && k > 0u && ph == h) { mis = !name_equal(c, pr, r); is_head = mis; }
    if (active) head[k] = is_head ? 1u : 0u;
    const unsigned long long m = __ballot(mis);
    if (m && lane == 0) atomicAdd(mismatch, (uint32_t)__popcll(m));
}

// before: head[] after its exclusive scan, n + 1 words (before[n] = groups).  head_pos has n + 1 words: head_pos[groups] = n.
__global__ __launch_bounds__(NAME_THREADS)
void k_name_firsts(const uint32_t *__restrict__ before, const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ head_pos, uint32_t *__restrict__ first_idx)
{
    const uint32_t k = blockIdx.x * NAME_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint32_t g = before[k];
    if (g != before[k + 1u] && g < n) { head_pos[g] = k; first_idx[g] = idx ? idx[k] : k; }
    if (k == 0u) { const uint32_t G = before[n]; if (G <= n) head_pos[G] = n; }
}

// sizes: n words, cleared by the caller
__global__ __launch_bounds__(NAME_THREADS)
void k_name_sizes(const uint32_t *__restrict__ before, const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ first_idx, uint32_t n, uint32_t *__restrict__ sizes)
{
    const uint32_t g = blockIdx.x * NAME_THREADS + threadIdx.x;
    const uint32_t G = before[n];
    if (g >= G || g >= n) return;
    const uint32_t f = first_idx[g];
    if (f < n) sizes[f] = head_pos[g + 1u] - head_pos[g];
}

// base: sizes[] after its exclusive scan.  *moved |= 1 where a record is not at its own index (the order is not the identity).
__global__ __launch_bounds__(NAME_THREADS)
void k_name_place(const uint32_t *__restrict__ before, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ first_idx,
                  const uint32_t *__restrict__ base, uint32_t n, uint32_t *__restrict__ order, uint32_t *__restrict__ moved)
{
    const uint32_t k = blockIdx.x * NAME_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool mv = false;
    if (k < n) {
        const uint32_t g = before[k + 1u] - 1u;
        if (g < n) {
            const uint32_t f = first_idx[g], x = idx ? idx[k] : k;
            if (f < n) {
                const uint32_t o = base[f] + (k - head_pos[g]);
                if (o < n) order[o] = x;
                mv = o != x;
            }
        }
    }
    if (__any(mv) && lane == 0) atomicOr(moved, 1u);
}

}  // namespace l2r
