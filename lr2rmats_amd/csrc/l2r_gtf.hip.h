// l2r_gtf.hip.h -- `sort-gtf`: the kept lines of concatenated GTF text in the order update-gtf wants, as rows (gfx950).
//
// The order is defined in include/lr2rmats_hip.h and restated in l2r_gtforder.hip.h.  The text is uploaded once and stays as bytes;
// what leaves the device is one row (start, length, line number) per kept line and the permutation.  Every offset is a 32-bit word
// (the engine sends texts of 2^32 - 64 bytes and more to the host routine).
//
//   k_gtf_count      one workgroup per tile of L2R_GTF_TILE bytes: its newlines; the NUL bytes of the whole text into one word
//   k_gtf_starts     behind the exclusive k_scan_u32 of the tiles' counts: start[j] for every line j.  The rank of a newline inside its
//                    wave's quarter of the tile comes from ballots and popcounts
//   k_gtf_fields     one thread per line: the comment test, the blank-separated fields 1 to 5, the kept flag and the transcript flag;
//                    for a transcript line field 1's (offset, length), start and end as uint32, and the domain check -- the smallest
//                    bad line number by one atomicMin per wave
//   k_gtf_rows       behind the exclusive scans of both flags: the row of every kept line with the index of the transcript whose key it
//                    carries, and the transcripts densely in line order.  The carry-forward is that scan
//   k_gtf_chr_heads  a transcript is a head iff it is the first or its field 1 differs from the previous transcript's (length, then bytes)
//   k_gtf_head_take  behind the scan of the head flags: the heads' (offset, length), densely; the host ranks them (l2r_gtforder.hip.h)
//   k_gtf_triples    every row's (c, s, e) through its transcript and that transcript's head; one word says whether any row's triple
//                    is below its predecessor's (none: the order is the identity and nothing else runs)
//   GtfEndKeyOf, GtfChrStartKeyOf    k_radix_keys of the two stable stages: e, then c << 32 | s read through the first stage's order
//   k_gtf_compose    order[k] = order1[perm2[k]]
//
// Text is read in the two line kernels as ALIGNED 16-byte words, neighbouring lanes neighbouring words: the allocation is 16-byte
// aligned and has GTF_TEXT_ROOM zeroed bytes behind the text; bytes behind the text are masked to a blank before they are counted.
// Every offset that comes out of a column is checked against its bound before it is used as an address.  No kernel waits for another
// workgroup.
#pragma once
#include "l2r_radix.hip.h"

namespace l2r {

constexpr int GTF_THREADS = RADIX_THREADS;
constexpr uint32_t GTF_TILE = L2R_GTF_TILE;              // bytes of text of one workgroup of the line kernels
constexpr uint32_t GTF_WAVE_BYTES = GTF_TILE / (GTF_THREADS / 64);       // a wave's contiguous quarter
constexpr int GTF_ROUNDS = (int)(GTF_WAVE_BYTES / (64 * 16));              // 16-byte loads per lane
constexpr size_t GTF_TEXT_ROOM = 16;
constexpr uint32_t GTF_NONE = 0xffffffffu;
static_assert(GTF_TILE % (GTF_THREADS * 16) == 0 && GTF_ROUNDS >= 1 && GTF_ROUNDS <= 8, "a tile is a whole number of 16-byte rounds of the workgroup");

// bit 7 of every byte of x that is zero, exactly (no carry crosses a byte)
__device__ __forceinline__ uint32_t gtf_zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
// bits 7, 15, 23, 31 -> bits 0..3
__device__ __forceinline__ uint32_t gtf_pack4(uint32_t m) { return ((m >> 7) * 0x01020408u) >> 24 & 0xfu; }

// The 16 bytes at the aligned offset `at` (< n), the bytes at n and behind it turned into spaces.
__device__ __forceinline__ uint4 gtf_load16(const uint4 *__restrict__ text, uint32_t at, uint32_t n)
{
    uint4 v = text[at >> 4];
    if (n - at < 16u) {                                  // the text's last, partial word
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = at + 4u * (uint32_t)k;
            const uint32_t valid = o >= n ? 0u : n - o >= 4u ? 4u : n - o;
            const uint32_t keep = valid >= 4u ? 0xffffffffu : (1u << (8u * valid)) - 1u;
            w[k] = (w[k] & keep) | (0x20202020u & ~keep);
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}
// bit k: byte k of the 16 equals c
__device__ __forceinline__ uint32_t gtf_mask16(const uint4 &v, uint32_t c4)
{
    return gtf_pack4(gtf_zero_bytes(v.x ^ c4)) | gtf_pack4(gtf_zero_bytes(v.y ^ c4)) << 4 | gtf_pack4(gtf_zero_bytes(v.z ^ c4)) << 8 | gtf_pack4(gtf_zero_bytes(v.w ^ c4)) << 12;
}

__device__ __forceinline__ uint32_t gtf_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// count: one word per tile (cleared by nobody: every tile writes its own).  *nul: cleared by the caller.
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_count(const uint4 *__restrict__ text, uint32_t n, uint32_t *__restrict__ count, uint32_t *__restrict__ nul)
{
    __shared__ uint32_t s_nl[GTF_THREADS / 64], s_z[GTF_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t0 = blockIdx.x * GTF_TILE + (uint32_t)w * GTF_WAVE_BYTES;    // (n < 2^32 - 64: no tile base wraps)
    uint32_t c_nl = 0, c_z = 0;
#pragma unroll
    for (int r = 0; r < GTF_ROUNDS; ++r) {
        const uint32_t at = t0 + (uint32_t)r * 1024u + 16u * (uint32_t)lane;
        if (at < n && at >= t0) {
            const uint4 v = gtf_load16(text, at, n);
            c_nl += (uint32_t)__popc(gtf_mask16(v, 0x0a0a0a0au));
            c_z += (uint32_t)__popc(gtf_mask16(v, 0u));
        }
    }
    c_nl = gtf_wave_sum(c_nl); c_z = gtf_wave_sum(c_z);
    if (lane == 0) { s_nl[w] = c_nl; s_z[w] = c_z; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, z = 0;
#pragma unroll
        for (int k = 0; k < GTF_THREADS / 64; ++k) { a += s_nl[k]; z += s_z[k]; }
        count[blockIdx.x] = a;
        if (z) atomicAdd(nul, z);
    }
}

// first: count[] after its exclusive scan.  start has n_lines + 1 words: start[0] = 0, start[j] = the byte behind newline j - 1, and
// where the text's last line has no newline start[n_lines] = n + 1, so that line j is [start[j], start[j + 1] - 1) for every j.
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_starts(const uint4 *__restrict__ text, uint32_t n, const uint32_t *__restrict__ first, uint32_t n_lines, uint32_t open_end, uint32_t *__restrict__ start)
{
    __shared__ uint32_t s_w[GTF_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t0 = blockIdx.x * GTF_TILE + (uint32_t)w * GTF_WAVE_BYTES;
    uint32_t m[GTF_ROUNDS], before[GTF_ROUNDS];          // the lane's newline bits of a round; newlines of the wave in front of them
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < GTF_ROUNDS; ++r) {
        const uint32_t at = t0 + (uint32_t)r * 1024u + 16u * (uint32_t)lane;
        m[r] = 0u;
        if (at < n && at >= t0) m[r] = gtf_mask16(gtf_load16(text, at, n), 0x0a0a0a0au);
        // newlines of the lanes in front of this one: the lane's count has five bits, one ballot per bit
        const uint32_t cnt = (uint32_t)__popc(m[r]);
        uint32_t mine = total;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned long long b = __ballot((cnt >> k) & 1u);
            mine += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)) << k;      // set bits below this lane
            total += (uint32_t)__popcll(b) << k;
        }
        before[r] = mine;
    }
    if (lane == 0) s_w[w] = total;
    __syncthreads();
    uint32_t base = first[blockIdx.x];
    for (int k = 0; k < w; ++k) base += s_w[k];
#pragma unroll
    for (int r = 0; r < GTF_ROUNDS; ++r) {
        const uint32_t at = t0 + (uint32_t)r * 1024u + 16u * (uint32_t)lane;
        uint32_t bits = m[r], k = base + before[r] + 1u;
        while (bits) {
            const uint32_t j = (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            if (k <= n_lines) start[k] = at + j + 1u;
            ++k;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { start[0] = 0u; if (open_end) start[n_lines] = n + 1u; }
}

// What the fields kernel leaves per line; name_off .. e only on transcript lines.
struct GtfLineCols { uint32_t *__restrict__ kept, *__restrict__ tx, *__restrict__ name_off, *__restrict__ name_len, *__restrict__ s, *__restrict__ e; };

// the decimal number [p, q): false where empty, not all digits or above 2^32 - 1
__device__ __forceinline__ bool gtf_number(const uint8_t *__restrict__ text, uint32_t p, uint32_t q, uint32_t *out)
{
    if (p >= q) return false;
    uint64_t v = 0;
    bool ok = true;
    for (; p < q && ok; ++p) {
        const uint32_t d = (uint32_t)text[p] - (uint32_t)'0';
        ok = d <= 9u;
        v = v * 10u + d;
        ok = ok && v <= 0xffffffffull;
    }
    *out = (uint32_t)v;
    return ok;
}

// kept / tx: 0 or 1 per line, n_lines + 1 words each (the scans put their totals behind them).  *bad_line: 0xffffffff from the caller.
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_fields(const uint8_t *__restrict__ text, uint32_t n, const uint32_t *__restrict__ start, uint32_t n_lines, GtfLineCols o, uint32_t *__restrict__ bad_line)
{
    const uint32_t j = blockIdx.x * GTF_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool bad = false;
    if (j < n_lines) {
        uint32_t b = start[j], e = start[j + 1u] - 1u;
        if (e > n) e = n;                                // (what k_gtf_starts wrote is within the text; a wrong word reads nothing outside it)
        if (b > e) b = e;
        bool kept = false, tx = false;
        if (b == e || text[b] != (uint8_t)'#') {
            uint32_t p = b, f1 = b, f1_len = 0, f4 = 0, f4e = 0, f5 = 0, f5e = 0;
            int nf = 0;
            for (int f = 1; f <= 5; ++f) {
                while (p < e) { const uint8_t c = text[p]; if (c != ' ' && c != '\t') break; ++p; }
                if (p >= e) break;
                const uint32_t fs = p;
                if (f == 3) {
                    // "transcript" has no border but the single 't', so a mismatch falls back to state 1 on 't' and to 0 otherwise
                    uint32_t st = 0, w4 = 0;
                    bool has = false;
                    while (p < e) {
                        const uint8_t c = text[p];
                        if (c == ' ' || c == '\t') break;
                        const uint64_t word_lo = 0x697263736e617274ull;      // "transcri", little endian; 'p' and 't' follow
                        const uint8_t want = st < 8u ? (uint8_t)(word_lo >> (8u * st)) : st == 8u ? (uint8_t)'p' : (uint8_t)'t';
                        st = c == want ? st + 1u : c == (uint8_t)'t' ? 1u : 0u;
                        if (st == 10u) { has = true; st = 1u; }
                        if (p - fs < 4u) w4 |= (uint32_t)c << (8u * (p - fs));
                        ++p;
                    }
                    const uint32_t len = p - fs;
                    kept = has || (len == 4u && w4 == 0x6e6f7865u);        // "exon"
                    tx = has && len == 10u;
                } else {
                    while (p < e) { const uint8_t c = text[p]; if (c == ' ' || c == '\t') break; ++p; }
                    if (f == 1) { f1 = fs; f1_len = p - fs; }
                    if (f == 4) { f4 = fs; f4e = p; }
                    if (f == 5) { f5 = fs; f5e = p; }
                }
                nf = f;
                if (f == 3 && !tx) break;
            }
            if (tx) {
                uint32_t s = 0, en = 0;
                bad = nf < 5 || !gtf_number(text, f4, f4e, &s) || !gtf_number(text, f5, f5e, &en);
                o.name_off[j] = f1; o.name_len[j] = f1_len; o.s[j] = s; o.e[j] = en;
            }
        }
        o.kept[j] = kept ? 1u : 0u;
        o.tx[j] = tx ? 1u : 0u;
    }
    const unsigned long long m = __ballot(bad);
    if (m && lane == (int)__ffsll((long long)m) - 1) atomicMin(bad_line, j + 1u);       // lines ascend with the lanes
}

struct GtfRowCols { uint32_t *__restrict__ start, *__restrict__ len, *__restrict__ line, *__restrict__ tx; };      // per kept line, in line order
struct GtfTxCols { uint32_t *__restrict__ name_off, *__restrict__ name_len, *__restrict__ s, *__restrict__ e; };   // per transcript line, in line order

// kept_at / tx_at: the flags after their exclusive scans (n_lines + 1 words)
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_rows(const uint32_t *__restrict__ start, uint32_t n, uint32_t n_lines, const uint32_t *__restrict__ kept_at, const uint32_t *__restrict__ tx_at, GtfLineCols in,
                uint32_t n_rows, uint32_t n_tx, GtfRowCols rows, GtfTxCols txs)
{
    const uint32_t j = blockIdx.x * GTF_THREADS + threadIdx.x;
    if (j >= n_lines) return;
    const uint32_t r = kept_at[j], t = tx_at[j], t_in = tx_at[j + 1u];
    if (kept_at[j + 1u] != r && r < n_rows) {
        uint32_t b = start[j], e = start[j + 1u] - 1u;
        if (e > n) e = n;
        if (b > e) b = e;
        rows.start[r] = b; rows.len[r] = e - b; rows.line[r] = j + 1u;
        rows.tx[r] = t_in ? t_in - 1u : GTF_NONE;        // the last transcript line at or before this one
    }
    if (t_in != t && t < n_tx) { txs.name_off[t] = in.name_off[j]; txs.name_len[t] = in.name_len[j]; txs.s[t] = in.s[j]; txs.e[t] = in.e[j]; }
}

// head: 0 or 1 per transcript, n_tx + 1 words
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_chr_heads(const uint8_t *__restrict__ text, uint32_t n, GtfTxCols txs, uint32_t n_tx, uint32_t *__restrict__ head)
{
    const uint32_t t = blockIdx.x * GTF_THREADS + threadIdx.x;
    if (t >= n_tx) return;
    bool is_head = t == 0u;
    if (!is_head) {
        const uint32_t len = txs.name_len[t], a = txs.name_off[t], b = txs.name_off[t - 1u];
        is_head = len != txs.name_len[t - 1u];
        if (!is_head && a <= n && b <= n && len <= n - a && len <= n - b)
            for (uint32_t k = 0; k < len && !is_head; ++k) is_head = text[a + k] != text[b + k];
    }
    head[t] = is_head ? 1u : 0u;
}

// head_at: head[] after its exclusive scan
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_head_take(const uint32_t *__restrict__ head_at, GtfTxCols txs, uint32_t n_tx, uint32_t n_heads, uint32_t *__restrict__ off, uint32_t *__restrict__ len)
{
    const uint32_t t = blockIdx.x * GTF_THREADS + threadIdx.x;
    if (t >= n_tx) return;
    const uint32_t h = head_at[t];
    if (head_at[t + 1u] != h && h < n_heads) { off[h] = txs.name_off[t]; len[h] = txs.name_len[t]; }
}

struct GtfTriple { uint32_t c, s, e; };
struct GtfTripleIn { const uint32_t *__restrict__ row_tx, *__restrict__ head_at, *__restrict__ rank, *__restrict__ tx_s, *__restrict__ tx_e; uint32_t n_tx, n_heads; };

__device__ __forceinline__ GtfTriple gtf_triple(const GtfTripleIn &in, uint32_t r)
{
    GtfTriple k{0u, 0u, 0u};
    const uint32_t t = in.row_tx[r];
    if (t != GTF_NONE && t < in.n_tx) {
        const uint32_t h = in.head_at[t + 1u] - 1u;      // heads at or before t, less one: t's own head
        k.c = h < in.n_heads ? in.rank[h] : 0u;
        k.s = in.tx_s[t]; k.e = in.tx_e[t];
    }
    return k;
}

__device__ __forceinline__ bool gtf_below(const GtfTriple &a, const GtfTriple &b) { return a.c != b.c ? a.c < b.c : a.s != b.s ? a.s < b.s : a.e < b.e; }

// c, s, e: one word per row.  *descends |= 1 where a row's triple is below its predecessor's.
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_triples(GtfTripleIn in, uint32_t n_rows, uint32_t *__restrict__ c, uint32_t *__restrict__ s, uint32_t *__restrict__ e, uint32_t *__restrict__ descends)
{
    const uint32_t r = blockIdx.x * GTF_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = r < n_rows;
    GtfTriple k{0u, 0u, 0u};
    if (active) { k = gtf_triple(in, r); c[r] = k.c; s[r] = k.s; e[r] = k.e; }
    GtfTriple p;
    p.c = (uint32_t)__shfl_up((int)k.c, 1, 64); p.s = (uint32_t)__shfl_up((int)k.s, 1, 64); p.e = (uint32_t)__shfl_up((int)k.e, 1, 64);
    if (lane == 0 && active && r > 0u) p = gtf_triple(in, r - 1u);
    const bool down = active && r > 0u && gtf_below(k, p);
    if (__any(down) && lane == 0) atomicOr(descends, 1u);
}

// the key of stage 1: e
struct GtfEndKeyOf {
    const uint32_t *__restrict__ e;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return (uint64_t)e[i]; }
};
// the key of stage 2: c << 32 | s of the row at rank i of stage 1 (order1 null: stage 1 left the identity)
struct GtfChrStartKeyOf {
    const uint32_t *__restrict__ c, *__restrict__ s, *__restrict__ order1; uint32_t n;
    __device__ __forceinline__ uint64_t key(int64_t i) const
    {
        uint32_t r = order1 ? order1[i] : (uint32_t)i;
        if (r >= n) r = n - 1u;
        return (uint64_t)c[r] << 32 | (uint64_t)s[r];
    }
};

// order1 / perm2 null: that stage left the identity
__global__ __launch_bounds__(GTF_THREADS)
void k_gtf_compose(const uint32_t *__restrict__ order1, const uint32_t *__restrict__ perm2, uint32_t n, uint32_t *__restrict__ order)
{
    const uint32_t k = blockIdx.x * GTF_THREADS + threadIdx.x;
    if (k >= n) return;
    uint32_t p = perm2 ? perm2[k] : k;
    if (p >= n) p = n - 1u;
    uint32_t r = order1 ? order1[p] : p;
    if (r >= n) r = n - 1u;
    order[k] = r;
}

}  // namespace l2r
