// l2r_detail.hip.h -- the kernels of l2r_detail_* (include/lr2rmats_hip.h): the per-read detail table of `update-gtf -A`, one text line
// per read, the text composed on the device.
//
//   k_detail_measure<false>  one thread per read: its domain error, or the exact bytes of its line and the split -- where the segments
//                            1..6 (starts, ends, L1, L2, L3, L4) begin in the line, DETAIL_SPLIT words per read
//   k_detail_measure<true>   one wave per read (hundreds of exons): lane l takes the exons l, l + 64, ...; the counts and the digit sums
//                            are wave reductions
//   (k_scan_u32 over the lengths of one batch: line offsets and the batch's byte count)
//   k_detail_write           one workgroup of 256 lanes per L2R_DETAIL_TILE consecutive reads of the batch, whose text is one contiguous
//                            span of the output.  Lines differ a hundredfold in length, so the work items are not the lines but their
//                            SEGMENTS, seven per read, each with its place from the split: no item waits for another.  A lane takes a
//                            segment of a short read and walks it; the list segments of a read with more than DETAIL_LONG exons go on
//                            a list (LDS) that the four waves then share: a wave's lanes take 64 exons a round and place their members
//                            by a wave prefix sum of the member lengths.  The lines go into the LDS image of the span, which the
//                            workgroup then streams out (l2r_text.hip.h); a span beyond L2R_DETAIL_LDS_BYTES is written straight to
//                            the text.
//
// The rule of a line, the order its domain errors are looked for and the length pieces are in l2r_detailplan.hip.h.  A domain error goes
// into one 64-bit word by atomicMin on read << 4 | kind.  The results are those of the last l2r_run where its kernels left them, or
// uploaded ones in the same layout (32-bit exon offsets, the exon count in info >> 8).  k_detail_write runs only behind rows without an
// error; a byte that would leave its segment (measure and write disagreeing: a bug) is not written and counted instead, as is a segment
// that does not end where the split says.  No workgroup waits for another.  Plain stores throughout; wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lr2rmats_hip.h"
#include "l2r_detailplan.hip.h"
#include "l2r_text.hip.h"

namespace l2r {

constexpr int DETAIL_TILE = L2R_DETAIL_TILE;            // reads of one workgroup of k_detail_write
constexpr int DETAIL_THREADS = 256;                     // its lanes
constexpr uint32_t DETAIL_LDS = L2R_DETAIL_LDS_BYTES;   // bytes of a tile's text the LDS image holds
constexpr uint32_t DETAIL_LONG = 64;                    // exons beyond which a read's list segments are a wave's work
static_assert(DETAIL_TILE >= 1 && DETAIL_LDS % 16 == 0 && DETAIL_LDS + 16 + 4 * (DETAIL_SPLIT * DETAIL_TILE + 8) <= 65536, "k_detail_write: one LDS image, one list of the long segments");

struct DetailIn {
    int64_t n;                                          // reads
    const int32_t *tid; const uint8_t *names; int64_t names_len; const uint32_t *qname;
    const uint32_t *ex_off, *info; const int32_t *xs, *xe, *ref_tx; const uint8_t *f;
    int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;
    int64_t n_tx, anno_names_len; const uint8_t *anno_names; const uint32_t *tx_gid, *tx_gname;
};

// words of k_detail_measure's result
struct DetailMeasure { uint32_t *len, *split; unsigned long long *bad; };

template <bool WAVE_FORM>
__global__ __launch_bounds__(256)
void k_detail_measure(DetailIn in, DetailMeasure out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = WAVE_FORM ? g >> 6 : g;
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= in.n) return;                                          // (wave form: the whole wave leaves; thread form: no wave operation follows)
    int kind = DET_OK;
    uint32_t qlen = 0u, chr = 0u, gid = 2u, gname = 2u, n = 0u, off = 0u;
    const int32_t tid = in.tid[i];
    if (tid < 0 || tid >= in.n_ref) kind = DET_E_TID;
    else {
        chr = (uint32_t)(in.ref_off[tid + 1] - in.ref_off[tid]);
        int e = gtx_name_len(in.names, in.names_len, in.qname[i], &qlen);
        if (e) kind = e == GTX_E_NAME_ID ? DET_E_QNAME_ID : e == GTX_E_NAME_LONG ? DET_E_QNAME_LONG : DET_E_QNAME_NUL;
        else {
            const int32_t ref = in.ref_tx[i];
            if (ref >= 0 && (int64_t)ref >= in.n_tx) kind = DET_E_REF;
            else if (ref >= 0) {
                e = gtx_name_len(in.anno_names, in.anno_names_len, in.tx_gid[ref], &gid);
                if (!e) e = gtx_name_len(in.anno_names, in.anno_names_len, in.tx_gname[ref], &gname);
                if (e) kind = e == GTX_E_NAME_ID ? DET_E_GENE_ID : e == GTX_E_NAME_LONG ? DET_E_GENE_LONG : DET_E_GENE_NUL;
            }
        }
        if (!kind) { n = in.info[i] >> 8; off = in.ex_off[i]; if (n < 1u) kind = DET_E_NOEXON; }
    }
    uint64_t total = 0;
    uint32_t split[DETAIL_SPLIT] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (!kind) {                                                    // (wave-uniform: every lane has looked at the same words)
        DetailSums s = {0, 0, {0u, 0u, 0u, 0u}, {0, 0, 0, 0}};
        bool neg = false;
        uint32_t sx = 0u, se = 0u, c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u, m0 = 0u, m1 = 0u, m2 = 0u, m3 = 0u;   // (at most 2^24 exons of 22 bytes)
        for (uint32_t j = WAVE_FORM ? lane : 0u; j < n; j += WAVE_FORM ? 64u : 1u) {
            const int32_t a = in.xs[off + j], b = in.xe[off + j];
            const uint32_t f = in.f[off + j];
            neg |= (a | b) < 0;
            sx += text_digits((uint32_t)a) + 1u; se += text_digits((uint32_t)b) + 1u;
            uint32_t c, m;
            detail_members(j, n, f, 0, c, m); c0 += c; m0 += m;
            detail_members(j, n, f, 1, c, m); c1 += c; m1 += m;
            detail_members(j, n, f, 2, c, m); c2 += c; m2 += m;
            detail_members(j, n, f, 3, c, m); c3 += c; m3 += m;
        }
        if (WAVE_FORM) {
            sx = wave_sum(sx); se = wave_sum(se);
            c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2); c3 = wave_sum(c3);
            m0 = wave_sum(m0); m1 = wave_sum(m1); m2 = wave_sum(m2); m3 = wave_sum(m3);
            neg = __any(neg) != 0;
        }
        s.xs = sx; s.xe = se;
        s.cnt[0] = c0; s.cnt[1] = c1; s.cnt[2] = c2; s.cnt[3] = c3;
        s.mem[0] = m0; s.mem[1] = m1; s.mem[2] = m2; s.mem[3] = m3;
        total = detail_split(detail_head_len(qlen, chr, gid, gname, n), s, split);
        if (neg) kind = DET_E_NEG;
        else if (total >= DETAIL_BATCH_BYTES) kind = DET_E_BIG;
    }
    if (WAVE_FORM && lane) return;
    if (kind) {
        atomicMin(out.bad, (unsigned long long)i << 4 | (unsigned long long)kind);
        total = 0;
#pragma unroll
        for (int k = 0; k < DETAIL_SPLIT; ++k) split[k] = 0u;
    }
    out.len[i] = (uint32_t)total;
    uint32_t *sp = out.split + (size_t)i * DETAIL_SPLIT;
#pragma unroll
    for (int k = 0; k < DETAIL_SPLIT; ++k) sp[k] = split[k];
}

// one byte at p where p lies in front of `end`; returns the byte behind it
__device__ __forceinline__ uint8_t *detail_put_byte(uint8_t *p, uint8_t c, const uint8_t *end) { if (p < end) *p = c; return p + 1; }

// A number and the byte behind it at dst[pos .. ), where that stays in front of hi; returns the bytes it did NOT write
__device__ __forceinline__ uint32_t detail_put_member(uint8_t *dst, uint32_t pos, uint32_t hi, uint32_t v, uint8_t behind)
{
    const uint32_t d = text_digits(v);
    if (pos + d + 1u > hi) return d + 1u;
    *text_put_num(dst + pos, v) = behind;
    return 0u;
}

// The head of read i's line at dst[lo, hi): <qname>\t<chr>\t<+|->\t<cls>\t<gid>\t<gname>\t<n>\t.  Returns what it could not place.
__device__ __forceinline__ uint32_t detail_put_head(uint8_t *dst, uint32_t lo, uint32_t hi, const DetailIn &in, int64_t i, uint32_t info)
{
    uint8_t *p = dst + lo;
    const uint8_t *end = dst + hi;
    p = text_put_name(p, in.names + in.qname[i], L2R_DETAIL_NAME_MAX, end); p = detail_put_byte(p, '\t', end);
    const int32_t tid = in.tid[i];
    for (int64_t k = in.ref_off[tid]; k < in.ref_off[tid + 1]; ++k) p = detail_put_byte(p, in.ref_names[k], end);
    p = detail_put_byte(p, '\t', end);
    p = detail_put_byte(p, (info & L2R_INFO_REV) ? '-' : '+', end); p = detail_put_byte(p, '\t', end);
    p = detail_put_byte(p, (uint8_t)('0' + detail_cls(info)), end); p = detail_put_byte(p, '\t', end);
    const int32_t ref = in.ref_tx[i];
    if (ref < 0) {
        p = detail_put_byte(p, 'N', end); p = detail_put_byte(p, 'A', end); p = detail_put_byte(p, '\t', end);
        p = detail_put_byte(p, 'N', end); p = detail_put_byte(p, 'A', end); p = detail_put_byte(p, '\t', end);
    } else {
        p = text_put_name(p, in.anno_names + in.tx_gid[ref], L2R_DETAIL_NAME_MAX, end); p = detail_put_byte(p, '\t', end);
        p = text_put_name(p, in.anno_names + in.tx_gname[ref], L2R_DETAIL_NAME_MAX, end); p = detail_put_byte(p, '\t', end);
    }
    const uint32_t n = info >> 8, d = text_digits(n);
    if (p + d + 1u <= end) *text_put_num(p, n) = '\t';
    p += d + 1u;
    return p == end ? 0u : p > end ? (uint32_t)(p - end) : 1u;
}

// ---- a lane walks a whole segment

// n numbers a[0 .. n), a comma between them and a tab behind the last, at dst[lo, hi)
__device__ __forceinline__ uint32_t detail_coords_lane(uint8_t *dst, uint32_t lo, uint32_t hi, const int32_t *__restrict__ a, uint32_t n)
{
    uint32_t pos = lo, out = 0u;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t v = (uint32_t)a[j];
        out += detail_put_member(dst, pos, hi, v, j + 1u < n ? ',' : '\t');
        pos += text_digits(v) + 1u;
    }
    return out + (pos != hi ? 1u : 0u);
}

// the start of list k with cnt members at dst[lo, hi): <cnt>\t, and NA\t (for L4 the newline too) where it is empty.  pos: behind it
__device__ __forceinline__ uint32_t detail_list_front(uint8_t *dst, uint32_t lo, uint32_t hi, int k, uint32_t cnt, uint32_t &pos)
{
    const uint32_t d = text_digits(cnt), front = d + 1u + (cnt ? 0u : k == 3 ? 4u : 3u);
    pos = lo + front;
    if (pos > hi) return front;
    uint8_t *p = text_put_num(dst + lo, cnt);
    *p++ = '\t';
    if (!cnt) { *p++ = 'N'; *p++ = 'A'; *p++ = '\t'; if (k == 3) *p = '\n'; }
    return 0u;
}

// list k over the flags f[0 .. n) at dst[lo, hi)
__device__ __forceinline__ uint32_t detail_list_lane(uint8_t *dst, uint32_t lo, uint32_t hi, const uint8_t *__restrict__ f, uint32_t n, int k)
{
    uint32_t cnt = 0u, v[2];
    for (uint32_t j = 0; j < n; ++j) cnt += detail_member_vals(j, n, f[j], k, v);
    uint32_t pos, out = detail_list_front(dst, lo, hi, k, cnt, pos);
    const uint8_t behind = k == 3 ? '\n' : '\t';
    uint32_t left = cnt;
    for (uint32_t j = 0; j < n && left; ++j) {
        const uint32_t c = detail_member_vals(j, n, f[j], k, v);
        if (c > 0u) { --left; out += detail_put_member(dst, pos, hi, v[0], left ? ',' : behind); pos += text_digits(v[0]) + 1u; }
        if (c > 1u) { --left; out += detail_put_member(dst, pos, hi, v[1], left ? ',' : behind); pos += text_digits(v[1]) + 1u; }
    }
    return out + (pos != hi ? 1u : 0u);
}

// ---- a wave shares a segment: 64 exons a round, the members placed by a wave prefix sum of their lengths (all 64 lanes are here)

__device__ __forceinline__ uint32_t detail_coords_wave(uint8_t *dst, uint32_t lo, uint32_t hi, const int32_t *__restrict__ a, uint32_t n, uint32_t lane)
{
    uint32_t run = lo, out = 0u;
    for (uint32_t base = 0u; base < n; base += 64u) {
        const uint32_t j = base + lane;
        const bool live = j < n;
        const uint32_t v = live ? (uint32_t)a[j] : 0u, len = live ? text_digits(v) + 1u : 0u;
        const uint32_t inc = wave_inclusive_scan(len);
        if (live) out += detail_put_member(dst, run + inc - len, hi, v, j + 1u < n ? ',' : '\t');
        run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    return out + (lane == 0u && run != hi ? 1u : 0u);
}

__device__ __forceinline__ uint32_t detail_list_wave(uint8_t *dst, uint32_t lo, uint32_t hi, const uint8_t *__restrict__ f, uint32_t n, int k, uint32_t lane)
{
    uint32_t mine = 0u, v[2];
    for (uint32_t j = lane; j < n; j += 64u) mine += detail_member_vals(j, n, f[j], k, v);
    const uint32_t cnt = wave_sum(mine);
    uint32_t run = 0u, out = 0u;
    {   uint32_t pos;
        const uint32_t o = detail_list_front(dst, lo, lane == 0u ? hi : 0u, k, cnt, pos);      // (lane 0 writes it; the others only learn pos)
        if (lane == 0u) out = o;
        run = pos; }
    const uint8_t behind = k == 3 ? '\n' : '\t';
    uint32_t seen = 0u;                                 // members of the rounds before
    for (uint32_t base = 0u; base < n && seen < cnt; base += 64u) {
        const uint32_t j = base + lane;
        const uint32_t c = j < n ? detail_member_vals(j, n, f[j], k, v) : 0u;
        const uint32_t l0 = c > 0u ? text_digits(v[0]) + 1u : 0u, l1 = c > 1u ? text_digits(v[1]) + 1u : 0u;
        const uint32_t inc = wave_inclusive_scan(l0 + l1), cinc = wave_inclusive_scan(c);
        const uint32_t pos = run + inc - (l0 + l1), ord = seen + cinc - c;      // my first member's place, and how many stand in front of it
        if (c > 0u) out += detail_put_member(dst, pos, hi, v[0], ord + 1u < cnt ? ',' : behind);
        if (c > 1u) out += detail_put_member(dst, pos + l0, hi, v[1], ord + 2u < cnt ? ',' : behind);
        run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        seen += (uint32_t)__builtin_amdgcn_readlane((int)cinc, 63);
    }
    return out + (lane == 0u && run != hi ? 1u : 0u);
}

// words of k_detail_write's counters
enum { DETC_DIRECT = 0, DETC_OUTSIDE, DETC_LONG, DETC_N };

// one segment's place: dst[lo, hi) of read i with n exons at `off`; false where the split does not fit the line or the line its tile
struct DetailSeg { int64_t i; uint32_t k, lo, hi, n, info, off; };
__device__ __forceinline__ bool detail_seg(const DetailIn &in, int64_t first, int64_t i0, uint32_t item, const uint32_t *__restrict__ off, const uint32_t *__restrict__ split,
                                           uint32_t b0, uint32_t bytes, DetailSeg &s)
{
    const uint32_t r = item / (uint32_t)DETAIL_SEGS;
    s.k = item - r * (uint32_t)DETAIL_SEGS;
    const int64_t q = i0 + r;
    s.i = first + q;
    const uint32_t line0 = off[q] - b0, line_len = off[q + 1] - off[q];
    const uint32_t *sp = split + (size_t)s.i * DETAIL_SPLIT;
    const uint32_t a = s.k ? sp[s.k - 1u] : 0u, b = s.k < (uint32_t)DETAIL_SPLIT ? sp[s.k] : line_len;
    s.lo = line0 + a; s.hi = line0 + b;
    s.info = in.info[s.i]; s.n = s.info >> 8; s.off = in.ex_off[s.i];
    return a <= b && b <= line_len && (uint64_t)line0 + line_len <= bytes;
}

// The reads [first, first + count) of the rows; off: the scanned lengths of the batch (count + 1 words), split: of all the rows.
__global__ __launch_bounds__(DETAIL_THREADS)
void k_detail_write(DetailIn in, int64_t first, int64_t count, const uint32_t *__restrict__ off, const uint32_t *__restrict__ split, uint8_t *__restrict__ text,
                    uint32_t *__restrict__ counters)
{
    __shared__ uint4 s_img[DETAIL_LDS / 16 + 1];        // the image of the tile's span (l2r_text.hip.h)
    __shared__ uint32_t s_long[DETAIL_SPLIT * DETAIL_TILE];     // the segments left to the waves
    __shared__ uint32_t s_n_long;
    const int64_t i0 = (int64_t)blockIdx.x * DETAIL_TILE, i1 = i0 + DETAIL_TILE < count ? i0 + DETAIL_TILE : count;
    const uint32_t n_items = (uint32_t)(i1 - i0) * (uint32_t)DETAIL_SEGS;
    const uint32_t b0 = off[i0], b1 = off[i1], bytes = b1 - b0;
    const bool direct = bytes > DETAIL_LDS;             // (workgroup-uniform)
    uint8_t *dst = direct ? text + b0 : text_image(s_img, text_head(b0));
    if (threadIdx.x == 0) s_n_long = 0u;
    __syncthreads();
    uint32_t outside = 0u;
    for (uint32_t item = threadIdx.x; item < n_items; item += DETAIL_THREADS) {
        DetailSeg s;
        if (!detail_seg(in, first, i0, item, off, split, b0, bytes, s)) { ++outside; continue; }
        if (s.k == 0u) outside += detail_put_head(dst, s.lo, s.hi, in, s.i, s.info);
        else if (s.n > DETAIL_LONG) s_long[atomicAdd(&s_n_long, 1u)] = item;
        else if (s.k <= 2u) outside += detail_coords_lane(dst, s.lo, s.hi, (s.k == 1u ? in.xs : in.xe) + s.off, s.n);
        else outside += detail_list_lane(dst, s.lo, s.hi, in.f + s.off, s.n, (int)s.k - 3);
    }
    __syncthreads();
    const uint32_t n_long = s_n_long, lane = threadIdx.x & 63u;
    for (uint32_t it = threadIdx.x >> 6; it < n_long; it += DETAIL_THREADS / 64) {         // (wave-uniform)
        DetailSeg s;
        (void)detail_seg(in, first, i0, s_long[it], off, split, b0, bytes, s);              // (it was sound in the first round)
        if (s.k <= 2u) outside += detail_coords_wave(dst, s.lo, s.hi, (s.k == 1u ? in.xs : in.xe) + s.off, s.n, lane);
        else outside += detail_list_wave(dst, s.lo, s.hi, in.f + s.off, s.n, (int)s.k - 3, lane);
    }
    if (outside) atomicAdd(counters + DETC_OUTSIDE, outside);
    if (threadIdx.x == 0) { if (n_long) atomicAdd(counters + DETC_LONG, n_long); if (direct) atomicAdd(counters + DETC_DIRECT, 1u); }
    if (direct) return;
    __syncthreads();
    text_stream_out<DETAIL_THREADS>(s_img, b0, bytes, text);
}

}  // namespace l2r
