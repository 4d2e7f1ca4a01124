// l2r_bed.hip.h -- the kernels of `bam2bed` (l2r_bed_lines, include/lr2rmats_hip.h): alignment records as BED12 text, the text composed
// on the device.
//
//   k_bed_measure<false>  one thread per record, a serial walk over its CIGAR words: the bytes of its line (0 for an unmapped record), its
//                         block count, its span and the bytes of its block-size column
//   k_bed_measure<true>   one wave per record (long-read CIGARs): lane l takes the words l, l + 64, ...; a wave prefix sum of the reference
//                         advances gives every operation its place, a ballot the N operations, and a block's size is the prefix in front
//                         of its N minus the prefix behind the N before (the carried block start where the round has none in front)
//   (k_scan_u32 over the line lengths: line offsets and the batch's byte count)
//   k_bed_write           one workgroup per L2R_BED_TILE consecutive records, whose text is one contiguous span of the output.  One thread
//                         per record walks its CIGAR again (cheaper than storing every block) and writes digits, names and punctuation
//                         into the LDS image of the span, which the workgroup then streams out (l2r_text.hip.h).  A span beyond
//                         L2R_BED_LDS_BYTES (long names, hundreds of blocks) is written line by line straight to the text.
//
// The rule of a line is stated in l2r_bedplan.hip.h.  A domain error (reference outside the table, negative position, operation code above
// 8, end beyond 2147483647) goes into one word by atomicMin on the record index; the host names its kind.  Sums are 64 bit in the measure
// kernels (a bad record's numbers may be anything); k_bed_write runs only behind a batch without an error, where every number fits 31 bits.
// Plain stores throughout; wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lr2rmats_hip.h"
#include "l2r_bedplan.hip.h"
#include "l2r_text.hip.h"

namespace l2r {

constexpr int BED_TILE = L2R_BED_TILE;                  // records, and threads, of one workgroup of k_bed_write
constexpr uint32_t BED_LDS = L2R_BED_LDS_BYTES;         // bytes of a tile's text the LDS image holds
static_assert(BED_TILE % 64 == 0 && BED_TILE <= 1024 && BED_LDS % 16 == 0 && BED_LDS + 16 <= 65536, "k_bed_write: one workgroup, one LDS image");

// One batch on the device.  cig / names hold the batch's own words and bytes: record i's are [cig_off[i] - cig_base, cig_off[i + 1] - cig_base).
struct BedIn {
    int64_t n;
    const uint16_t *flag; const int32_t *tid, *pos; const uint8_t *mapq;
    const int64_t *cig_off; const uint32_t *cig; int64_t cig_base;
    const int64_t *name_off; const uint8_t *names; int64_t name_base;
    int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;
    uint32_t color_len, color_w0, color_w1, color_w2;   // the colour's bytes, four to a word
};
// what k_bed_measure leaves per record: len is scanned in place into the line offsets (n + 1 words)
struct BedMeasure { uint32_t *len, *n_blocks, *span, *size_len; };

__device__ __forceinline__ uint64_t bed_shfl64(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
    return (uint64_t)hi << 32 | lo;
}

template <bool WAVE_FORM>
__global__ __launch_bounds__(256)
void k_bed_measure(BedIn in, BedMeasure out, uint32_t *__restrict__ bad_record)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = WAVE_FORM ? t >> 6 : t;
    if (i >= in.n) return;                                          // (WAVE_FORM: the whole wave leaves)
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t f = in.flag[i];
    if (f & 4u) {
        if (!WAVE_FORM || lane == 0) { out.len[i] = 0u; out.n_blocks[i] = 0u; out.span[i] = 0u; out.size_len[i] = 0u; }
        return;
    }
    const int32_t tid = in.tid[i], pos = in.pos[i];
    bool bad = tid < 0 || tid >= in.n_ref || pos < 0;
    const int64_t c0 = in.cig_off[i] - in.cig_base, c1 = in.cig_off[i + 1] - in.cig_base;
    uint64_t cur = 0;
    uint32_t n_blocks = 1u, size_len = 0u, start_len = 1u;          // (the first start is "0")
    if (!WAVE_FORM) {
        uint64_t blen = 0;
        for (int64_t k = c0; k < c1; ++k) {
            const uint32_t w = in.cig[k], op = w & 0xfu, l = w >> 4;
            bad |= op > 8u;
            if (op == 3u) { size_len += text_digits64(blen) + 1u; cur += l; start_len += text_digits64(cur) + 1u; blen = 0; ++n_blocks; }
            else if ((BED_ADVANCE >> op) & 1u) { cur += l; blen += l; }
        }
        size_len += text_digits64(blen);
    } else {
        uint64_t block_start = 0;                                   // where the block that is open at the round's start began
        uint32_t my_size = 0u, my_start = 0u;
        for (int64_t base = c0; base < c1; base += 64) {            // (wave-uniform)
            const int64_t k = base + lane;
            const bool valid = k < c1;
            const uint32_t w = valid ? in.cig[k] : 0u, op = w & 0xfu, l = w >> 4;
            bad |= op > 8u;
            const uint32_t adv = ((BED_ADVANCE >> op) & 1u) ? l : 0u;
            const bool is_n = valid && op == 3u;
            // 64 advances of up to 2^28 - 1: two 32-bit scans of their halves are exact
            const uint64_t incl = cur + (uint64_t)wave_inclusive_scan(adv & 0xffffu) + ((uint64_t)wave_inclusive_scan(adv >> 16) << 16);
            const unsigned long long m = __ballot(is_n);
            const unsigned long long below = m & ((1ull << lane) - 1ull);
            const uint64_t prev = bed_shfl64(incl, below ? 63 - __clzll((long long)below) : 0);
            if (is_n) {
                my_size += text_digits64(incl - l - (below ? prev : block_start)) + 1u;
                my_start += text_digits64(incl) + 1u;
            }
            if (m) { block_start = bed_shfl64(incl, 63 - __clzll((long long)m)); n_blocks += (uint32_t)__popcll(m); }
            cur = bed_shfl64(incl, 63);
        }
        size_len = wave_sum(my_size) + text_digits64(cur - block_start);
        start_len += wave_sum(my_start);
        bad = __any(bad) != 0;
        if (lane) return;
    }
    const uint64_t end = (uint64_t)(uint32_t)pos + cur;
    bad |= end > 2147483647ull;
    uint32_t len = 0u;
    if (bad) atomicMin(bad_record, (uint32_t)i);
    else {
        const uint32_t chrom = (uint32_t)(in.ref_off[tid + 1] - in.ref_off[tid]), name = (uint32_t)(in.name_off[i + 1] - in.name_off[i]);
        len = chrom + 2u * (text_digits((uint32_t)pos) + text_digits((uint32_t)end)) + name + ((f & 0xc0u) ? 2u : 0u) + text_digits(in.mapq[i]) + 1u + in.color_len +
              text_digits(n_blocks) + size_len + start_len + 12u;
    }
    out.len[i] = len; out.n_blocks[i] = n_blocks; out.span[i] = (uint32_t)cur; out.size_len[i] = size_len;
}

// The line of the mapped record i at dst (LDS or the text itself): exactly the bytes k_bed_measure counted.
__device__ __forceinline__ void bed_put_line(uint8_t *dst, const BedIn &in, int64_t i, uint32_t n_blocks, uint32_t span, uint32_t size_len)
{
    const uint32_t f = in.flag[i], pos = (uint32_t)in.pos[i], end = pos + span;
    const int32_t tid = in.tid[i];
    uint8_t *p = dst;
    for (int64_t k = in.ref_off[tid]; k < in.ref_off[tid + 1]; ++k) *p++ = in.ref_names[k];
    *p++ = '\t'; p = text_put_num(p, pos); *p++ = '\t'; p = text_put_num(p, end); *p++ = '\t';
    for (int64_t k = in.name_off[i] - in.name_base; k < in.name_off[i + 1] - in.name_base; ++k) *p++ = in.names[k];
    if (f & 0xc0u) { *p++ = '/'; *p++ = (f & 0x40u) ? '1' : '2'; }
    *p++ = '\t'; p = text_put_num(p, in.mapq[i]); *p++ = '\t'; *p++ = (f & 16u) ? '-' : '+';
    *p++ = '\t'; p = text_put_num(p, pos); *p++ = '\t'; p = text_put_num(p, end); *p++ = '\t';
    for (uint32_t k = 0; k < in.color_len; ++k) {
        const uint32_t w = k < 4u ? in.color_w0 : k < 8u ? in.color_w1 : in.color_w2;
        *p++ = (uint8_t)(w >> ((k & 3u) * 8u));
    }
    *p++ = '\t'; p = text_put_num(p, n_blocks); *p++ = '\t';
    // the sizes from p on, the starts behind them: one walk, two cursors
    uint8_t *q = p + size_len;
    *q++ = '\t'; *q++ = '0';
    uint32_t cur = 0u, blen = 0u;
    for (int64_t k = in.cig_off[i] - in.cig_base; k < in.cig_off[i + 1] - in.cig_base; ++k) {
        const uint32_t w = in.cig[k], op = w & 0xfu, l = w >> 4;
        if (op == 3u) { p = text_put_num(p, blen); *p++ = ','; cur += l; *q++ = ','; q = text_put_num(q, cur); blen = 0u; }
        else if ((BED_ADVANCE >> op) & 1u) { cur += l; blen += l; }
    }
    (void)text_put_num(p, blen);
    *q = '\n';
}

__global__ __launch_bounds__(BED_TILE)
void k_bed_write(BedIn in, const uint32_t *__restrict__ off, const uint32_t *__restrict__ n_blocks, const uint32_t *__restrict__ span,
                 const uint32_t *__restrict__ size_len, uint8_t *__restrict__ text, uint32_t *__restrict__ n_direct)
{
    __shared__ uint4 s_img[BED_LDS / 16 + 1];           // the image of the tile's span (l2r_text.hip.h)
    const int64_t i0 = (int64_t)blockIdx.x * BED_TILE, i1 = i0 + BED_TILE < in.n ? i0 + BED_TILE : in.n;
    const uint32_t b0 = off[i0], b1 = off[i1], bytes = b1 - b0;
    if (bytes == 0u) return;                            // (a tile of unmapped records)
    const bool direct = bytes > BED_LDS;                // (workgroup-uniform)
    const uint32_t head = text_head(b0);
    const int64_t i = i0 + threadIdx.x;
    if (i < i1) {
        const uint32_t o = off[i];
        if (off[i + 1] > o) {
            if (direct) bed_put_line(text + o, in, i, n_blocks[i], span[i], size_len[i]);
            else bed_put_line(text_image(s_img, head) + (o - b0), in, i, n_blocks[i], span[i], size_len[i]);
        }
    }
    if (direct) { if (threadIdx.x == 0) atomicAdd(n_direct, 1u); return; }
    __syncthreads();
    text_stream_out<BED_TILE>(s_img, b0, bytes, text);
}

}  // namespace l2r
