// l2r_fusion.hip.h -- the kernels of `fusion` (reference src/bam_fusion.c:61-129, src/parse_bam.c:543-595 bam2seg, :261-270
// bam_query_len): per alignment record the part of the read and of the reference it covers, per read the two parts of a
// candidate gene fusion.
//
//   k_fusion_seg<false>  one thread per record, a serial walk over its CIGAR words (short-read CIGARs: a few words a record)
//   k_fusion_seg<true>   one wave per record (long-read CIGARs, hundreds of words a record): lane l reads the words l, l + 64, ...
//                        (coalesced, 256 bytes a round), sums three classes of operation lengths of its own and the wave adds the
//                        lanes up by shuffles; lane 0 adds the leading clip, applies the strand swap and stores the five words
//   k_fusion_select      one thread per group of consecutive mapped records with one read name, two passes over its rows:
//                        s0 = the first row of the reference's order (score descending, then edit distance ascending, then the
//                        earlier record), s1 = the first row behind it in that order that passes check_fusion's three tests
//                        against s0; a candidate iff the two cover all_cov of the read
//
// A record's coordinates are three sums over its CIGAR words -- only the FIRST word is special (a clip there shifts the read
// interval, a clip anywhere else adds nothing, parse_bam.c:574-580):
//     q_al = sum len(M = X I)   r_al = sum len(M = X D N)   qlen = sum len(M I S = X)
//     read = [1 + clip0, clip0 + q_al]   ref = [pos + 1, pos + r_al]   on the reverse strand read -> qlen + 1 - read, swapped
// 32-bit sums that wrap like the reference's ints.  HBM-bound integer work: 4 bytes per operation in, 20 bytes per record out.
// No atomics, no waiting between workgroups; wave64, 256 threads a workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l2r {

struct FusionPrm { float ovlp_frac, each_cov, all_cov; int32_t dis; };

#define FUSION_Q_AL 0x183u      // M I = X       read_end       (parse_bam.c:561-569)
#define FUSION_R_AL 0x18du      // M D N = X     ref_end        (:561-573)
#define FUSION_QLEN 0x193u      // M I S = X     bam_query_len  (:258-270, BAM_CIGAR_QUERY_TYPE bit 1)

template <bool WAVE>
__global__ __launch_bounds__(256)
void k_fusion_seg(int64_t n, const uint16_t *__restrict__ flag, const int32_t *__restrict__ pos, const int64_t *__restrict__ cig_off,
                  const uint32_t *__restrict__ cig, int32_t *__restrict__ read_start, int32_t *__restrict__ read_end,
                  int32_t *__restrict__ ref_start, int32_t *__restrict__ ref_end, int32_t *__restrict__ qlen)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = WAVE ? t >> 6 : t;
    if (i >= n) return;                                            // (WAVE: the whole wave leaves)
    const uint32_t f = flag[i];
    const int64_t c0 = cig_off[i], c1 = cig_off[i + 1];
    uint32_t q_al = 0, r_al = 0, ql = 0;
    if (!(f & 4u))
        for (int64_t k = c0 + (WAVE ? (int64_t)(threadIdx.x & 63u) : 0); k < c1; k += WAVE ? 64 : 1) {
            const uint32_t w = cig[k], op = w & 0xfu, len = w >> 4;
            q_al += ((FUSION_Q_AL >> op) & 1u) ? len : 0u;
            r_al += ((FUSION_R_AL >> op) & 1u) ? len : 0u;
            ql += ((FUSION_QLEN >> op) & 1u) ? len : 0u;
        }
    if (WAVE) {
        for (int d = 32; d > 0; d >>= 1) { q_al += __shfl_down(q_al, d, 64); r_al += __shfl_down(r_al, d, 64); ql += __shfl_down(ql, d, 64); }
        if (threadIdx.x & 63u) return;
    }
    uint32_t rs = 0, re = 0, fs = 0, fe = 0;
    if (!(f & 4u)) {                                               // bam_unmap: the row stays 0
        uint32_t clip0 = 0;
        if (c1 > c0) { const uint32_t w0 = cig[c0]; if ((w0 & 0xfu) == 4u || (w0 & 0xfu) == 5u) clip0 = w0 >> 4; }
        rs = 1u + clip0; re = clip0 + q_al;
        fs = (uint32_t)pos[i] + 1u; fe = (uint32_t)pos[i] + r_al;
        if (f & 16u) { const uint32_t tmp = rs; rs = ql + 1u - re; re = ql + 1u - tmp; }
    } else ql = 0;
    read_start[i] = (int32_t)rs; read_end[i] = (int32_t)re; ref_start[i] = (int32_t)fs; ref_end[i] = (int32_t)fe; qlen[i] = (int32_t)ql;
}

// ovlp_rat() src/bam_fusion.c:67-72: not symmetric -- the numerator is end1 - start2 + 1 whenever the intervals meet (the other arm
// of the ?: there cannot be taken); double division, returned as float
__device__ inline float fusion_ovlp_rat(int32_t a1, int32_t b1, int32_t a2, int32_t b2)
{
    if (a1 > b2 || a2 > b1) return 0.0f;
    const int32_t ov = (int32_t)((uint32_t)b1 - (uint32_t)a2 + 1u);
    const int32_t l1 = (int32_t)((uint32_t)b1 - (uint32_t)a1 + 1u), l2 = (int32_t)((uint32_t)b2 - (uint32_t)a2 + 1u);
    return (float)((double)ov / ((double)(l1 < l2 ? l1 : l2) + 0.0));
}

// positions of [1, rlen] inside [a, b]
__device__ inline void fusion_clip(int32_t &a, int32_t &b, int32_t rlen) { if (a < 1) a = 1; if (b > rlen) b = rlen; }

__global__ __launch_bounds__(256)
void k_fusion_select(int64_t n_groups, const int64_t *__restrict__ group_off, const int32_t *__restrict__ score, const int32_t *__restrict__ ed,
                     const int32_t *__restrict__ tid, const int32_t *__restrict__ read_start, const int32_t *__restrict__ read_end,
                     const int32_t *__restrict__ ref_start, const int32_t *__restrict__ ref_end, const int32_t *__restrict__ rlen_of_group,
                     FusionPrm p, int64_t *__restrict__ first, int64_t *__restrict__ second)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const int64_t a = group_off[g], b = group_off[g + 1];
    const int32_t rlen = rlen_of_group[g];
    int64_t i0 = -1, i1 = -1;
    if (b - a >= 2 && rlen > 0) {                                  // (bam_fusion.c:181: a group of one record is never looked at)
        // pass 1: s0, the first row of seg_cmpfunc's order (:61-65; by value, the earlier row of equal ones)
        i0 = a;
        int32_t sc0 = score[a], ed0 = ed[a];
        for (int64_t k = a + 1; k < b; ++k) {
            const int32_t s = score[k], e = ed[k];
            if (s > sc0 || (s == sc0 && e < ed0)) { i0 = k; sc0 = s; ed0 = e; }
        }
        const int32_t t0 = tid[i0], rs0 = read_start[i0], re0 = read_end[i0], fs0 = ref_start[i0], fe0 = ref_end[i0];
        // pass 2: s1, the first of the other rows in that order that passes the tests of check_fusion (:119-120)
        int32_t sc1 = 0, ed1 = 0, rs1 = 0, re1 = 0;
        for (int64_t k = a; k < b; ++k) {
            if (k == i0) continue;
            const int32_t s = score[k], e = ed[k];
            if (i1 >= 0 && !(s > sc1 || (s == sc1 && e < ed1))) continue;          // not in front of the best one so far
            const int32_t rs = read_start[k], re = read_end[k];
            if ((double)(int32_t)((uint32_t)re - (uint32_t)rs + 1u) / ((double)rlen + 0.0) < (double)p.each_cov) continue;      // :119
            if (fusion_ovlp_rat(rs0, re0, rs, re) > p.ovlp_frac) continue;                                                 // :76
            if (tid[k] == t0) {                                                                                            // :78-85
                const int32_t fs = ref_start[k], fe = ref_end[k];
                if (fusion_ovlp_rat(fs0, fe0, fs, fe) > 0.0f) continue;
                const int32_t d0 = (int32_t)((uint32_t)fs0 - (uint32_t)fe), d1 = (int32_t)((uint32_t)fs - (uint32_t)fe0);
                if ((d0 > 0 && d0 < p.dis) || (d1 > 0 && d1 < p.dis)) continue;
            }
            i1 = k; sc1 = s; ed1 = e; rs1 = rs; re1 = re;
        }
        if (i1 >= 0) {
            // bam_seg_cov (:98-112) of the two: positions of [1, rlen] in the union (intervals clipped to the read: a hard clip
            // puts read_start past a length that does not count H)
            int32_t x0 = rs0, y0 = re0, x1 = rs1, y1 = re1;
            fusion_clip(x0, y0, rlen); fusion_clip(x1, y1, rlen);
            const int32_t n0 = y0 >= x0 ? y0 - x0 + 1 : 0, n1 = y1 >= x1 ? y1 - x1 + 1 : 0;
            const int32_t lo = x0 > x1 ? x0 : x1, hi = y0 < y1 ? y0 : y1;
            const int32_t both = (n0 && n1 && hi >= lo) ? hi - lo + 1 : 0;
            const int32_t cov_n = n0 + n1 - both;
            if (!((float)(((double)cov_n + 0.0) / (double)rlen) >= p.all_cov)) { i0 = -1; i1 = -1; }                          // :123
        } else i0 = -1;
    }
    first[g] = i0; second[g] = i1;
}

}  // namespace l2r
