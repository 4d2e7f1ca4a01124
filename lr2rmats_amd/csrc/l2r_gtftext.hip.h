// l2r_gtftext.hip.h -- the kernels of l2r_gtftext_* (include/lr2rmats_hip.h): the GTF block of `bam2gtf` and `unique-gtf`, transcripts as
// GTF text, the text composed on the device.
//
//   k_gtx_measure<false>  one thread per block of the selection: its domain error, or the exact bytes of its text, its lines, and `fix`,
//                         the bytes of one of its exon lines without the two numbers (gtx_line_fix: every line of a block has the same
//                         prefix <ref>\t<src>\t and the same suffix from \t.\t on)
//   k_gtx_measure<true>   one wave per block (hundreds of exons): lanes 0..3 take a name each, lane l the exons l, l + 64, ...
//   (k_scan_u32 over the lengths of one batch: block offsets and the batch's byte count)
//   k_gtx_write           one workgroup of 256 lanes per L2R_GTX_TILE consecutive blocks of the batch, whose text is one contiguous span of
//                         the output.  Blocks differ a hundredfold in size, so the tile's LINES are spread over the lanes, not its
//                         blocks: a scan of the blocks' line counts (LDS) numbers the lines; round by round every lane takes one line,
//                         finds its block by bisection, its length from `fix` and the digits of its two numbers, and its place by a
//                         workgroup scan of the round's lengths behind the bytes of the rounds before.  The lines go into the LDS image
//                         of the span, which the workgroup then streams out (l2r_text.hip.h); a span beyond L2R_GTX_LDS_BYTES is written
//                         line by line straight to the text.
//
// The rule of a block, the order its domain errors are looked for and the length pieces are in l2r_gtftextplan.hip.h.  A domain error goes
// into one 64-bit word by atomicMin on block << 4 | kind.  The exon chains are either the uploaded ones (ex_off64) or those of the last
// l2r_run where its kernels left them (ex_off32 and the exon count in info >> 8).  k_gtx_write runs only behind a selection without an
// error; a line that would leave its tile's span (measure and write disagreeing: a bug) is not written and counted instead.
// Plain stores throughout; wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lr2rmats_hip.h"
#include "l2r_gtftextplan.hip.h"
#include "l2r_text.hip.h"

namespace l2r {

constexpr int GTX_TILE = L2R_GTX_TILE;                  // blocks of one workgroup of k_gtx_write
constexpr int GTX_THREADS = 256;                        // its lanes
constexpr uint32_t GTX_LDS = L2R_GTX_LDS_BYTES;         // bytes of a tile's text the LDS image holds
static_assert(GTX_TILE >= 1 && GTX_TILE < GTX_THREADS && GTX_LDS % 16 == 0 && GTX_LDS + 16 + 4 * (GTX_TILE + 8) <= 65536, "k_gtx_write: one workgroup, one scan of the line counts, one LDS image");

struct GtxIn {
    int64_t n, m;                                       // transcripts; blocks of the selection
    const int32_t *tid; const uint8_t *rev;
    const int64_t *ex_off64;                            // n + 1, or null: the chains of the last run
    const uint32_t *ex_off32, *info;
    const int32_t *xs, *xe;
    const uint8_t *names; int64_t names_len;
    const uint32_t *id[4];                              // gid, tids, gname, tname (the last two: form READ)
    const int32_t *sel, *start, *end, *cov;             // any may be null
    int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;
    const uint8_t *src; uint32_t src_len; int32_t form;
};

__device__ __forceinline__ void gtx_chain(const GtxIn &in, int64_t t, int64_t &off, int64_t &n)
{
    if (in.ex_off64) { off = in.ex_off64[t]; n = in.ex_off64[t + 1] - off; }
    else { off = (int64_t)in.ex_off32[t]; n = (int64_t)(in.info[t] >> 8); }
}

// the id column of name c (a select, not an indexed read of the kernel's arguments)
__device__ __forceinline__ const uint32_t *gtx_id(const GtxIn &in, int c) { return c == 0 ? in.id[0] : c == 1 ? in.id[1] : c == 2 ? in.id[2] : in.id[3]; }

// words of k_gtx_measure's result
struct GtxMeasure { uint32_t *len, *fix; unsigned long long *bad, *lines; };

template <bool WAVE_FORM>
__global__ __launch_bounds__(256)
void k_gtx_measure(GtxIn in, GtxMeasure out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t q = WAVE_FORM ? g >> 6 : g;
    const int lane = (int)(threadIdx.x & 63u);
    const bool live = q < in.m;
    if (WAVE_FORM && !live) return;                                 // (the whole wave leaves)
    int kind = GTX_OK;
    uint64_t bytes = 0, lines = 0;
    uint32_t fix = 0;
    if (live) {
        const int64_t t = in.sel ? (int64_t)in.sel[q] : q;
        int32_t tid = 0;
        int64_t off = 0, n = 0;
        if (t < 0 || t >= in.n) kind = GTX_E_SEL;
        else {
            tid = in.tid[t];
            if (tid < 0 || tid >= in.n_ref) kind = GTX_E_TID;
            else { gtx_chain(in, t, off, n); if (n < 1) kind = GTX_E_NOEXON; }
        }
        if (!kind) {
            const int n_names = in.form == L2R_GTX_READ ? 4 : 2;
            uint32_t len[4] = {0u, 0u, 0u, 0u};
            if (!WAVE_FORM) {
                for (int c = 0; c < n_names && !kind; ++c) kind = gtx_name_len(in.names, in.names_len, gtx_id(in, c)[t], &len[c]);
            } else {
                // lanes 0..3 take a name each; the first name with an error gives the kind
                uint32_t mine = 0u;
                const int e = lane < n_names ? gtx_name_len(in.names, in.names_len, gtx_id(in, lane)[t], &mine) : GTX_OK;
                const unsigned long long bad = __ballot(e != GTX_OK);
                if (bad) kind = __shfl(e, __ffsll((long long)bad) - 1, 64);
#pragma unroll
                for (int c = 0; c < 4; ++c) len[c] = (uint32_t)__shfl((int)mine, c, 64);
            }
            if (!kind) {
                const int32_t S = in.start ? in.start[q] : in.xs[off], E = in.end ? in.end[q] : in.xe[off + n - 1], cov = in.cov ? in.cov[q] : 1;
                if (S < 0 || E < 0 || cov < 0) kind = GTX_E_NEG;
                else {
                    fix = gtx_line_fix((uint32_t)(in.ref_off[tid + 1] - in.ref_off[tid]), in.src_len, gtx_attr_len(in.form, len));
                    // the exons' digits; the overrides stand for the first start and the last end
                    bool neg = false;
                    uint64_t dig = 0;
                    if (!WAVE_FORM) {
                        for (int64_t j = 0; j < n; ++j) {
                            const int32_t s = j == 0 ? S : in.xs[off + j], x = j == n - 1 ? E : in.xe[off + j];
                            neg |= (s | x) < 0;
                            dig += text_digits((uint32_t)s) + text_digits((uint32_t)x);
                        }
                    } else {
                        uint32_t mine = 0u;                         // (at most 2^25 exons of 20 digits per lane)
                        for (int64_t j = lane; j < n; j += 64) {
                            const int32_t s = j == 0 ? S : in.xs[off + j], x = j == n - 1 ? E : in.xe[off + j];
                            neg |= (s | x) < 0;
                            mine += text_digits((uint32_t)s) + text_digits((uint32_t)x);
                        }
                        dig = (uint64_t)wave_sum(mine & 0xffffu) + ((uint64_t)wave_sum(mine >> 16) << 16);
                        neg = __any(neg) != 0;
                    }
                    bytes = (uint64_t)(n + 1) * fix + gtx_head_extra(in.form, (uint32_t)cov) + text_digits((uint32_t)S) + text_digits((uint32_t)E) + dig;
                    lines = (uint64_t)n + 1u;
                    if (neg) kind = GTX_E_NEG;
                    else if (bytes >= GTX_BATCH_BYTES) kind = GTX_E_BIG;
                }
            }
        }
        if (kind) { bytes = 0; lines = 0; }
    }
    if (WAVE_FORM) {
        if (lane) return;
        atomicAdd(out.lines, (unsigned long long)lines);
    } else {
        // (every lane of the wave is here) the wave's lines in one atomic
        const uint32_t lo = wave_sum((uint32_t)lines & 0xffffu), hi = wave_sum((uint32_t)(lines >> 16));
        if (lane == 0) atomicAdd(out.lines, (unsigned long long)lo + ((unsigned long long)hi << 16));
        if (!live) return;
    }
    if (kind) atomicMin(out.bad, (unsigned long long)q << 4 | (unsigned long long)kind);
    out.len[q] = (uint32_t)bytes; out.fix[q] = fix;
}

// One line at dst (LDS or the text itself): exactly the bytes its length says.  head: the transcript line (then a = S, e = E).
__device__ __forceinline__ void gtx_put_line(uint8_t *dst, const GtxIn &in, int64_t t, bool head, uint32_t a, uint32_t e, uint32_t cov)
{
    const int32_t tid = in.tid[t];
    uint8_t *p = dst;
    for (int64_t k = in.ref_off[tid]; k < in.ref_off[tid + 1]; ++k) *p++ = in.ref_names[k];
    *p++ = '\t';
    for (uint32_t k = 0; k < in.src_len; ++k) *p++ = in.src[k];
    *p++ = '\t';
    p = head ? text_put_lit(p, "transcript\t") : text_put_lit(p, "exon\t");
    p = text_put_num(p, a); *p++ = '\t'; p = text_put_num(p, e);
    p = text_put_lit(p, "\t.\t"); *p++ = in.rev[t] ? '-' : '+'; p = text_put_lit(p, "\t.\t");
    if (in.form == L2R_GTX_PLAIN) {
        p = text_put_lit(p, "gene_id \""); p = text_put_name(p, in.names + in.id[0][t], L2R_GTX_NAME_MAX);
        p = text_put_lit(p, "\"; transcript_id \""); p = text_put_name(p, in.names + in.id[1][t], L2R_GTX_NAME_MAX);
        p = text_put_lit(p, "\";");
    } else {
        bool any = false;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint8_t *s = in.names + in.id[c][t];
            if (!s[0]) continue;
            if (any) *p++ = ' ';
            any = true;
            p = c == 0 ? text_put_lit(p, "gene_id \"") : c == 1 ? text_put_lit(p, "transcript_id \"") : c == 2 ? text_put_lit(p, "gene_name \"") : text_put_lit(p, "transcript_name \"");
            p = text_put_name(p, s, L2R_GTX_NAME_MAX);
            p = text_put_lit(p, "\";");
        }
        // (all four names empty: the blank of <C> then stands behind the tab, as emit_gtf_named writes it; the reference would write none)
        if (head) { p = text_put_lit(p, " transcript_cov \""); p = text_put_num(p, cov); p = text_put_lit(p, "\";"); }
    }
    *p = '\n';
}

// words of k_gtx_write's counters
enum { GTXC_DIRECT = 0, GTXC_LINES, GTXC_OUTSIDE, GTXC_N };

// The blocks [first, first + count) of the selection; off: the scanned lengths of the batch (count + 1 words), fix: of the whole selection.
__global__ __launch_bounds__(GTX_THREADS)
void k_gtx_write(GtxIn in, int64_t first, int64_t count, const uint32_t *__restrict__ off, const uint32_t *__restrict__ fix, uint8_t *__restrict__ text,
                 uint32_t *__restrict__ counters)
{
    __shared__ uint4 s_img[GTX_LDS / 16 + 1];           // the image of the tile's span (l2r_text.hip.h)
    __shared__ uint32_t s_line[GTX_TILE + 1];           // lines in front of the tile's blocks; the tile's lines last
    __shared__ uint32_t s_wave[4];
    const int64_t i0 = (int64_t)blockIdx.x * GTX_TILE, i1 = i0 + GTX_TILE < count ? i0 + GTX_TILE : count;
    const uint32_t nb = (uint32_t)(i1 - i0);
    const uint32_t b0 = off[i0], b1 = off[i1], bytes = b1 - b0;
    const bool direct = bytes > GTX_LDS;                // (workgroup-uniform)
    const uint32_t head = text_head(b0);
    uint32_t n_lines = 0u;
    {   uint32_t nl = 0u;
        if (threadIdx.x < nb) {
            const int64_t q = first + i0 + threadIdx.x, t = in.sel ? (int64_t)in.sel[q] : q;
            int64_t o, n;
            gtx_chain(in, t, o, n);
            nl = (uint32_t)n + 1u;
        }
        const uint32_t ex = block_exclusive_scan(nl, s_wave, n_lines);
        if (threadIdx.x <= GTX_TILE) s_line[threadIdx.x] = ex;      // (lanes from nb on hold the total)
        __syncthreads(); }
    uint32_t run = 0u;                                  // bytes of the rounds before (workgroup-uniform)
    for (uint32_t base = 0u; base < n_lines; base += GTX_THREADS) {
        const uint32_t l = base + threadIdx.x;
        const bool valid = l < n_lines;
        uint32_t len = 0u, a = 0u, e = 0u, cov = 1u;
        int64_t t = 0;
        bool is_head = false;
        if (valid) {
            uint32_t lo = 0u, hi = nb;                  // the last block with s_line[block] <= l
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_line[mid] <= l) lo = mid; else hi = mid; }
            const uint32_t k = l - s_line[lo];
            const int64_t q = first + i0 + lo;
            t = in.sel ? (int64_t)in.sel[q] : q;
            int64_t o, n;
            gtx_chain(in, t, o, n);
            is_head = k == 0u;
            uint32_t extra = 0u;
            if (is_head) {
                a = (uint32_t)(in.start ? in.start[q] : in.xs[o]); e = (uint32_t)(in.end ? in.end[q] : in.xe[o + n - 1]);
                cov = in.cov ? (uint32_t)in.cov[q] : 1u;
                extra = gtx_head_extra(in.form, cov);
            } else {
                int64_t j = (int64_t)k - 1;
                if (in.form == L2R_GTX_READ && in.rev[t]) j = n - 1 - j;
                a = (uint32_t)(j == 0 && in.start ? in.start[q] : in.xs[o + j]);
                e = (uint32_t)(j == n - 1 && in.end ? in.end[q] : in.xe[o + j]);
            }
            len = fix[q] + extra + text_digits(a) + text_digits(e);
        }
        uint32_t round_bytes;
        const uint32_t pos = run + block_exclusive_scan(len, s_wave, round_bytes);
        run += round_bytes;
        if (valid) {
            if ((uint64_t)pos + len > bytes) atomicAdd(counters + GTXC_OUTSIDE, 1u);
            else gtx_put_line(direct ? text + b0 + pos : text_image(s_img, head) + pos, in, t, is_head, a, e, cov);
        }
    }
    if (threadIdx.x == 0) { atomicAdd(counters + GTXC_LINES, n_lines); if (direct) atomicAdd(counters + GTXC_DIRECT, 1u); }
    if (direct) return;
    __syncthreads();
    text_stream_out<GTX_THREADS>(s_img, b0, bytes, text);
}

}  // namespace l2r
