// l2r_readlist.hip.h -- the kernels of the read lists of `update-gtf -a / -k / -v / -u` (l2r_gtftext_reads / _list, include/lr2rmats_hip.h):
// classified reads as GTF blocks of form L2R_GTX_READ, selected by class on the device.
//
//   k_rl_count            one thread per read: the blocks it brings to the list -- 0, 1, or the pieces of a split candidate, whose flags
//                         are then walked (rl_pieces); no other read's flags are read
//   (k_scan_u32 over the counts: where a read's blocks stand in the selection, and the blocks' count)
//   k_rl_take             one thread per read: (read, first exon, exon count, piece or -1) of its blocks, in read order
//   k_rl_measure<false>   one thread per block: its domain error, or the exact bytes of its text, its lines, `fix` (the bytes of one of
//                         its exon lines without the two numbers) and `hfix` (the same of its transcript line: a piece's stands on
//                         reference 0, so the two differ by more than a constant)
//   k_rl_measure<true>    one wave per block: lanes 0..3 take a name each, lane l the exons l, l + 64, ...
//   k_rl_write            k_gtx_write (l2r_gtftext.hip.h) over this row source: one workgroup of 256 lanes per L2R_GTX_TILE consecutive
//                         blocks, the tile's LINES spread over the lanes, composed in the LDS image of the tile's span and streamed out;
//                         a span beyond L2R_GTX_LDS_BYTES is written line by line straight to the text.
//
// The row source resolves on the device what form READ's rows brought as columns: the strand from info, g / G from ref_tx through the
// annotation's gene tables (`NA` where ref_tx < 0), t / T from the reads' table, the chain from the run's 32-bit offsets (or an uploaded
// result in the same layout) and the block's sub-range of it.  The rule, the order of the domain errors and the length pieces are in
// l2r_readlistplan.hip.h.  A line that would leave its tile's span (measure and write disagreeing: a bug) is not written and counted
// instead (GTXC_OUTSIDE).  Plain stores throughout; wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lr2rmats_hip.h"
#include "l2r_gtftext.hip.h"
#include "l2r_readlistplan.hip.h"

namespace l2r {

struct RlIn {
    int64_t n, m;                                       // reads; blocks of the selection
    const int32_t *tid;
    const uint32_t *ex_off, *info;                      // the run's, or an uploaded result's in the same layout
    const int32_t *xs, *xe, *ref_tx; const uint8_t *f;
    const uint8_t *names; int64_t names_len;            // the reads' table
    const uint32_t *qname, *tid_name;                   // (tid_name == qname where none was given)
    int64_t n_tx, anno_len; const uint8_t *anno; const uint32_t *tx_gid, *tx_gname;
    const int32_t *b_read, *b_first, *b_count, *b_piece;
    int32_t n_ref; const int64_t *ref_off; const uint8_t *ref_names;
    const uint8_t *src; uint32_t src_len;
    int32_t list, has_sj, split;
};

__global__ __launch_bounds__(256)
void k_rl_count(RlIn in, uint32_t *__restrict__ cnt, uint32_t *__restrict__ pieces)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.n) return;
    const uint32_t info = in.info[i];
    const int mode = rl_mode(in.list, info, in.has_sj != 0, in.split != 0);
    uint32_t c = mode == RL_WHOLE ? 1u : 0u;
    if (mode == RL_PIECES) {                                        // (a few reads of the novel list)
        c = rl_pieces(in.f + in.ex_off[i], (int64_t)(info >> 8), [](uint32_t, int64_t, int64_t) {});
        if (c) atomicAdd(pieces, c);
    }
    cnt[i] = c;
}

// at: the scanned counts (n + 1 words); the columns have at[n] entries
__global__ __launch_bounds__(256)
void k_rl_take(RlIn in, const uint32_t *__restrict__ at, int32_t *__restrict__ b_read, int32_t *__restrict__ b_first, int32_t *__restrict__ b_count,
               int32_t *__restrict__ b_piece)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.n) return;
    const uint32_t q0 = at[i], q1 = at[i + 1];
    if (q0 == q1) return;
    const uint32_t info = in.info[i];
    const int64_t n = (int64_t)(info >> 8);
    if (rl_mode(in.list, info, in.has_sj != 0, in.split != 0) == RL_WHOLE) { b_read[q0] = (int32_t)i; b_first[q0] = 0; b_count[q0] = (int32_t)n; b_piece[q0] = -1; return; }
    rl_pieces(in.f + in.ex_off[i], n, [&](uint32_t k, int64_t first, int64_t last) {
        const uint32_t q = q0 + k;
        if (q >= q1) return;                                        // (the count's walk saw the same flags)
        b_read[q] = (int32_t)i; b_first[q] = (int32_t)first; b_count[q] = (int32_t)(last - first + 1); b_piece[q] = (int32_t)k;
    });
}

// Name c (0 g, 1 t, 2 G, 3 T) of read i with the annotation transcript ref: where it stands, or null for `NA`; *table_len its table's bytes
__device__ __forceinline__ const uint8_t *rl_name_table(const RlIn &in, int c, int32_t ref, int64_t i, uint32_t *id, int64_t *table_len)
{
    const bool gene = c == 0 || c == 2;
    if (gene && ref < 0) return nullptr;
    *id = c == 0 ? in.tx_gid[ref] : c == 2 ? in.tx_gname[ref] : c == 1 ? in.tid_name[i] : in.qname[i];
    *table_len = gene ? in.anno_len : in.names_len;
    return gene ? in.anno : in.names;
}
__device__ __forceinline__ int rl_name_len(const RlIn &in, int c, int32_t ref, int64_t i, uint32_t *len)
{
    uint32_t id = 0; int64_t table_len = 0;
    const uint8_t *table = rl_name_table(in, c, ref, i, &id, &table_len);
    if (!table) { *len = rl_na_len(); return RL_OK; }
    const int e = gtx_name_len(table, table_len, id, len);
    return e == GTX_OK ? RL_OK : e == GTX_E_NAME_ID ? RL_E_NAME_ID : e == GTX_E_NAME_LONG ? RL_E_NAME_LONG : RL_E_NAME_NUL;
}

// words of k_rl_measure's result
struct RlMeasure { uint32_t *len, *fix, *hfix; unsigned long long *bad, *lines; };

template <bool WAVE_FORM>
__global__ __launch_bounds__(256)
void k_rl_measure(RlIn in, RlMeasure out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t q = WAVE_FORM ? g >> 6 : g;
    const int lane = (int)(threadIdx.x & 63u);
    const bool live = q < in.m;
    if (WAVE_FORM && !live) return;                                 // (the whole wave leaves)
    int kind = RL_OK;
    uint64_t bytes = 0, lines = 0;
    uint32_t fix = 0, hfix = 0;
    if (live) {
        const int64_t i = in.b_read[q], n = in.b_count[q];
        const int32_t piece = in.b_piece[q];
        const int32_t tid = in.tid[i];
        if (tid < 0 || tid >= in.n_ref) kind = RL_E_TID;
        else if (n < 1) kind = RL_E_NOEXON;
        const int32_t ref = in.ref_tx[i];
        if (!kind && ref >= 0 && (int64_t)ref >= in.n_tx) kind = RL_E_REF;
        if (!kind) {
            uint32_t len[4] = {0u, 0u, 0u, 0u};
            if (!WAVE_FORM) {
                for (int c = 0; c < 4 && !kind; ++c) kind = rl_name_len(in, c, ref, i, &len[c]);
            } else {
                uint32_t mine = 0u;
                const int e = lane < 4 ? rl_name_len(in, lane, ref, i, &mine) : RL_OK;
                const unsigned long long bad = __ballot(e != RL_OK);
                if (bad) kind = __shfl(e, __ffsll((long long)bad) - 1, 64);
#pragma unroll
                for (int c = 0; c < 4; ++c) len[c] = (uint32_t)__shfl((int)mine, c, 64);
            }
            const uint32_t sfx = rl_suffix_len(piece);
            if (!kind && piece >= 0 && (len[1] + sfx >= L2R_GTX_PIECE_NAME_MAX || len[3] + sfx >= L2R_GTX_PIECE_NAME_MAX)) kind = RL_E_PIECE_NAME;
            if (!kind) {
                len[1] += sfx; len[3] += sfx;
                const uint32_t attr = gtx_attr_len(L2R_GTX_READ, len);
                const uint32_t ref_len = (uint32_t)(in.ref_off[tid + 1] - in.ref_off[tid]), head_ref_len = piece < 0 ? ref_len : (uint32_t)(in.ref_off[1] - in.ref_off[0]);
                fix = gtx_line_fix(ref_len, in.src_len, attr);
                hfix = gtx_line_fix(head_ref_len, in.src_len, attr) + gtx_head_extra(L2R_GTX_READ, 1u);
                const int64_t off = (int64_t)in.ex_off[i] + in.b_first[q];
                bool neg = false;
                uint64_t dig = 0;
                if (!WAVE_FORM) {
                    for (int64_t j = 0; j < n; ++j) {
                        const int32_t s = in.xs[off + j], x = in.xe[off + j];
                        neg |= (s | x) < 0;
                        dig += text_digits((uint32_t)s) + text_digits((uint32_t)x);
                    }
                } else {
                    uint32_t mine = 0u;                             // (at most 2^18 exons of 20 digits per lane)
                    for (int64_t j = lane; j < n; j += 64) {
                        const int32_t s = in.xs[off + j], x = in.xe[off + j];
                        neg |= (s | x) < 0;
                        mine += text_digits((uint32_t)s) + text_digits((uint32_t)x);
                    }
                    dig = (uint64_t)wave_sum(mine & 0xffffu) + ((uint64_t)wave_sum(mine >> 16) << 16);
                    neg = __any(neg) != 0;
                }
                const uint32_t head_dig = piece < 0 ? text_digits((uint32_t)in.xs[off]) + text_digits((uint32_t)in.xe[off + n - 1]) : 2u;
                bytes = (uint64_t)n * fix + hfix + head_dig + dig;
                lines = (uint64_t)n + 1u;
                if (neg) kind = RL_E_NEG;
                else if (bytes >= GTX_BATCH_BYTES) kind = RL_E_BIG;
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
    out.len[q] = (uint32_t)bytes; out.fix[q] = fix; out.hfix[q] = hfix;
}

// One line of block (read i, piece) at dst (LDS or the text itself): exactly the bytes its length says.  head: the transcript line.
__device__ __forceinline__ void rl_put_line(uint8_t *dst, const RlIn &in, int64_t i, int32_t piece, bool head, uint32_t a, uint32_t e)
{
    const int32_t tid = head && piece >= 0 ? 0 : in.tid[i];
    const bool rev = !(head && piece >= 0) && (in.info[i] & L2R_INFO_REV);
    const int32_t ref = in.ref_tx[i];
    uint8_t *p = dst;
    for (int64_t k = in.ref_off[tid]; k < in.ref_off[tid + 1]; ++k) *p++ = in.ref_names[k];
    *p++ = '\t';
    for (uint32_t k = 0; k < in.src_len; ++k) *p++ = in.src[k];
    *p++ = '\t';
    p = head ? text_put_lit(p, "transcript\t") : text_put_lit(p, "exon\t");
    p = text_put_num(p, a); *p++ = '\t'; p = text_put_num(p, e);
    p = text_put_lit(p, "\t.\t"); *p++ = rev ? '-' : '+'; p = text_put_lit(p, "\t.\t");
    bool any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t id = 0; int64_t table_len = 0;
        const uint8_t *table = rl_name_table(in, c, ref, i, &id, &table_len);
        const bool sfx = piece >= 0 && (c == 1 || c == 3);
        if (table && !table[id] && !sfx) continue;
        if (any) *p++ = ' ';
        any = true;
        p = c == 0 ? text_put_lit(p, "gene_id \"") : c == 1 ? text_put_lit(p, "transcript_id \"") : c == 2 ? text_put_lit(p, "gene_name \"") : text_put_lit(p, "transcript_name \"");
        if (table) p = text_put_name(p, table + id, L2R_GTX_NAME_MAX); else p = text_put_lit(p, "NA");
        if (sfx) { p = text_put_lit(p, ".split."); p = text_put_num(p, (uint32_t)piece); }
        p = text_put_lit(p, "\";");
    }
    if (head) p = text_put_lit(p, " transcript_cov \"1\";");
    *p = '\n';
}

// The blocks [first, first + count) of the selection; off: the scanned lengths of the batch (count + 1 words), fix / hfix: of the whole
// selection.  counters: GTXC_* of l2r_gtftext.hip.h.
__global__ __launch_bounds__(GTX_THREADS)
void k_rl_write(RlIn in, int64_t first, int64_t count, const uint32_t *__restrict__ off, const uint32_t *__restrict__ fix, const uint32_t *__restrict__ hfix,
                uint8_t *__restrict__ text, uint32_t *__restrict__ counters)
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
    {   const uint32_t nl = threadIdx.x < nb ? (uint32_t)in.b_count[first + i0 + threadIdx.x] + 1u : 0u;
        const uint32_t ex = block_exclusive_scan(nl, s_wave, n_lines);
        if (threadIdx.x <= GTX_TILE) s_line[threadIdx.x] = ex;      // (lanes from nb on hold the total)
        __syncthreads(); }
    uint32_t run = 0u;                                  // bytes of the rounds before (workgroup-uniform)
    for (uint32_t base = 0u; base < n_lines; base += GTX_THREADS) {
        const uint32_t l = base + threadIdx.x;
        const bool valid = l < n_lines;
        uint32_t len = 0u, a = 0u, e = 0u;
        int64_t i = 0;
        int32_t piece = -1;
        bool is_head = false;
        if (valid) {
            uint32_t lo = 0u, hi = nb;                  // the last block with s_line[block] <= l
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (s_line[mid] <= l) lo = mid; else hi = mid; }
            const uint32_t k = l - s_line[lo];
            const int64_t q = first + i0 + lo;
            i = in.b_read[q]; piece = in.b_piece[q];
            const int64_t n = in.b_count[q], o = (int64_t)in.ex_off[i] + in.b_first[q];
            is_head = k == 0u;
            if (is_head) {
                if (piece < 0) { a = (uint32_t)in.xs[o]; e = (uint32_t)in.xe[o + n - 1]; }
                len = hfix[q] + text_digits(a) + text_digits(e);
            } else {
                int64_t j = (int64_t)k - 1;
                if (piece < 0 && (in.info[i] & L2R_INFO_REV)) j = n - 1 - j;
                a = (uint32_t)in.xs[o + j]; e = (uint32_t)in.xe[o + j];
                len = fix[q] + text_digits(a) + text_digits(e);
            }
        }
        uint32_t round_bytes;
        const uint32_t pos = run + block_exclusive_scan(len, s_wave, round_bytes);
        run += round_bytes;
        if (valid) {
            if ((uint64_t)pos + len > bytes) atomicAdd(counters + GTXC_OUTSIDE, 1u);
            else rl_put_line(direct ? text + b0 + pos : text_image(s_img, head) + pos, in, i, piece, is_head, a, e);
        }
    }
    if (threadIdx.x == 0) { atomicAdd(counters + GTXC_LINES, n_lines); if (direct) atomicAdd(counters + GTXC_DIRECT, 1u); }
    if (direct) return;
    __syncthreads();
    text_stream_out<GTX_THREADS>(s_img, b0, bytes, text);
}

}  // namespace l2r
