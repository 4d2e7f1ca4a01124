// l2r_text.hip.h -- what composing text on the device needs, for the write kernels of l2r_bed.hip.h, l2r_gtftext.hip.h and l2r_detail.hip.h: decimal
// digits, literals, names, and the way a tile's text leaves the workgroup.
//
// The LDS image and the stream-out.  A workgroup's text is one contiguous span [b0, b0 + bytes) of the output.  Its lines are composed in
// an LDS image that starts at the span's 16-byte boundary: `head` = b0 & 15 unused bytes, then the text (text_head, text_image), so that image and
// output agree modulo 16 and the image needs 16 bytes more than the text it holds.  Behind a __syncthreads() the workgroup streams the
// image out (text_stream_out): every 16-byte chunk that lies wholly inside the span in one aligned store, the span's head and tail --
// the chunks it shares with the neighbouring tiles or with nothing -- byte by byte.  Nothing outside [b0, b0 + bytes) is written.
// Plain stores throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace l2r {

__device__ __forceinline__ uint32_t text_digits(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
// (a number beyond 32 bits belongs to an item whose text is an error: any count will do)
__device__ __forceinline__ uint32_t text_digits64(uint64_t v) { return v > 0xffffffffull ? 10u : text_digits((uint32_t)v); }

// the decimal digits of v at p; returns the byte behind them
__device__ __forceinline__ uint8_t *text_put_num(uint8_t *p, uint32_t v)
{
    const uint32_t d = text_digits(v);
    uint8_t *q = p + d;
    do { *--q = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
    return p + d;
}

// s[0 .. N) at p; returns the byte behind them
template <int N> __device__ __forceinline__ uint8_t *text_put_lit(uint8_t *p, const char (&s)[N])
{
#pragma unroll
    for (int k = 0; k < N - 1; ++k) p[k] = (uint8_t)s[k];
    return p + (N - 1);
}

// The name at s up to its NUL, max_len bytes at the most (its measure kernel has found a NUL within them), at p; returns the byte behind
// the name.  With `end`, a byte at or beyond it is not written -- the name still counts in full.
__device__ __forceinline__ uint8_t *text_put_name(uint8_t *p, const uint8_t *__restrict__ s, int max_len, const uint8_t *end = nullptr)
{
    for (int k = 0; k <= max_len; ++k) { const uint8_t c = s[k]; if (!c) break; if (!end || p < end) *p = c; ++p; }
    return p;
}

// the unused bytes in front of the text in the image of the span that begins at b0, and where the span's first byte stands in the image
__device__ __forceinline__ uint32_t text_head(uint32_t b0) { return b0 & 15u; }
__device__ __forceinline__ uint8_t *text_image(uint4 *s_img, uint32_t head) { return reinterpret_cast<uint8_t *>(s_img) + head; }

// The image of the span [b0, b0 + bytes) to the text, by the THREADS lanes of the workgroup (behind the __syncthreads() that completes it)
template <int THREADS>
__device__ __forceinline__ void text_stream_out(const uint4 *s_img, uint32_t b0, uint32_t bytes, uint8_t *text)
{
    const uint32_t head = text_head(b0);
    const uint8_t *img = reinterpret_cast<const uint8_t *>(s_img);
    uint8_t *g = text + (b0 - head);                    // 16-byte aligned (the text buffer is)
    const uint32_t img_end = head + bytes, n_chunk = (img_end + 15u) / 16u;
    for (uint32_t c = threadIdx.x; c < n_chunk; c += THREADS) {
        const uint32_t lo = c * 16u, hi = lo + 16u;
        if (lo >= head && hi <= img_end) *reinterpret_cast<uint4 *>(g + lo) = s_img[c];
        else for (uint32_t b = lo < head ? head : lo; b < (hi < img_end ? hi : img_end); ++b) g[b] = img[b];
    }
}

}  // namespace l2r
