// l2r_masks.hip.h -- the device functions that carry the semantics of a ONE-WINDOW classification (src/update_gtf.c:717-835), one body
// each for both mask widths: M = uint32_t (a window of up to WIN_TX = 32 transcripts: k_classify_fast, k_probe_slab, k_tile) and
// M = m64_t (33 .. WIDE_MEMBERS = 63: k_probe_slab_wide, k_tile<..., WIDE>, l2r_wide.hip.h).  Bit j of a mask = member j of the window.
//     visit_window<LEVEL, M>            the members a read's sweep visits, its terminal-exon masks
//     probe_near                        one probe of a staged slice with a tolerance (-d > 0): one name, a body per width
//     overlapping_exon_members<M>       members with an exon over an interval (full-length evidence)
//     pick_known<M>, decide<LEVEL, M>   the verdict from the masks
//     verdict_info, redo_append         the chunked kernels' info word (l2r_chunk / l2r_tchunk.hip.h; decide has its lines), the redo list
// What depends on the width is a set of plain overloads (first_member, lowest_bit, highest_bit, low_bits; the 32-bit ones keep their
// inline assembly) and the staged entry's type, which has the same field names at either width (WEnt).
// Not a header of its own standing: l2r_kernels.hip.h includes it behind what it uses.
#pragma once

namespace l2r {

typedef unsigned long long m64_t;
struct WEnt { int32_t x, y; m64_t z, w; };                      // staged dictionary entry of a 64-bit window, 24 bytes (two 8-byte key / mask reads); fields named
                                                                // as in the 16-byte vector {k1, k2, pm, sm} of a 32-bit window: one body reads either
template <typename M> struct ent_of { typedef v4i_t type; };
template <> struct ent_of<m64_t> { typedef WEnt type; };

// index of the lowest set bit, 63 when there is none (a window holds members 0 .. 62 at most)
__device__ __forceinline__ uint32_t first_member(uint32_t x)
{
    return (uint32_t)(__ffs((int)x) - 1) & 63u;                         // v_ffbl_b32 (-1 for 0), masked to 63
}
__device__ __forceinline__ uint32_t first_member(m64_t x) { return x ? (uint32_t)(__ffsll((long long)x) - 1) : 63u; }
__device__ __forceinline__ int lowest_bit(uint32_t x) { return __ffs((int)x) - 1; }                  // (x != 0)
__device__ __forceinline__ int lowest_bit(m64_t x) { return __ffsll((long long)x) - 1; }
__device__ __forceinline__ int highest_bit(uint32_t x) { return 31 - __clz((int)x); }
__device__ __forceinline__ int highest_bit(m64_t x) { return 63 - __clzll((long long)x); }
template <typename M> __device__ __forceinline__ M low_bits(int n)                                   // bits 0 .. n - 1; every bit from the width on
{
    return n >= (int)(8 * sizeof(M)) ? (M)~(M)0 : (M)(((M)1 << n) - (M)1);
}

// x != 0 as 0 / 1 in one VALU instruction (the compiler turns min(x, 1) into compare + select + a literal move)
__device__ __forceinline__ uint32_t nonzero(uint32_t x)
{
    uint32_t r;
    asm("v_min_u32 %0, 1, %1" : "=v"(r) : "v"(x));
    return r;
}

// -d > 0 (src/update_gtf.c:717-779 with dis > 0): a read site matches EVERY annotation site within `dis` of it, and identical_site_n
// counts the matching (annotation site, read site) PAIRS.  One probe of a staged slice with a tolerance: entries [lo, hi) are the
// buckets of k1 - dis .. k1 + dis (one or two of them: 2 dis + 1 <= 129 bases with dis <= DIS_MASK_MAX; the range arithmetic of
// near_range would take more -- lo = the first bucket's first entry, hi = the last bucket's end), sorted by (key 1, key 2).  The staged
// directories are bytes: a slice holds at most SLAB_KEY_CAP / KEY_CAP (< 256) entries whatever the tolerance adds to its span.
//   sm |= site members of every entry whose first key lies within dis of k1 AND inside the read's span [rs, re] -- an annotation site
//         counts only inside the overlap span (:732,742); inside the transcript's own span it always is (TX_COMPACT);
//   pm |= pair members of every entry with both keys within dis (the exon / junction flags know no overlap span, :753-768);
//   amb |= members that have TWO different sites within dis of this one read site: for them the pair count is not the number of
//         matched read sites, the masks cannot say whether the read is known -- such a read goes to the generic kernel (it takes a
//         transcript with two donors or two acceptors less than 2 dis + 1 bases apart).
static_assert(2 * DIS_MASK_MAX + 1 <= (1 << SITE_SHIFT) && KEY_CAP < 256, "a tolerance window spans two buckets at most; byte directories");
// Two bodies of the one name: the 32-bit one takes no branch per entry and looks at the first two entries without a loop; that form on
// 24-byte entries costs k_probe_slab_wide three spilled registers more, so the 64-bit one keeps its plain loop with branches.
__device__ __forceinline__ void probe_near(const v4i_t *ent, uint32_t lo, uint32_t hi, int32_t k1, int32_t k2, int dis, int rs, int re,
                                           uint32_t &pm, uint32_t &sm, uint32_t &amb)
{
    pm = 0u; sm = 0u;
    int last = INT32_MIN;
    const uint32_t span = 2u * (uint32_t)dis, b1 = (uint32_t)k1 - (uint32_t)dis, b2 = (uint32_t)k2 - (uint32_t)dis;
    // (no branch per entry: selects; an entry outside the tolerance adds nothing, sorted or not)
    auto one = [&](const v4i_t q, bool on) {
        const bool in = on && (uint32_t)q.x - b1 <= span;
        const bool sp = in && q.x >= rs && q.x <= re;
        const uint32_t w = sp ? (uint32_t)q.w : 0u;
        amb |= q.x != last ? (sm & w) : 0u;
        last = sp ? q.x : last;
        sm |= w;
        pm |= (in && (uint32_t)q.y - b2 <= span) ? (uint32_t)q.z : 0u;
    };
    // the first NEAR_FIRST entries without a loop (most tolerance windows hold no more), the others only where some lane has them
    const v4i_t q0 = lds_entry(ent, lo), q1 = lds_entry(ent, lo + 1u);
    one(q0, lo < hi); one(q1, lo + 1u < hi);
    if (__any(hi > lo + 2u))
        for (uint32_t r = lo + 2u; r < hi; ++r) one(lds_entry(ent, r), true);
}
__device__ __forceinline__ void probe_near(const WEnt *ent, uint32_t lo, uint32_t hi, int32_t k1, int32_t k2, int dis, int rs, int re, m64_t &pm, m64_t &sm, m64_t &amb)
{
    pm = 0ull; sm = 0ull;
    int last = INT32_MIN;
    for (uint32_t r = lo; r < hi; ++r) {
        const WEnt q = ent[r];
        if (q.x > k1 + dis) break;
        if (q.x < k1 - dis) continue;
        if (q.x >= rs && q.x <= re) {
            if (q.x != last) { amb |= sm & q.w; last = q.x; }
            sm |= q.w;
        }
        if (__builtin_abs(q.y - k2) <= dis) pm |= q.z;
    }
}

// Transcripts (tile frame) that have an exon overlapping [s, e]: union of the exon masks of the START entries
// from the first one that reaches into the bucket of s up to the last one that starts in the bucket of e.
// (DirT: byte directories in the one-window kernels, words in the chunked one)
template <typename M, typename DirT>
__device__ __forceinline__ M overlapping_exon_members(const DirT *rdir, const DirT *dir, const typename ent_of<M>::type *ent, int b_off, int nb, int s, int e)
{
    const int bs = s >> SITE_SHIFT;
    if (bs >= nb) return 0;                                  // beyond the last annotated site of the chromosome
    const int be = min(e >> SITE_SHIFT, nb - 1);
    M m = 0;
    const uint32_t i1 = dir[be + b_off + 1];
    for (uint32_t i = rdir[bs + b_off]; i < i1; ++i) {
        const typename ent_of<M>::type q = ent[i];
        if (q.x <= e && q.y >= s) m |= (M)q.z;
    }
    return m;
}

// ---- the three classification phases of a tile (all lanes of a wave call them together) -------------------------

template <typename M>
struct TileLds {                 // the tile's LDS image (layout in the kernels)
    int *S, *E; uint16_t *W;     // exon starts, ends and work words of the tile: k_classify_fast alone (the others keep them in staged positions, SlabStage)
    const typename ent_of<M>::type *ent0, *ent1; const uint8_t *dir0, *dir1, *rdir;
    const int4 *hk, *hx;
    const int *win;              // window member -> annotation index
};
template <typename M> struct VisitMasks { M vpre, lmask, rmask, k1mask; bool redo; };
template <typename M> struct SiteMasks { M kand, kor, dm_first, am_last, amb; };      // amb (-d > 0 only): members with TWO sites within the tolerance of one read site (probe_near)

// V' = window transcripts j >= j0 up to the first one the read lies before (src/update_gtf.c:799-800), minus the ones
// that lie before the read (:801); terminal-exon masks of check_full (:629-681); single-exon known candidates (:806-811).
// One pass over the window with a wave-uniform member index (header words broadcast from LDS) that only BUILDS per-read
// bit masks -- "the read lies before member j", "member j lies before the read", "first / last exons overlap" -- with no
// per-member branch; the sweep's stop (:799) and the cursor (:801-802) are applied to the masks afterwards:
//     V' = ~before & (members below the first "read lies before") & (members from the cursor value on).
// tilemask[0] / [1]: the tile's members with one exon / without TX_COMPACT (set where the headers are staged).
template <int LEVEL, typename M>
__device__ __forceinline__ VisitMasks<M> visit_window(const TileLds<M> &L, const TileDesc &d, int w_n, bool work, uint32_t n, int j0,
                                                      const ReadEnds &re, const M *tilemask)
{
    constexpr M one = 1, none = 0;
    VisitMasks<M> m{none, none, none, none, false};
    // (a wave without a read to classify -- the upper waves of a tile of few reads -- has nothing to visit: the pass below would
    //  still cost it a dozen instructions per member.  The 32-bit kernels only: with this return, the 32-bit spelling of V in pick_known
    //  and of the site flags in decide, k_tile<..., WIDE> measured 1.7 % slower on 40 isoforms per gene -- the 64-bit forms stay.)
    if constexpr (sizeof(M) == 4) { if (!__any(work)) return m; }
    M m_aft = 0, m_bef = 0;
    // (one member's step; a macro, not a lambda: behind a call boundary of any kind the 32-bit kernels come out scheduled differently)
#define L2R_VISIT_MEMBER(j) do { \
        const int4 hk = L.hk[j]; \
        const M bit = one << (j); \
        m_aft |= re.el <= hk.x ? bit : none;                                 /* comp_trans <= (Q5): the read lies before the member */ \
        m_bef |= hk.y <= re.s0 ? bit : none;                                 /* the member lies before the read */ \
        if (LEVEL >= 1 && LEVEL <= 4) { \
            const int4 hx = L.hx[j]; \
            if (LEVEL == 1) { \
                m.lmask |= re.e0 == hx.y ? bit : none; \
                m.rmask |= re.sl == hx.z ? bit : none; \
            } else { \
                m.lmask |= closed_overlap(re.s0, re.e0, hx.x, hx.y) ? bit : none; \
                if (LEVEL != 4) m.rmask |= closed_overlap(re.sl, re.el, hx.z, hx.w) ? bit : none; \
            } \
        } \
    } while (0)
    int jrel0 = j0 - d.j_lo;                       // first member the read's sweep reaches
    // The unroll counts are the 64-bit pass's tuning: without them k_probe_slab_wide spills three registers more (12 bytes of scratch);
    // the 32-bit kernels leave the choice to the compiler.
    if constexpr (sizeof(M) == 8) {
#pragma unroll 4
        for (int j = 0; j < w_n; ++j) L2R_VISIT_MEMBER(j);
        if (!(d.flags & TD_CONTIG)) {
            jrel0 = 0;
#pragma unroll 8
            for (int j = 0; j < w_n; ++j) jrel0 += L.win[j] < j0 ? 1 : 0;
        }
    } else {
        for (int j = 0; j < w_n; ++j) L2R_VISIT_MEMBER(j);
        if (!(d.flags & TD_CONTIG)) {
            jrel0 = 0;
            for (int j = 0; j < w_n; ++j) jrel0 += L.win[j] < j0 ? 1 : 0;
        }
    }
#undef L2R_VISIT_MEMBER
    // members the sweep reaches: index >= jrel0 (which may be negative or beyond the window)
    const M reach = jrel0 <= 0 ? (M)~none : (jrel0 >= (int)(8 * sizeof(M)) ? none : (M)~((one << jrel0) - one));
    const M stop = m_aft & reach;                                            // the sweep ends at the lowest of these (:799-800)
    const M below = (stop & (none - stop)) - one;                            // all ones when there is none
    m.vpre = work ? (~m_bef & below & reach & low_bits<M>(w_n)) : none;
    m.lmask &= m.vpre; m.rmask &= m.vpre;
    // single-exon members only count against single-exon reads (:806-811); a member without TX_COMPACT needs the literal loops
    const M single = tilemask[0];
    if (n == 1) {
        M c = m.vpre & single;
        while (c) {
            const int j = lowest_bit(c);
            c &= c - one;
            const int4 hx = L.hx[j];
            if (overlap_frac(re.s0, re.e0, hx.x, hx.y) >= fast_args()->p.frac) m.k1mask |= one << j;
        }
    } else if (m.vpre & tilemask[1] & ~single) m.redo = true;
    return m;
}

// The first known transcript in visiting order (jstar, -1: none), the visited set V up to it, "a member of V other than jstar has a site
// of the read" and the reference member (jref, -1: none) -- of one window, or of one chunk of a window (l2r_chunk / l2r_tchunk.hip.h).
template <typename M> struct Known { int jstar, jref; M V; bool ksite; };
template <typename M>
__device__ __forceinline__ Known<M> pick_known(const int4 *hk_of, uint32_t n, const ReadEnds &re, M vpre, M k1mask, M kand, M kor)
{
    int jstar = -1;
    if (n > 1) {
        // every probed site is in the transcript; known also needs every read site inside the overlap span:
        // donors e_0..e_{n-2} and acceptors s_1..s_{n-1} increase, so e_0 >= a.start and s_{n-1} <= a.end suffice
        M c = kand & vpre;
        while (c) {
            const int j = lowest_bit(c);
            c &= c - (M)1;
            const int4 hk = hk_of[j];
            if (hk.x <= re.e0 && re.sl <= hk.y) { jstar = j; break; }
        }
    } else if (k1mask) jstar = lowest_bit(k1mask);
    const bool known = jstar >= 0;
    M upto = ((M)2 << (known ? jstar : 0)) - (M)1;                          // (member 31: the shift leaves 0, all ones)
    if constexpr (sizeof(M) == 8) upto = jstar >= 63 ? ~(M)0 : upto;        // (the 64-bit kernels' spelling: see visit_window)
    const M V = known ? (vpre & upto) : vpre;
    const M ks = (n > 1) ? (kor & V) : (M)0;
    const bool ksite = (ks & ~(known ? ((M)1 << jstar) : (M)0)) != (M)0;
    int jref = -1;
    if (n > 1) { if (ks) jref = highest_bit(ks); }
    else jref = jstar;
    return Known<M>{jstar, jref, V, ksite};
}

// The info word of a verdict (count = the read's exon count in its place, n << 8); I_ACCEPT: the routing of update_gtf.c:943-950 when there is no junction table (finish_info)
__device__ __forceinline__ uint32_t verdict_info(int level, uint32_t count, bool known, bool ksite, bool lfull, bool lnoth, bool rfull, bool rnoth, bool out_rev)
{
    uint32_t info = 0;
    if (known) info |= I_KNOWN;
    if (ksite) info |= I_KSITE;
    if (full_decision(level, lfull, lnoth, rfull, rnoth)) info |= I_FULL;
    if (out_rev) info |= I_REV;
    if (fast_args()->p.n_sj == 0 && (info & (I_FULL | I_KNOWN | I_KSITE)) == (I_FULL | I_KSITE)) info |= I_ACCEPT;
    return info | count;
}

// Known / known site / reference transcript / full-length / flag bytes of one read from its masks.
// getw(k) = the work word map_exons left for exon k, emit(k, flag byte) receives the exons' flags (the classic kernel keeps both in its
// 16-bit W array, the slab kernels in the upper bits of their staged positions).
template <int LEVEL, typename M, typename GetW, typename Emit>
__device__ __forceinline__ Verdict decide(const TileLds<M> &L, const TileDesc &d, uint32_t n, const ReadEnds &re,
                                          const VisitMasks<M> &vm, const SiteMasks<M> &sm, bool rev_in, GetW getw, Emit emit)
{
    const Known<M> kn = pick_known(L.hk, n, re, vm.vpre, vm.k1mask, sm.kand, sm.kor);
    const bool known = kn.jstar >= 0;
    const M V = kn.V;
    // ---- full-length evidence (:629-681) over V.  lfull: the first exon of a member of V overlaps the read's first
    // exon.  lnoth stays set unless SOME exon of a member of V overlaps it; that is certain when the read's first donor
    // is a donor of a member (the exon that ends there), else the START slice decides.
    bool lfull = false, rfull = false, lnoth = true, rnoth = true;
    if (LEVEL >= 1 && LEVEL <= 4) { lfull = (vm.lmask & V) != 0; rfull = (vm.rmask & V) != 0; }
    if (LEVEL == 3 || LEVEL == 4) {
        if (!lfull) {
            if (sm.dm_first & V) lnoth = false;
            else if (V) lnoth = (overlapping_exon_members<M>(L.rdir, L.dir0, L.ent0, d.b_off, d.nb, re.s0, re.e0) & V) == 0;
        }
        if (LEVEL == 3 && !rfull) {
            if (sm.am_last & V) rnoth = false;
            else if (V) rnoth = (overlapping_exon_members<M>(L.rdir, L.dir0, L.ent0, d.b_off, d.nb, re.sl, re.el) & V) == 0;
        }
    }
    // ---- flags: an exon / junction is no longer novel iff the first member of V' that has it comes no later than
    // j*; a known read has every probed donor and acceptor in transcript j*
    const uint32_t lim = known ? (uint32_t)kn.jstar : 62u;                     // (63 = no member)
    const uint32_t site_bits = known ? 0u : (uint32_t)(F_DON | F_ACC);         // bits 12, 13 of a work word: the site is in V' (F_DON = 2, F_ACC = 4)
    if (n > 1) {
        for (int k = 0; k < (int)n; ++k) {
            const uint32_t w = getw(k);
            uint32_t f = ((w & 63u) > lim ? (uint32_t)F_EXON : 0u) | (((w >> 6) & 63u) > lim ? (uint32_t)F_JUNC : 0u);
            if constexpr (sizeof(M) == 4) f |= (~w >> 11) & site_bits;
            else if (!known) f |= (((w >> 12) & 1u) ? 0u : (uint32_t)F_DON) | (((w >> 13) & 1u) ? 0u : (uint32_t)F_ACC);      // (the 64-bit kernels' spelling: see visit_window)
            f &= (k + 1 == (int)n) ? (uint32_t)F_EXON : 0xffu;                   // the last exon has no junction behind it
            emit(k, f);
        }
    } else emit(0, (uint32_t)F_EXON);
    int ref = -1;
    bool out_rev = rev_in;
    if (kn.jref >= 0) { ref = L.win[kn.jref]; out_rev = ((L.hk[kn.jref].w >> 8) & 1) != 0; }     // :825-831
    // (verdict_info's lines, written out: as a call k_tile's level-1 instances came out with two more branches)
    uint32_t info = 0;
    if (known) info |= I_KNOWN;
    if (kn.ksite) info |= I_KSITE;
    if (full_decision(LEVEL, lfull, lnoth, rfull, rnoth)) info |= I_FULL;
    if (out_rev) info |= I_REV;
    if (fast_args()->p.n_sj == 0 && (info & (I_FULL | I_KNOWN | I_KSITE)) == (I_FULL | I_KSITE)) info |= I_ACCEPT;
    return Verdict{info | (n << 8), ref};
}

// The reads of a wave that the generic kernel takes, appended to the redo list: one atomic per wave, a read's place by its rank among
// the wave's.  Returns the wave's ballot.  (The list's two addresses are read from the argument block HERE, behind the ballot: handed in
// as arguments they were fetched ahead of it, in one load with their neighbours -- other instructions in every 32-bit kernel.)
__device__ __forceinline__ unsigned long long redo_append(FastArgsK f, bool redo, uint32_t r)
{
    const unsigned long long m = __ballot(redo);
    if (m) {
        const int lane = threadIdx.x & (WAVE - 1);
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(f->redo_count, (uint32_t)__popcll(m));
        at = __shfl(at, 0, WAVE);
        if (redo) f->redo[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = r;
    }
    return m;
}

}  // namespace l2r
