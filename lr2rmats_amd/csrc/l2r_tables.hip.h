// l2r_tables.hip.h -- the tables of an annotation and of a junction table: everything l2r_set_annotation and l2r_set_junctions
// (l2r_engine.hip) derive on the host from the caller's arrays, the annotation tables' cache file, and the host side of the two sequential
// cursors.  The kernels trust these arrays as they trust the upload's plan (l2r_plan.hip.h): site dictionaries with their parts and SE_WIDE,
// bucket and reach-back directories, cursor keys and their directory, TX_MONO / TX_COMPACT, the junction directories are decided here alone.
// Host arithmetic and file I/O only: no HIP call, no context, no environment.  The engine stages what the tables hold; tests/tables_dump.hip
// writes them out for tests/test_tables_cpu.py.  Included behind the kernel headers (TxHdr, SiteEnt, SITE_SHIFT, TX_*, SE_WIDE).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lr2rmats_hip.h"

namespace l2r {
static int tables_fail(std::string &msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return -1;
}

static inline int64_t host_key(int32_t tid, int32_t x) { return ((int64_t)(tid + 1) << 32) | (uint32_t)x; }

// ---- site dictionaries -------------------------------------------------------------------------
// A site of a kind with the transcript (file order) that has it.  Sorting by (tid, k1, k2, tx) groups the
// members of every distinct site.
struct SiteTx {
    int32_t tid, k1, k2, tx;
    bool operator<(const SiteTx &o) const
    {
        if (tid != o.tid) return tid < o.tid;
        if (k1 != o.k1) return k1 < o.k1;
        if (k2 != o.k2) return k2 < o.k2;
        return tx < o.tx;
    }
};

// Everything l2r_set_annotation derives from the annotation, on the host: what is uploaded, and what the cache file holds.
struct AnnoTables {
    std::vector<TxHdr> hdr;
    std::vector<int64_t> key, key_raw;                 // cursor keys: prefix maximum / per transcript
    std::vector<int2> ex;
    std::vector<SiteEnt> st_ent, en_ent;               // START / END dictionaries
    std::vector<uint32_t> st_dir, st_rdir, en_dir;     // their bucket directories (START: + reach-back directory)
    std::vector<int32_t> tid_base, kb_base;
    std::vector<uint32_t> key_dir;
    int64_t n_wide = 0, n_compact = 0;
    int32_t n_tid_dir = 0, n_tid_key = 0;
};

// Entries of one dictionary + its bucket directory.  `pairs`: sorted (tid, k1, k2, tx) rows of the pair kind
// (exons for START, junctions for END); `singles`: sorted (tid, k1, 0, tx) rows of the single kind (acceptors /
// donors).  An entry's masks are relative to its tx_base and say 64 transcripts; a key whose members (of either kind) lie further
// apart gets SEVERAL entries in a row -- parts, same (k1, k2), rising tx_base, each flagged SE_WIDE: the 32- and 64-bit mask kernels
// leave a tile with such an entry to k_probe_slab_chunked (slab pipeline; it ORs the parts) or to the generic kernel (classic).
static void build_dict(const std::vector<SiteTx> &pairs, const std::vector<SiteTx> &singles, const std::vector<int32_t> &tid_base,
                       std::vector<SiteEnt> &ent, std::vector<uint32_t> &dir, std::vector<uint32_t> *rdir_out, int64_t &n_wide)
{
    const size_t nb = (size_t)tid_base.back();
    dir.assign(nb + 1, 0);                                // dir[b] = number of entries whose bucket id is < b
    ent.clear();
    ent.reserve(pairs.size());
    std::vector<uint32_t> parts;                          // entries per distinct pair (reach-back directory below)
    parts.reserve(pairs.size());
    size_t si = 0;                                        // walks `singles` in step (both sorted by (tid, k1))
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i;
        while (j < pairs.size() && pairs[j].tid == pairs[i].tid && pairs[j].k1 == pairs[i].k1 && pairs[j].k2 == pairs[i].k2) ++j;
        // members of the single kind with the same (tid, k1)
        while (si < singles.size() && (singles[si].tid < pairs[i].tid || (singles[si].tid == pairs[i].tid && singles[si].k1 < pairs[i].k1))) ++si;
        size_t sj = si;
        while (sj < singles.size() && singles[sj].tid == pairs[i].tid && singles[sj].k1 == pairs[i].k1) ++sj;
        const size_t first_ent = ent.size();
        size_t pk = i, sk = si;                            // (members of both kinds rise with tx)
        while (pk < j || sk < sj) {
            int32_t lo = INT32_MAX;
            if (pk < j) lo = std::min(lo, pairs[pk].tx);
            if (sk < sj) lo = std::min(lo, singles[sk].tx);
            SiteEnt e;
            memset(&e, 0, sizeof e);
            e.k1 = pairs[i].k1; e.k2 = pairs[i].k2; e.tx_base = lo;
            for (; pk < j && (int64_t)pairs[pk].tx - lo < 64; ++pk) { const int off = pairs[pk].tx - lo; e.pm[off >> 5] |= 1u << (off & 31); }
            for (; sk < sj && (int64_t)singles[sk].tx - lo < 64; ++sk) { const int off = singles[sk].tx - lo; e.sm[off >> 5] |= 1u << (off & 31); }
            ent.push_back(e);
        }
        const uint32_t np = (uint32_t)(ent.size() - first_ent);
        if (np > 1) { for (size_t q = first_ent; q < ent.size(); ++q) ent[q].flags |= SE_WIDE; ++n_wide; }
        parts.push_back(np);
        const size_t b = (size_t)tid_base[(size_t)pairs[i].tid] + (size_t)(pairs[i].k1 >> SITE_SHIFT);
        dir[b + 1] += np;
        i = j;                                             // `si` stays: the next pair may share (tid, k1)
    }
    for (size_t b = 0; b < nb; ++b) dir[b + 1] += dir[b];
    if (rdir_out) {
        // reach-back directory (START: k1 = exon start, k2 = exon end): first entry whose exon reaches into the bucket
        std::vector<uint32_t> &rdir = *rdir_out;
        rdir = dir;
        size_t i = 0, u = 0;
        for (size_t q = 0; q < pairs.size(); ++u) {       // entries [i, i + parts[u]) <-> the u-th distinct pair
            size_t j = q;
            while (j < pairs.size() && pairs[j].tid == pairs[q].tid && pairs[j].k1 == pairs[q].k1 && pairs[j].k2 == pairs[q].k2) ++j;
            const size_t t0 = (size_t)tid_base[(size_t)pairs[q].tid], nbt = (size_t)tid_base[(size_t)pairs[q].tid + 1] - t0;
            const size_t sb = (size_t)(pairs[q].k1 >> SITE_SHIFT);
            size_t eb = pairs[q].k2 < 0 ? sb : (size_t)(pairs[q].k2 >> SITE_SHIFT);
            if (eb >= nbt) eb = nbt - 1;
            for (size_t b = sb + 1; b <= eb; ++b) if (rdir[t0 + b] > (uint32_t)i) rdir[t0 + b] = (uint32_t)i;
            i += parts[u]; q = j;
        }
    }
}

// Directory over non-decreasing 64-bit keys host_key(tid, x): dir[base[tid] + c] = first j with key_j >= (tid, c << 9), one closing word
// (first j with key_j >= (n_tid, 0)); mx[tid] = the largest x of the chromosome (-1: none, no buckets).  Used for the annotation cursor,
// the junction cursor and the junction table's donors (cursor_value / sj_first_row in l2r_kernels.hip.h).
static int build_key_dir(const int64_t *key, int64_t n, int32_t n_tid, const std::vector<int64_t> &mx, std::vector<int32_t> &base, std::vector<uint32_t> &dir)
{
    base.assign((size_t)n_tid + 1, 0);
    int64_t acc = 0;
    for (int32_t t = 0; t < n_tid; ++t) { base[(size_t)t] = (int32_t)acc; acc += mx[(size_t)t] < 0 ? 0 : (mx[(size_t)t] >> SITE_SHIFT) + 1; }
    if (acc > 0x7ffffff0LL) return -1;
    base[(size_t)n_tid] = (int32_t)acc;
    dir.assign((size_t)acc + 1, 0);
    size_t j = 0;
    for (int32_t t = 0; t < n_tid; ++t) {
        const int32_t nbk = base[(size_t)t + 1] - base[(size_t)t];
        for (int32_t cb = 0; cb < nbk; ++cb) {
            const int64_t q = host_key(t, cb << SITE_SHIFT);
            while (j < (size_t)n && key[j] < q) ++j;
            dir[(size_t)base[(size_t)t] + (size_t)cb] = (uint32_t)j;
        }
    }
    {   // closing word: first j with key >= (n_tid, 0)
        const int64_t q = host_key(n_tid, 0);
        while (j < (size_t)n && key[j] < q) ++j;
        dir[(size_t)acc] = (uint32_t)j;
    }
    // (words of chromosomes without buckets: they share the next chromosome's first word)
    return 0;
}

static int build_tables(const l2r_annotation *a, AnnoTables &o, std::string &msg)
{
    const int64_t T = a->n_tx;
    std::vector<TxHdr> &h = o.hdr;
    std::vector<int64_t> &key = o.key;
    h.assign((size_t)T, TxHdr());
    key.assign((size_t)T, 0);
    o.key_raw.assign((size_t)T, 0);
    int64_t run = INT64_MIN;
    // headers, cursor keys, and the (site, transcript) rows of every kind
    std::vector<SiteTx> kd, ka, kx, kj;
    kd.reserve((size_t)a->n_exon); ka.reserve((size_t)a->n_exon); kx.reserve((size_t)a->n_exon); kj.reserve((size_t)a->n_exon);
    int64_t n_compact = 0;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t lo = a->tx_ex_off[i], hi = a->tx_ex_off[i + 1];
        if (lo < 0 || hi < lo || hi > a->n_exon) return tables_fail(msg, "[l2r_set_annotation] bad exon offsets at transcript %lld", (long long)i);
        if (hi == lo) return tables_fail(msg, "[l2r_set_annotation] transcript %lld has no exon", (long long)i);
        TxHdr &t = h[(size_t)i];
        memset(&t, 0, sizeof t);
        t.tid = a->tx_tid[i]; t.start = a->tx_start[i]; t.end = a->tx_end[i]; t.ex_off = (int32_t)lo;
        t.n = (int32_t)(hi - lo); t.rev = a->tx_rev[i] ? 1 : 0;
        t.s0 = a->ex_start[lo]; t.e0 = a->ex_end[lo]; t.sl = a->ex_start[hi - 1]; t.el = a->ex_end[hi - 1];
        bool mono = true, sane = a->ex_start[lo] <= a->ex_end[lo];
        for (int64_t k = lo + 1; k < hi; ++k) {
            if (!(a->ex_start[k] > a->ex_start[k - 1] && a->ex_end[k] > a->ex_end[k - 1])) mono = false;
            if (a->ex_start[k] > a->ex_end[k]) sane = false;
        }
        int flags = mono ? TX_MONO : 0;
        // the "equal value => inside both spans" argument of the fast kernel holds for these
        if (mono && sane && t.tid >= 0 && t.n >= 2 && t.start == t.s0 && t.end == t.el) { flags |= TX_COMPACT; ++n_compact; }
        t.flags = flags;
        if (t.tid >= 0 && t.n >= 2) for (int64_t k = lo; k < hi; ++k) {
            if (a->ex_start[k] < 0 || a->ex_end[k] < 0) return tables_fail(msg, "[l2r_set_annotation] negative exon coordinate");
            kx.push_back(SiteTx{t.tid, a->ex_start[k], a->ex_end[k], (int32_t)i});
            if (k + 1 < hi) { kd.push_back(SiteTx{t.tid, a->ex_end[k], 0, (int32_t)i}); kj.push_back(SiteTx{t.tid, a->ex_end[k], a->ex_start[k + 1], (int32_t)i}); }
            if (k > lo) ka.push_back(SiteTx{t.tid, a->ex_start[k], 0, (int32_t)i});
        }
        // "annotation before read": tid smaller, or same tid and end <= read start (update_gtf.c:786-790).
        // The sequential cursor equals the longest prefix that is entirely before the read = first index
        // whose running maximum of (tid,end) exceeds (read.tid, read.start)  (SURVEY.md 3.3).
        const int64_t k = host_key(t.tid, t.end);
        o.key_raw[(size_t)i] = k;
        if (k > run) run = k;
        key[(size_t)i] = run;
    }
    {   // the four row sets are independent: one thread each
        std::thread t1([&] { std::sort(kd.begin(), kd.end()); }), t2([&] { std::sort(ka.begin(), ka.end()); }), t3([&] { std::sort(kx.begin(), kx.end()); });
        std::sort(kj.begin(), kj.end());
        t1.join(); t2.join(); t3.join();
    }
    o.n_compact = n_compact;
    {   // one bucket grid for the four kinds: per tid, enough 512-bp buckets for its largest site coordinate
        int32_t n_tid = 0;
        for (const auto *v : {&kd, &ka, &kx, &kj}) if (!v->empty()) n_tid = std::max(n_tid, v->back().tid + 1);
        std::vector<int64_t> mx((size_t)n_tid, -1);
        for (const auto *v : {&kd, &ka, &kx, &kj}) for (const SiteTx &k : *v) mx[(size_t)k.tid] = std::max<int64_t>(mx[(size_t)k.tid], k.k1);
        // ... and for the last exon END of every chromosome: the full-length evidence looks for exons that reach into
        // the bucket of a read's terminal exon (rdir), so the grid has to cover exon ends, not only the probe keys
        for (const SiteTx &k : kx) mx[(size_t)k.tid] = std::max<int64_t>(mx[(size_t)k.tid], k.k2);
        std::vector<int32_t> &tb = o.tid_base;
        tb.assign((size_t)n_tid + 1, 0);
        int64_t acc = 0;
        for (int32_t t = 0; t < n_tid; ++t) { tb[(size_t)t] = (int32_t)acc; acc += mx[(size_t)t] < 0 ? 0 : (mx[(size_t)t] >> SITE_SHIFT) + 1; }
        if (acc > 0x7ffffff0LL) return tables_fail(msg, "[l2r_set_annotation] site directory too large");
        tb[(size_t)n_tid] = (int32_t)acc;
        // START: exons + the transcripts in which their start is an acceptor; END: junctions + donors
        o.n_wide = 0;
        build_dict(kx, ka, tb, o.st_ent, o.st_dir, &o.st_rdir, o.n_wide);
        build_dict(kj, kd, tb, o.en_ent, o.en_dir, nullptr, o.n_wide);
        o.n_tid_dir = n_tid;
    }
    {   // cursor directory over the prefix-max keys: dir[kb_base[tid] + c] = first j with key_j >= (tid, c << 9)
        int32_t n_tid = 0;
        for (int64_t i = 0; i < T; ++i) n_tid = std::max(n_tid, h[(size_t)i].tid + 1);
        std::vector<int64_t> mxe((size_t)n_tid, -1);
        for (int64_t i = 0; i < T; ++i) if (h[(size_t)i].tid >= 0) mxe[(size_t)h[(size_t)i].tid] = std::max<int64_t>(mxe[(size_t)h[(size_t)i].tid], std::max(h[(size_t)i].end, 0));
        if (build_key_dir(key.data(), T, n_tid, mxe, o.kb_base, o.key_dir)) return tables_fail(msg, "[l2r_set_annotation] cursor directory too large");
        // words of chromosomes without buckets (no transcript): they share the next chromosome's first word
        o.n_tid_key = n_tid;
    }
    o.ex.resize((size_t)a->n_exon);
    for (int64_t k = 0; k < a->n_exon; ++k) o.ex[(size_t)k] = make_int2(a->ex_start[k], a->ex_end[k]);
    return 0;
}

// ---- the tables on disk (L2R_ANNO_CACHE=<directory>, or l2r_set_annotation_cache): one file per annotation, named by a
// hash of the arrays l2r_set_annotation was given + the layout constants; a hit replaces the sorts and the dictionary build
// by one read.  The file is written to a temporary name and renamed, so a reader never sees a partial file; anything that
// does not match (length, magic, hash, sizes) is ignored and rebuilt.
static uint64_t mix64(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, b + i, 8); h = (h ^ w) * 0x9E3779B97F4A7C15ULL; h ^= h >> 29; }
    uint64_t w = 0;
    if (i < n) { memcpy(&w, b + i, n - i); h = (h ^ w) * 0x9E3779B97F4A7C15ULL; h ^= h >> 29; }
    return (h ^ n) * 0xD6E8FEB86659FD93ULL;
}

static uint64_t annotation_hash(const l2r_annotation *a)
{
    const uint64_t consts[] = {0x4c3252414e4e4f32ULL /* format */, (uint64_t)SITE_SHIFT, sizeof(TxHdr), sizeof(SiteEnt), (uint64_t)a->n_tx, (uint64_t)a->n_exon};
    uint64_t h = mix64(0x1234567ULL, consts, sizeof consts);
    const size_t T = (size_t)a->n_tx, X = (size_t)a->n_exon;
    h = mix64(h, a->tx_tid, T * 4); h = mix64(h, a->tx_start, T * 4); h = mix64(h, a->tx_end, T * 4); h = mix64(h, a->tx_rev, T);
    h = mix64(h, a->tx_ex_off, (T + 1) * 8); h = mix64(h, a->ex_start, X * 4); h = mix64(h, a->ex_end, X * 4);
    return h;
}

struct CacheHead { char magic[8]; uint64_t hash; uint64_t n[12]; int64_t n_wide, n_compact; int32_t n_tid_dir, n_tid_key; uint64_t sum; };

static uint64_t tables_sum(const AnnoTables &t)
{
    uint64_t h = 0x7ab1e5;
    h = mix64(h, t.hdr.data(), t.hdr.size() * sizeof(TxHdr)); h = mix64(h, t.key.data(), t.key.size() * 8); h = mix64(h, t.key_raw.data(), t.key_raw.size() * 8);
    h = mix64(h, t.ex.data(), t.ex.size() * sizeof(int2)); h = mix64(h, t.st_ent.data(), t.st_ent.size() * sizeof(SiteEnt));
    h = mix64(h, t.en_ent.data(), t.en_ent.size() * sizeof(SiteEnt)); h = mix64(h, t.st_dir.data(), t.st_dir.size() * 4);
    h = mix64(h, t.st_rdir.data(), t.st_rdir.size() * 4); h = mix64(h, t.en_dir.data(), t.en_dir.size() * 4);
    h = mix64(h, t.tid_base.data(), t.tid_base.size() * 4); h = mix64(h, t.kb_base.data(), t.kb_base.size() * 4);
    return mix64(h, t.key_dir.data(), t.key_dir.size() * 4);
}

template <typename T> static bool put_vec(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool get_vec(FILE *f, std::vector<T> &v, uint64_t n) { v.resize((size_t)n); return n == 0 || fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n; }

static std::string cache_path(const std::string &dir, uint64_t hash)
{
    char name[64];
    snprintf(name, sizeof name, "/l2r_anno_%016llx.tables", (unsigned long long)hash);
    return dir + name;
}

static bool cache_load(const std::string &path, uint64_t hash, int64_t n_tx, int64_t n_exon, AnnoTables &t)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    CacheHead hd;
    bool ok = fread(&hd, sizeof hd, 1, f) == 1 && memcmp(hd.magic, "L2RANNO3", 8) == 0 && hd.hash == hash &&
              hd.n[0] == (uint64_t)n_tx && hd.n[1] == (uint64_t)n_tx && hd.n[2] == (uint64_t)n_tx && hd.n[3] == (uint64_t)n_exon;
    if (ok) {
        // the lengths must add up to the file's length before anything is allocated from them
        const uint64_t sz[12] = {sizeof(TxHdr), 8, 8, sizeof(int2), sizeof(SiteEnt), sizeof(SiteEnt), 4, 4, 4, 4, 4, 4};
        uint64_t want = sizeof hd;
        for (int k = 0; k < 12; ++k) { if (hd.n[k] > 0x7ffffff0ULL) ok = false; want += hd.n[k] * sz[k]; }
        fseek(f, 0, SEEK_END);
        ok = ok && (uint64_t)ftell(f) == want;
        fseek(f, (long)sizeof hd, SEEK_SET);
    }
    ok = ok && get_vec(f, t.hdr, hd.n[0]) && get_vec(f, t.key, hd.n[1]) && get_vec(f, t.key_raw, hd.n[2]) && get_vec(f, t.ex, hd.n[3]) &&
         get_vec(f, t.st_ent, hd.n[4]) && get_vec(f, t.en_ent, hd.n[5]) && get_vec(f, t.st_dir, hd.n[6]) && get_vec(f, t.st_rdir, hd.n[7]) &&
         get_vec(f, t.en_dir, hd.n[8]) && get_vec(f, t.tid_base, hd.n[9]) && get_vec(f, t.kb_base, hd.n[10]) && get_vec(f, t.key_dir, hd.n[11]);
    fclose(f);
    if (ok) { t.n_wide = hd.n_wide; t.n_compact = hd.n_compact; t.n_tid_dir = hd.n_tid_dir; t.n_tid_key = hd.n_tid_key; }
    // the payload is what was written, and the directories index the entries: nothing else may reach the kernels
    ok = ok && tables_sum(t) == hd.sum;
    ok = ok && t.tid_base.size() == (size_t)t.n_tid_dir + 1 && t.kb_base.size() == (size_t)t.n_tid_key + 1 &&
         t.st_dir.size() == t.st_rdir.size() && t.st_dir.size() == t.en_dir.size() && !t.st_dir.empty() &&
         t.st_dir.back() == t.st_ent.size() && t.en_dir.back() == t.en_ent.size() &&
         (int64_t)t.st_dir.size() == (int64_t)t.tid_base.back() + 1 && (int64_t)t.key_dir.size() == (int64_t)t.kb_base.back() + 1;
    return ok;
}

static void cache_store(const std::string &path, uint64_t hash, const AnnoTables &t)
{
    char tmp_suffix[48];
    snprintf(tmp_suffix, sizeof tmp_suffix, ".tmp.%ld", (long)getpid());
    const std::string tmp = path + tmp_suffix;
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return;                                        // a cache that cannot be written is no error
    CacheHead hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, "L2RANNO3", 8); hd.hash = hash;
    const uint64_t n[12] = {t.hdr.size(), t.key.size(), t.key_raw.size(), t.ex.size(), t.st_ent.size(), t.en_ent.size(), t.st_dir.size(),
                            t.st_rdir.size(), t.en_dir.size(), t.tid_base.size(), t.kb_base.size(), t.key_dir.size()};
    memcpy(hd.n, n, sizeof n);
    hd.n_wide = t.n_wide; hd.n_compact = t.n_compact; hd.n_tid_dir = t.n_tid_dir; hd.n_tid_key = t.n_tid_key;
    hd.sum = tables_sum(t);
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && put_vec(f, t.hdr) && put_vec(f, t.key) && put_vec(f, t.key_raw) && put_vec(f, t.ex) &&
              put_vec(f, t.st_ent) && put_vec(f, t.en_ent) && put_vec(f, t.st_dir) && put_vec(f, t.st_rdir) && put_vec(f, t.en_dir) &&
              put_vec(f, t.tid_base) && put_vec(f, t.kb_base) && put_vec(f, t.key_dir);
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());
}

// The annotation's tables, from the cache directory `dir` where there is one: read from its file, else built and stored.  Returns the
// cache state (0 no cache, 1 built + stored, 2 read from the cache), or -1 with the message of build_tables.
static int anno_tables(const l2r_annotation *a, const std::string &dir, AnnoTables &t, std::string &msg)
{
    if (dir.empty()) return build_tables(a, t, msg);
    const uint64_t hash = annotation_hash(a);
    const std::string path = cache_path(dir, hash);
    if (cache_load(path, hash, a->n_tx, a->n_exon, t)) return 2;
    t = AnnoTables();
    if (build_tables(a, t, msg)) return -1;
    (void)mkdir(dir.c_str(), 0777);
    cache_store(path, hash, t);
    return 1;
}

// ---- junction table: everything l2r_set_junctions derives from the rows before its first copy
struct SjTables {
    std::vector<int64_t> key, key_raw;                 // cursor keys of (tid, acc): prefix maximum / per row
    std::vector<int32_t> cbase, dbase;                 // SjDir (l2r_kernels.hip.h): the junction cursor's directory over `key` ...
    std::vector<uint32_t> cdir, ddir;                  // ... and the donors' (rows are sorted by (tid, don, acc))
    std::vector<int4> row;                             // (don, acc, uniq_c, multi_c)
    int32_t n_tid = 0;
};

static int build_sj_tables(const l2r_junctions *s, SjTables &o, std::string &msg)
{
    if (s->n < 0 || s->n > 0x7ffffff0LL) return tables_fail(msg, "[l2r_set_junctions] size out of range");
    const int64_t n = s->n;
    o.key.assign((size_t)n, 0);
    o.key_raw.assign((size_t)n, 0);
    int64_t run = INT64_MIN;
    for (int64_t i = 0; i < n; ++i) {
        if (i && (s->tid[i] < s->tid[i - 1] || (s->tid[i] == s->tid[i - 1] && (s->don[i] < s->don[i - 1] ||
            (s->don[i] == s->don[i - 1] && s->acc[i] < s->acc[i - 1])))))
            return tables_fail(msg, "[l2r_set_junctions] rows are not sorted by (tid, don, acc) at row %lld", (long long)i);
        // "row before read": tid smaller, or same tid and acc <= read start (update_gtf.c:613)
        const int64_t k = host_key(s->tid[i], s->acc[i]);
        o.key_raw[(size_t)i] = k;
        if (k > run) run = k;
        o.key[(size_t)i] = run;
    }
    // directories: the junction cursor (prefix-max keys of (tid, acc)) and the donors (rows are sorted by (tid, don, acc)): SjDir
    int32_t sj_ntid = 0;
    {
        for (int64_t i = 0; i < n; ++i) sj_ntid = std::max(sj_ntid, s->tid[i] + 1);
        std::vector<int64_t> mxa((size_t)sj_ntid, -1), mxd((size_t)sj_ntid, -1), dkey((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            dkey[(size_t)i] = host_key(s->tid[i], std::max(s->don[i], 0));
            if (s->tid[i] < 0) continue;
            mxa[(size_t)s->tid[i]] = std::max<int64_t>(mxa[(size_t)s->tid[i]], std::max(s->acc[i], 0));
            mxd[(size_t)s->tid[i]] = std::max<int64_t>(mxd[(size_t)s->tid[i]], std::max(s->don[i], 0));
        }
        if (build_key_dir(o.key.data(), n, sj_ntid, mxa, o.cbase, o.cdir) || build_key_dir(dkey.data(), n, sj_ntid, mxd, o.dbase, o.ddir))
            return tables_fail(msg, "[l2r_set_junctions] junction directories too large");
    }
    o.n_tid = sj_ntid;
    o.row.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) o.row[(size_t)i] = make_int4(s->don[i], s->acc[i], s->uniq_c[i], s->multi_c[i]);
    return 0;
}

// ---- the two sequential cursors of check_trans() (src/update_gtf.c:938 last_anno_i, last_sj_i) on the host, over the keys above.  After a
// sorted prefix a cursor is the prefix function of its last record: the first index whose running maximum lies behind (tid, pos + 1)
static inline int64_t cursor_after(const std::vector<int64_t> &key_pm, int32_t tid, int32_t pos)
{
    return std::upper_bound(key_pm.begin(), key_pm.end(), host_key(tid, pos + 1)) - key_pm.begin();
}

// Unsorted input: the cursor is history dependent (update_gtf.c:801-802) and only moves forward.  Replayed from `cur` over the reads that
// move it (moves(i); the others get 0): out[i] = the cursor read i sees.  Returns the cursor behind the last read.
template <typename Moves>
static int64_t cursor_replay(const std::vector<int64_t> &key_raw, int64_t cur, const int32_t *tid, const int32_t *pos, int64_t n, int32_t *out, Moves moves)
{
    const int64_t K = (int64_t)key_raw.size();
    for (int64_t i = 0; i < n; ++i) {
        if (!moves(i)) { out[i] = 0; continue; }
        const int64_t q = host_key(tid[i], pos[i] + 1);
        while (cur < K && key_raw[(size_t)cur] <= q) ++cur;
        out[i] = (int32_t)cur;
    }
    return cur;
}
}  // namespace l2r
