"""Restatement of the annotation's and the junction table's tables (lr2rmats_amd/csrc/l2r_tables.hip.h) in Python: the checker of
tests/test_tables_cpu.py.

What l2r_set_annotation and l2r_set_junctions derive before anything is staged, as rules:

* headers -- per transcript its chromosome, span, strand, exon range, first and last exon; TX_MONO when exon starts and exon ends both
  rise strictly; TX_COMPACT when besides every exon has start <= end, the header's span is the exons' span, the transcript has a
  chromosome and two exons or more;
* sites -- only transcripts with a chromosome and two exons or more have any (none of their coordinates may be negative).  START keys
  are the exons (tid, start, end), END keys the junctions (tid, end, next start); a key's pair members are the transcripts that have
  it, its single members those in which its first coordinate is an acceptor (START: the start of an exon that is not the first) or a
  donor (END: the end of an exon that is not the last) -- the singles of a (tid, k1) belong to every key that begins with it;
* parts -- the members of a key, both kinds together, in rising order: a part begins at the lowest member no part has yet and holds
  the members less than 64 transcripts behind it, as two 64-bit masks relative to that member; a key of several parts has SE_WIDE on
  each of them and counts once in `n_wide`; the entries are in key order, a key's parts in a row;
* buckets -- per chromosome 512-base buckets up to the largest exon start or end of its transcripts with sites (none: no buckets);
  `dir[b]` is the number of entries in front of bucket b's, one closing word; START's `rdir[b]` is lower than `dir[b]` where an
  exon that begins in an earlier bucket reaches into b: the first part of the first such exon;
* cursor keys -- (tid + 1, end) of every transcript, `key_raw`, and their running maximum, `key`; `key_dir` has buckets per chromosome up
  to the largest transcript end (negative: 0), for every transcript with a chromosome, and says the first key at or behind a bucket's
  first base; one closing word for the first key behind every chromosome;
* junction rows -- sorted by (tid, don, acc) or rejected with the first row out of order; keys (tid + 1, acc) raw and as running
  maximum; the cursor directory over the running maximum with buckets up to the largest acceptor, the donor directory over
  (tid + 1, max(don, 0)) with buckets up to the largest donor (negative coordinates count as 0, rows without a chromosome give no
  buckets); the rows as (don, acc, unique, multi);
* cursors -- after a sorted upload that ends with a read: the first key whose running maximum lies behind (tid + 1, pos + 1); replayed:
  the cursor moves forward over the raw keys at or in front of (tid + 1, pos + 1), read by read, for the reads that move it.

`annotation_tables` and `junction_tables` take arrays and return dicts named like the members tests/tables_dump.hip writes.
"""
import bisect
from collections import defaultdict

SITE_SHIFT = 9                                                   # l2r_kernels.hip.h
TX_MONO, TX_COMPACT, SE_WIDE = 1, 2, 1
LIMIT_31 = 0x7ffffff0


class TablesError(Exception):
    pass


def host_key(tid, x):
    return ((tid + 1) << 32) | (x & 0xffffffff)


def _running_max(keys):
    out = []
    for k in keys:
        out.append(k if not out or k > out[-1] else out[-1])
    return out


def _key_dir(keys, n_tid, largest):
    """Buckets per chromosome up to largest[tid] (absent: none); per bucket the first key at or behind its first base; a closing word."""
    base, words = [0], []
    for t in range(n_tid):
        nb = (largest[t] >> SITE_SHIFT) + 1 if t in largest else 0
        words += [bisect.bisect_left(keys, host_key(t, c << SITE_SHIFT)) for c in range(nb)]
        base.append(base[-1] + nb)
    return base, words + [bisect.bisect_left(keys, host_key(n_tid, 0))]


def _dictionary(pairs, singles, tid_base, reach_back):
    """pairs: {(tid, k1, k2): set of transcripts}, singles: {(tid, k1): set of transcripts} -> entries (k1, k2, tx_base, flags, pair mask,
    single mask), dir, rdir (None without reach_back), keys of several parts."""
    ent, bucket, first_of, n_wide = [], [], {}, 0
    for key in sorted(pairs):
        tid, k1, k2 = key
        kinds = (sorted(pairs[key]), sorted(singles.get((tid, k1), ())))
        bases = []
        for m in sorted(set(kinds[0]) | set(kinds[1])):
            if not bases or m - bases[-1] >= 64:
                bases.append(m)
        first_of[key] = len(ent)
        n_wide += len(bases) > 1
        for b in bases:
            masks = [sum(1 << (m - b) for m in kind if 0 <= m - b < 64) for kind in kinds]
            ent.append((k1, k2, b, SE_WIDE if len(bases) > 1 else 0, masks[0], masks[1]))
            bucket.append(tid_base[tid] + (k1 >> SITE_SHIFT))
    n_buckets = tid_base[-1]
    dir_ = [bisect.bisect_left(bucket, b) for b in range(n_buckets)] + [len(ent)]
    rdir = None
    if reach_back:
        rdir = list(dir_)
        for (tid, k1, k2), first in first_of.items():
            last_bucket = tid_base[tid + 1] - tid_base[tid] - 1
            for cb in range((k1 >> SITE_SHIFT) + 1, min(k2 >> SITE_SHIFT, last_bucket) + 1):
                rdir[tid_base[tid] + cb] = min(rdir[tid_base[tid] + cb], first)
    return ent, dir_, rdir, n_wide


def annotation_tables(tx_tid, tx_start, tx_end, tx_rev, tx_ex_off, ex_start, ex_end):
    T, X = len(tx_tid), len(ex_start)
    hdr, key_raw = [], []
    st_pairs, st_singles, en_pairs, en_singles = defaultdict(set), defaultdict(set), defaultdict(set), defaultdict(set)
    largest, n_compact = {}, 0
    for i in range(T):
        lo, hi = int(tx_ex_off[i]), int(tx_ex_off[i + 1])
        if lo < 0 or hi < lo or hi > X:
            raise TablesError("[l2r_set_annotation] bad exon offsets at transcript %d" % i)
        if hi == lo:
            raise TablesError("[l2r_set_annotation] transcript %d has no exon" % i)
        tid, start, end = int(tx_tid[i]), int(tx_start[i]), int(tx_end[i])
        ex = [(int(ex_start[k]), int(ex_end[k])) for k in range(lo, hi)]
        mono = all(b[0] > a[0] and b[1] > a[1] for a, b in zip(ex, ex[1:]))
        compact = mono and all(s <= e for s, e in ex) and tid >= 0 and len(ex) >= 2 and (start, end) == (ex[0][0], ex[-1][1])
        n_compact += compact
        hdr += [tid, start, end, lo, len(ex), 1 if tx_rev[i] else 0, (TX_MONO if mono else 0) | (TX_COMPACT if compact else 0), 0,
                ex[0][0], ex[0][1], ex[-1][0], ex[-1][1]]
        key_raw.append(host_key(tid, end))
        if tid < 0 or len(ex) < 2:
            continue
        if any(s < 0 or e < 0 for s, e in ex):
            raise TablesError("[l2r_set_annotation] negative exon coordinate")
        largest[tid] = max([largest.get(tid, -1)] + [max(x) for x in ex])
        for k, (s, e) in enumerate(ex):
            st_pairs[(tid, s, e)].add(i)
            if k:
                st_singles[(tid, s)].add(i)
            if k + 1 < len(ex):
                en_pairs[(tid, e, ex[k + 1][0])].add(i)
                en_singles[(tid, e)].add(i)
    n_tid_dir = max(largest) + 1 if largest else 0
    tid_base = [0]
    for t in range(n_tid_dir):
        tid_base.append(tid_base[-1] + ((largest[t] >> SITE_SHIFT) + 1 if t in largest else 0))
    if tid_base[-1] > LIMIT_31:
        raise TablesError("[l2r_set_annotation] site directory too large")
    st_ent, st_dir, st_rdir, wide_st = _dictionary(st_pairs, st_singles, tid_base, True)
    en_ent, en_dir, _none, wide_en = _dictionary(en_pairs, en_singles, tid_base, False)
    key = _running_max(key_raw)
    n_tid_key = max([0] + [int(t) + 1 for t in tx_tid])
    ends = {}
    for t, e in zip(tx_tid, tx_end):
        if t >= 0:
            ends[int(t)] = max(ends.get(int(t), 0), int(e))
    kb_base, key_dir = _key_dir(key, n_tid_key, ends)
    return dict(hdr=hdr, key=key, key_raw=key_raw, ex=[int(v) for se in zip(ex_start, ex_end) for v in se],
                st_ent=st_ent, en_ent=en_ent, st_dir=st_dir, st_rdir=st_rdir, en_dir=en_dir, tid_base=tid_base, kb_base=kb_base, key_dir=key_dir,
                n_wide=wide_st + wide_en, n_compact=n_compact, n_tid_dir=n_tid_dir, n_tid_key=n_tid_key)


def junction_tables(tid, don, acc, uniq_c, multi_c):
    rows = [tuple(int(v) for v in r) for r in zip(tid, don, acc)]
    for i in range(1, len(rows)):
        if rows[i] < rows[i - 1]:
            raise TablesError("[l2r_set_junctions] rows are not sorted by (tid, don, acc) at row %d" % i)
    key_raw = [host_key(t, a) for t, _d, a in rows]
    key = _running_max(key_raw)
    n_tid = max([0] + [t + 1 for t, _d, _a in rows])
    accs, dons = {}, {}
    for t, d, a in rows:
        if t >= 0:
            accs[t], dons[t] = max(accs.get(t, 0), a), max(dons.get(t, 0), d)
    cbase, cdir = _key_dir(key, n_tid, accs)
    dbase, ddir = _key_dir([host_key(t, max(d, 0)) for t, d, _a in rows], n_tid, dons)
    return dict(sj_key=key, sj_key_raw=key_raw, sj_cbase=cbase, sj_cdir=cdir, sj_dbase=dbase, sj_ddir=ddir, sj_ntid=n_tid,
                sj_row=[int(v) for r in zip(don, acc, uniq_c, multi_c) for v in r])


def cursor_after(key, tid, pos):
    """The cursor behind a sorted upload that ends with the read (tid, pos): the keys whose running maximum is not behind it."""
    q = host_key(tid, pos + 1)
    return sum(1 for k in key if k <= q)


def cursor_replay(key_raw, start, tid, pos, moves=None):
    """(the cursor every read sees -- 0 for a read that does not move it --, the cursor behind the last read)"""
    seen, cur = [], start
    for i, (t, p) in enumerate(zip(tid, pos)):
        if moves is not None and not moves[i]:
            seen.append(0)
            continue
        rest = [j for j in range(cur, len(key_raw)) if key_raw[j] > host_key(int(t), int(p) + 1)]
        cur = rest[0] if rest else max(cur, len(key_raw))
        seen.append(cur)
    return seen, cur
