"""Restatement of the second filter stage of `lr2rmats sjtab` (l2r_sj_filter_rows2, `sjtab -d / -m / -s`): the checker of its tests.

The rule is the project's own, written after STAR's outSJfilterIntronMaxVsReadN and outSJfilterDistToOtherSJmin.  Rows are the nine
columns of tests/sjtab_restatement.py, (tid, don, acc, strand, motif, anno, uniq_c, multi_c, max_over), sorted by (tid, don, acc) with
one row per key.  Categories as there, and a motif above 6 counts as motif 0.

* stage 1, row-local -- the test of sjtab_restatement.kept, and the intron-size rule: with reads = max(1, uniq_c + multi_c), a row
  of category 1..4 with reads <= len(intron_max) stays only if acc - don + 1 <= intron_max[reads - 1]; annotated rows are exempt;
* stage 2, neighbours -- over exactly the rows stage 1 left, annotated ones included: dd(r) is the smallest |don(r) - don(q)| over the
  other rows q with r's tid, da(r) the same for acc; no other row on the tid gives FAR, and a distance is FAR at most.  A row of
  category c stays iff dd >= dist_min[c] and da >= dist_min[c].  The neighbours are the survivors of stage 1: a row that stage 2 drops
  still counts as a neighbour of the others.  All of dist_min zero: the stage is off.

Two forms: a literal one (for every row a loop over all other rows of its tid) and a numpy one (sort within tid, differences of
neighbours).  Nothing here imports lr2rmats_amd.
"""
import numpy as np

from tests import sjtab_restatement as st

FAR = 0x7fffffff
STAR_DIST = (0, 10, 0, 5, 10)                   # outSJfilterDistToOtherSJmin 10 0 5 10 behind the annotated class
STAR_INTRON_MAX = (50000, 100000, 200000)       # outSJfilterIntronMaxVsReadN
OFF = ((0,) * 5, ())


def category(anno, motif):
    return st.category(anno, motif if motif <= 6 else 0)


# ---------------------------------------------------------------------------------------------------- literal form

def too_long(row, intron_max):
    """The intron-size rule alone: True where it drops the row."""
    t, d, a, _, mo, an, u, m, _ = row
    reads = max(1, u + m)
    return category(an, mo) != 0 and reads <= len(intron_max) and a - d + 1 > intron_max[reads - 1]


def stage1(rows9, filt=st.DEFAULT_FILTER, intron_max=()):
    """-> (rows left, rows that pass the test of l2r_sj_filter_rows and that the intron-size rule drops)."""
    out, n_long = [], 0
    for r in rows9:
        if not st.kept(r[5], r[4] if r[4] <= 6 else 0, r[6], r[7], r[8], filt):
            continue
        if too_long(r, intron_max):
            n_long += 1
        else:
            out.append(r)
    return out, n_long


def nearest(rows9, i, col):
    """The smallest |difference| of column `col` between row i and every OTHER row of its tid; FAR where there is none."""
    best = FAR
    for k, q in enumerate(rows9):
        if k != i and q[0] == rows9[i][0]:
            best = min(best, abs(int(rows9[i][col]) - int(q[col])))
    return best


def stage2(rows9, dist_min=(0,) * 5):
    """-> (rows left, [(dd, da)] of every input row)."""
    if not any(dist_min):
        return list(rows9), [(FAR, FAR)] * len(rows9)
    near = [(nearest(rows9, i, 1), nearest(rows9, i, 2)) for i in range(len(rows9))]
    out = [r for r, (dd, da) in zip(rows9, near) if dd >= dist_min[category(r[5], r[4])] and da >= dist_min[category(r[5], r[4])]]
    return out, near


def filter2(rows9, filt=st.DEFAULT_FILTER, dist_min=(0,) * 5, intron_max=()):
    """-> (rows left, dropped for their intron size, dropped by the neighbour stage)."""
    s1, n_long = stage1(rows9, filt, intron_max)
    s2, _ = stage2(s1, dist_min)
    return s2, n_long, len(s1) - len(s2)


def expected_stdout(sam_text, seqs=None, introns=(), filt=st.DEFAULT_FILTER, dist_min=(0,) * 5, intron_max=(), min_intron=3, pair_only=False):
    """(the bytes `sjtab -d -m` writes for this SAM text, the two numbers of its extra stderr line)."""
    names, recs = st.sr.records_from_sam(sam_text)
    every = st.nine_columns(st.table(st.rows_of(recs, min_intron, pair_only)), seqs, introns, st.KEEP_ALL)
    rows, n_long, n_near = filter2(every, filt, dist_min, intron_max)
    return st.format_rows(rows, names), n_long, n_near


# ---------------------------------------------------------------------------------------------------- numpy form

def category_numpy(anno, motif):
    motif = np.asarray(motif).astype(np.int64)
    return st.category_numpy(anno, np.where(motif > 6, 0, motif))


def stage1_numpy(nine, filt=st.DEFAULT_FILTER, intron_max=()):
    """nine: the nine columns as arrays -> (keep mask, mask of the rows the intron-size rule alone drops)."""
    tid, don, acc, _, motif, anno, u, m, over = [np.asarray(c).astype(np.int64) for c in nine]
    motif = np.where(motif > 6, 0, motif)
    base = st.keep_numpy(anno, motif, u, m, over, filt)
    long_ = np.zeros(len(tid), bool)
    if len(intron_max):
        lim = np.asarray(intron_max, np.int64)
        reads = np.maximum(1, u + m)
        inside = (category_numpy(anno, motif) != 0) & (reads <= len(lim))
        long_ = inside & (acc - don + 1 > lim[np.minimum(reads, len(lim)) - 1])
    return base & ~long_, base & long_


def nearest_numpy(tid, val):
    """Per row the distance of `val` to the nearest other row of its tid: sort within tid, differences of the neighbours."""
    tid = np.asarray(tid, np.int64); val = np.asarray(val, np.int64)
    n = len(tid)
    out = np.full(n, FAR, np.int64)
    if n < 2:
        return out
    order = np.lexsort((val, tid))
    t, v = tid[order], val[order]
    gap = np.where(t[1:] == t[:-1], v[1:] - v[:-1], FAR)
    best = np.full(n, FAR, np.int64)
    best[1:] = np.minimum(best[1:], gap)
    best[:-1] = np.minimum(best[:-1], gap)
    out[order] = np.minimum(best, FAR)
    return out


def filter2_numpy(nine, filt=st.DEFAULT_FILTER, dist_min=(0,) * 5, intron_max=()):
    """-> dict(keep: mask over the input rows, s1: mask of the rows stage 1 left, n_long, n_near, dd, da: distances of the rows in s1)."""
    cols = [np.asarray(c).astype(np.int64) for c in nine]
    s1, long_ = stage1_numpy(cols, filt, intron_max)
    keep = s1.copy()
    dd = nearest_numpy(cols[0][s1], cols[1][s1])
    da = nearest_numpy(cols[0][s1], cols[2][s1])
    if any(dist_min):
        lim = np.asarray(dist_min, np.int64)[category_numpy(cols[5][s1], cols[4][s1])]
        keep[np.flatnonzero(s1)] = (dd >= lim) & (da >= lim)
    return dict(keep=keep, s1=s1, n_long=int(long_.sum()), n_near=int(s1.sum() - keep.sum()), dd=dd, da=da)


def columns(rows9):
    """[(nine values)] -> nine int64 arrays."""
    a = np.array(rows9, np.int64).reshape(-1, 9)
    return [a[:, k] for k in range(9)]


def random_rows(seed, n, n_tid=4, lo=1000, span=60000, len_max=30000, anno_every=7):
    """A sorted table of about n distinct rows for the size tests: donors dense in [lo, lo + span) so that many rows have another donor
    or acceptor within ten bases, intron lengths anywhere in [20, len_max) so that the acceptor order is not the donor order, 1 to 4
    reads per row, every `anno_every`-th row annotated.  Motifs are drawn here; a test that wants them from a genome replaces the two
    columns.  Returns the nine int64 columns."""
    rng = np.random.default_rng(seed)
    tid = rng.integers(0, n_tid, n)
    don = rng.integers(lo, lo + span, n)
    acc = don + rng.integers(20, len_max, n)
    key = np.unique(np.stack([tid, don, acc], axis=1), axis=0)
    m = len(key)
    motif = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5, 6]), m)
    strand = np.where(motif == 0, 0, 2 - (motif & 1))
    reads = rng.integers(1, 5, m)
    uq = rng.integers(0, reads + 1)
    anno = (np.arange(m) % anno_every == 3).astype(np.int64)
    over = rng.integers(0, 100, m)
    return [key[:, 0], key[:, 1], key[:, 2], strand, motif, anno, uq, reads - uq, over]


# ---------------------------------------------------------------------------------------------------- the hand-worked table

# STAR's two lists, and a row-local filter that lets a junction of the AT/AC class through without a read (the last case)
HAND_FILTER = ((1, 30, 12, 12, 12), (0, 3, 1, 1, 0), (0, 3, 1, 1, 0))
HAND_DIST = STAR_DIST
HAND_INTRON_MAX = STAR_INTRON_MAX
NC, GTAG, ATAC = (0, 0), (1, 1), (1, 5)         # (strand, motif)

# (tid, don, acc, (strand, motif), anno, uniq_c, multi_c, max_over), stays, why.  Groups are a thousand bases and more apart.
HAND = [
    ((0, 1000, 1100, GTAG, 0, 5, 0, 40), True, "GT/AG: dist_min 0, whatever shares its donor"),
    ((0, 1000, 1300, NC, 0, 5, 0, 40), False, "non-canonical on the donor of the row above: dd = 0 < 10"),
    ((0, 3000, 3500, GTAG, 0, 5, 0, 40), True, "GT/AG"),
    ((0, 3100, 3509, NC, 0, 5, 0, 40), False, "non-canonical, acceptor 9 bases from 3500: da = 9 < 10 (dd = 100)"),
    ((0, 5000, 5500, GTAG, 0, 5, 0, 40), True, "GT/AG"),
    ((0, 5100, 5510, NC, 0, 5, 0, 40), True, "non-canonical, acceptor 10 bases from 5500: da = 10, dd = 100"),
    ((0, 7000, 7100, GTAG, 0, 5, 0, 40), True, "GT/AG"),
    ((0, 7000, 7300, NC, 1, 5, 0, 40), True, "annotated non-canonical on a shared donor: dist_min[0] = 0"),
    ((0, 9000, 9100, NC, 0, 5, 0, 40), True, "its only close neighbour (the next row) went in stage 1, so it is no neighbour"),
    ((0, 9003, 9400, NC, 0, 1, 0, 40), False, "stage 1: non-canonical with one read"),
    ((0, 11000, 11100, NC, 0, 5, 0, 40), False, "dd = 5 to the next row"),
    ((0, 11005, 11300, NC, 0, 5, 0, 40), False, "dd = 5 to the row above"),
    ((0, 11012, 11600, NC, 0, 5, 0, 40), False, "dd = 7 to the row above, which stage 2 drops itself: it counts all the same"),
    ((0, 20000, 79999, GTAG, 0, 1, 0, 40), False, "60 000 bases, 1 read: above 50 000"),
    ((0, 100000, 159999, GTAG, 0, 1, 1, 40), True, "60 000 bases, 2 reads: 100 000 allowed"),
    ((0, 200000, 259999, GTAG, 0, 4, 0, 40), True, "60 000 bases, 4 reads: beyond the list"),
    ((0, 300000, 349999, GTAG, 0, 1, 0, 40), True, "exactly 50 000 bases, 1 read"),
    ((0, 400000, 459999, GTAG, 1, 1, 0, 40), True, "60 000 bases, 1 read, annotated: exempt"),
    ((0, 500000, 559999, ATAC, 0, 0, 0, 40), False, "both counts 0 count as one read: 60 000 > 50 000"),
    ((0, 600000, 649999, ATAC, 0, 0, 0, 40), True, "both counts 0, 50 000 bases"),
    ((1, 1000, 1100, GTAG, 0, 5, 0, 40), True, "the first pair on two references: alone on chr2"),
    ((2, 1000, 1300, NC, 0, 5, 0, 40), True, "... and alone on chr3: dd = da = FAR"),
]
HAND_ROWS = [(r[0], r[1], r[2], r[3][0], r[3][1], r[4], r[5], r[6], r[7]) for r, _, _ in HAND]
HAND_STAYS = [s for _, s, _ in HAND]
HAND_N_LONG = 2                                  # (20000, 79999) and (500000, 559999)
HAND_N_NEAR = 5
