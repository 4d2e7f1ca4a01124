"""Restatement of `lr2rmats sjtab` in Python: the checker of the sjtab tests.

The table of `bam2sj` (tests/sj_restatement.py: record filter, CIGAR walk, one row per (tid, don, acc) with the counts summed) in the
layout `update-gtf -j` reads, with three things the reference only advertises.  The rules are the project's own:

* overhang -- the junction operations (an N of at least `min_intron` bases) cut a record's CIGAR into blocks; a block's length is the
  sum of its M, = and X lengths; I, D, S, H, P, B and a shorter N add nothing and cut nothing; a record's overhang at a junction is
  min(block on its left, block on its right); the middle block of a record with two junctions serves both; an N that is the first or
  the last operation has overhang 0; a row's max_over is the maximum over the records that made it;
* annotated -- the row is the interval between two consecutive exons of a transcript (exons ascending inside the transcript,
  transcripts with tid -1 skipped, abutting or overlapping exons give nothing);
* filter -- category 0 annotated; else motif 0: 1, motif 1 2: 2, motif 3 4: 3, motif 5 6: 4; a row stays when
  max_over >= anchor_min[c] and (uniq_c >= uniq_min[c] or uniq_c + multi_c >= all_min[c]).

Two forms, as in sj_restatement: a literal one over parsed SAM records and a numpy one for size.  Nothing here imports lr2rmats_amd.
"""
import numpy as np

from tests import sj_restatement as sr

MATCH_OPS = (0, 7, 8)                           # M = X make up a block
DEFAULT_FILTER = ((1, 30, 12, 12, 12), (0, 3, 1, 1, 1), (0, 3, 1, 1, 1))      # anchor_min, uniq_min, all_min
KEEP_ALL = ((0,) * 5, (0,) * 5, (0,) * 5)
OVER_MAX = 0x7fffffff


def cigar_overhangs(cigar, min_intron=3):
    """[(length, op)] -> the overhang at every junction operation, in CIGAR order."""
    blocks, cur = [], 0
    for ln, op in cigar:
        if op == 3 and ln >= min_intron:
            blocks.append(cur)
            cur = 0
        elif op in MATCH_OPS:
            cur += ln
    blocks.append(cur)
    return [min(blocks[k], blocks[k + 1], OVER_MAX) for k in range(len(blocks) - 1)]


def record_kept(rec, pair_only=False):
    """Mapped; with -p also properly paired (bam2sj's quirk of always asking for FLAG & 2 is not carried over)."""
    return not (rec["flag"] & 4) and (not pair_only or bool(rec["flag"] & 2))


def record_rows(rec, min_intron=3):
    """Rows (tid, don, acc, uniq_c, multi_c, overhang) of one kept record."""
    rows = sr.record_rows(rec, min_intron)
    over = cigar_overhangs(rec["cigar"], min_intron)
    assert len(rows) == len(over)
    return [r + (o,) for r, o in zip(rows, over)]


def rows_of(recs, min_intron=3, pair_only=False):
    out = []
    for r in recs:
        if record_kept(r, pair_only):
            out += record_rows(r, min_intron)
    return out


def table(rows):
    """One row per (tid, don, acc) in that order: counts summed, overhang by maximum."""
    acc = {}
    for t, d, a, u, m, o in rows:
        s = acc.setdefault((t, d, a), [0, 0, 0])
        s[0] += u
        s[1] += m
        s[2] = max(s[2], o)
    return [k + tuple(acc[k]) for k in sorted(acc)]


def annotation_introns(tx_tid, tx_ex_off, ex_start, ex_end):
    """The set of (tid, first intron base, last intron base) of an annotation in the arrays of l2r_annotation."""
    out = set()
    for t in range(len(tx_tid)):
        if tx_tid[t] < 0:
            continue
        for k in range(int(tx_ex_off[t]), int(tx_ex_off[t + 1]) - 1):
            first, last = int(ex_end[k]) + 1, int(ex_start[k + 1]) - 1
            if last >= first:
                out.add((int(tx_tid[t]), first, last))
    return out


def category(anno, motif):
    if anno:
        return 0
    return 1 if motif == 0 else (motif + 1) // 2 + 1


def kept(anno, motif, uniq_c, multi_c, max_over, filt=DEFAULT_FILTER):
    c = category(anno, motif)
    return max_over >= filt[0][c] and (uniq_c >= filt[1][c] or uniq_c + multi_c >= filt[2][c])


def nine_columns(tab, seqs=None, introns=(), filt=DEFAULT_FILTER):
    """table() rows -> [(tid, don, acc, strand, motif, anno, uniq_c, multi_c, max_over)] of the rows that stay."""
    out = []
    for t, d, a, u, m, o in tab:
        mo, st = sr.motif_of(seqs, t, d, a)
        an = 1 if (t, d, a) in introns else 0
        if kept(an, mo, u, m, o, filt):
            out.append((t, d, a, st, mo, an, u, m, o))
    return out


def format_rows(rows9, names):
    return "".join("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((names[r[0]],) + tuple(r[1:])) for r in rows9).encode()


def expected_stdout(sam_text, seqs=None, introns=(), filt=DEFAULT_FILTER, min_intron=3, pair_only=False):
    """The bytes `sjtab` writes for this SAM text; introns: annotation_introns() of the -G file against the header's names."""
    names, recs = sr.records_from_sam(sam_text)
    return format_rows(nine_columns(table(rows_of(recs, min_intron, pair_only)), seqs, introns, filt), names)


def missing_nh(sam_text, pair_only=False):
    """The number the closing stderr line gives: kept records without an NH tag."""
    _, recs = sr.records_from_sam(sam_text)
    return sum(1 for r in recs if record_kept(r, pair_only) and not r["has_nh"])


# ---------------------------------------------------------------------------------------------------- numpy form

def rows_numpy(flag, tid, pos, uniq, cig_off, cig, min_intron=3, pair_only=False):
    """Six int64 columns (tid, don, acc, uniq_c, multi_c, overhang) in record order from the record columns."""
    five = sr.rows_numpy(flag, tid, pos, uniq, cig_off, cig, min_intron=min_intron, pair_only=pair_only)
    flag = np.asarray(flag).astype(np.int64); cig_off = np.asarray(cig_off).astype(np.int64); cig = np.asarray(cig).astype(np.int64)
    n = len(flag)
    keep = (flag & 4) == 0
    if pair_only:
        keep &= (flag & 2) != 0
    rec = np.repeat(np.arange(n), np.diff(cig_off))
    op, ln = cig & 15, cig >> 4
    junc = (op == 3) & (ln >= min_intron)
    # block id of every operation: junctions in front of it + its record (so no block spans two records and the block behind a
    # record's last junction is never another record's)
    blk = np.cumsum(junc) - junc + rec
    size = np.bincount(blk, weights=np.where(np.isin(op, MATCH_OPS), ln, 0).astype(np.float64), minlength=(int(blk.max()) + 2) if len(blk) else 2)
    size = np.minimum(size.astype(np.int64), OVER_MAX)
    hit = junc & keep[rec]
    over = np.minimum(size[blk[hit]], size[blk[hit] + 1])
    assert len(over) == len(five[0])
    return five + (over,)


def table_numpy(tid, don, acc, uniq_c, multi_c, over):
    """np.unique over the key, np.bincount of the counts, np.maximum.at of the overhang: six int64 columns, sorted."""
    five = sr.table_numpy(tid, don, acc, uniq_c, multi_c)
    if len(tid) == 0:
        return five + (np.zeros(0, np.int64),)
    keys = np.stack([np.asarray(tid, np.int64), np.asarray(don, np.int64), np.asarray(acc, np.int64)], axis=1)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    mx = np.zeros(len(five[0]), np.int64)
    np.maximum.at(mx, inv.reshape(-1), np.asarray(over, np.int64))
    return five + (mx,)


def anno_numpy(introns, tid, don, acc):
    return np.array([1 if (int(t), int(d), int(a)) in introns else 0 for t, d, a in zip(tid, don, acc)], np.uint8)


def category_numpy(anno, motif):
    motif = np.asarray(motif).astype(np.int64)
    return np.where(np.asarray(anno) != 0, 0, np.where(motif == 0, 1, (motif + 1) // 2 + 1))


def keep_numpy(anno, motif, uniq_c, multi_c, over, filt=DEFAULT_FILTER):
    c = category_numpy(anno, motif)
    f = [np.asarray(x, np.int64) for x in filt]
    u = np.asarray(uniq_c, np.int64); m = np.asarray(multi_c, np.int64)
    return (np.asarray(over, np.int64) >= f[0][c]) & ((u >= f[1][c]) | (u + m >= f[2][c]))


# ---------------------------------------------------------------------------------------------------- hand-worked cases

HAND_CIGARS = [
    # name, CIGAR, min_intron, overhangs
    ("plain", "10M20N7M", 3, [7]),
    ("shared middle block", "12M20N5M30N9M", 3, [5, 5]),
    ("I S D and a short N add nothing and cut nothing", "3S8M2I4M2D3M2N6M50N9M", 3, [9]),       # left 8 + 4 + 3 + 6 = 21, right 9
    ("N first", "40N10M", 3, [0]),
    ("= and X count", "4=3X50N10M", 3, [7]),
    ("N last", "10M40N", 3, [0]),
    ("H P B add nothing", "2H5M1P5M2B30N6M2H", 3, [6]),
    ("the short N cuts with -i 2", "3S8M2I4M2D3M2N6M50N9M", 2, [6, 6]),                         # 15 | 6 | 9
]
