"""TEST INFRASTRUCTURE ONLY -- one table of edge cases for the kernels of `filter` and `fusion` (lr2rmats_amd/csrc/l2r_filter.hip.h,
l2r_fusion.hip.h) and their host half (l2r_filterplan.hip.h), used without a GPU (tests/test_filter_fusion_cases_cpu.py,
tests/test_filter_plan_cpu.py) and on one (tests/test_gpu_filter_fusion_edges.py).

Every case is the smallest input at which one rule can go wrong; it carries a name, the rule it shows and, where the answer can be
worked on paper, that answer as literals (`hand`).  What a kernel has to give (`want(case)`) comes from the literal restatements of the
reference's lines -- oracle/filter_oracle.py (score_record, remove_overlap, select) and tests/fusion_restatement.py (bam2seg,
check_fusion with ovlp_rat, check_with_exist1, bam_seg_cov) -- fed record by record through small stand-ins for a SAM record, so that
the float / double mix is the one written there and nowhere else.

Families: a threshold triples and the inputs at which the reference's mix of widths decides, b CIGAR shapes of k_filter_score, c the
span table and its lookup, d k_filter_select, e k_fusion_seg, f k_fusion_select, g rejected arguments.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from oracle import filter_oracle as fo
from tests import fusion_restatement as fr

M, I, D, N, S, H, P, EQ, X = 0, 1, 2, 3, 4, 5, 6, 7, 8           # CIGAR operations
F24 = 1 << 24


class Case:
    """kind: score | select | seg | fsel | spans | args.  inputs: what the kind's runner takes.  hand: the answer as literals or None.
    triple: the records / groups that just fail, lie exactly at and just pass a threshold; mix: for the inputs of family a at which the
    widths decide, how to redo the comparison (see `mix_verdicts`)."""

    def __init__(self, family, name, rule, kind, hand=None, mix=None, triple=None, **inputs):
        self.family, self.name, self.rule, self.kind, self.hand, self.mix, self.triple, self.inputs = family, name, rule, kind, hand, mix, triple, inputs

    def __repr__(self):
        return "Case(%s/%s)" % (self.family, self.name)


# ------------------------------------------------------------------------------------------------ stand-ins and restatement runners

class _Seq:
    """A SEQ of a given length that is never "*" (score_record only asks for its length)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _Rec:
    """What score_record / remove_overlap / bam2seg read of a fo.Record: flag, 1-based pos, cigar [(len, op)], seq, aux, qname."""

    def __init__(self, flag=0, pos0=0, cigar=(), l_qseq=0, nm=0, score=None, qname="r"):
        self.flag, self.pos, self.cigar, self.seq, self.qname = flag, pos0 + 1, list(cigar), _Seq(l_qseq), qname
        self.aux = ["NM:i:%d" % nm] + ([] if score is None else ["AS:i:%d" % score])


def i32(v: int) -> int:
    """A Python int as the 32-bit two's complement word it wraps to."""
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def rec(cigar, l_qseq=None, nm=0, flag=0, tid=0, pos=0):
    """A record for k_filter_score / k_fusion_seg; l_qseq defaults to what the CIGAR says (M I S = X)."""
    if l_qseq is None:
        l_qseq = sum(l for (l, op) in cigar if op in (M, I, S, EQ, X))
    return dict(flag=flag, tid=tid, pos=pos, l_qseq=l_qseq, nm=nm, cigar=list(cigar))


def columns(records):
    """flag, tid, pos, l_qseq, nm, cig_off, cig of a list of rec()."""
    off = np.cumsum([0] + [len(r["cigar"]) for r in records]).astype(np.int64)
    cig = np.asarray([(l << 4) | op for r in records for (l, op) in r["cigar"]], np.uint32)
    col = lambda k, t: np.asarray([r[k] for r in records], t)
    return col("flag", np.uint16), col("tid", np.int32), col("pos", np.int32), col("l_qseq", np.int32), col("nm", np.int32), off, cig


def want_score(records, prm, spans=None):
    """(drop, score, intron_n) of l2r_filter_score: score_record per record; intron_n is counted for every mapped record."""
    drop, score, intron = [], [], []
    for r in records:
        o = _Rec(r["flag"], r["pos"], r["cigar"], r["l_qseq"], r["nm"])
        got = fo.score_record(o, r["tid"], prm[0], prm[1], spans or ())
        drop.append(0 if got is not None else 1)
        score.append(got[0] if got is not None else 0)
        intron.append(0 if r["flag"] & 4 else sum(1 for (_, op) in r["cigar"] if op == N))
    return np.asarray(drop, np.uint8), np.asarray(score, np.int32), np.asarray(intron, np.int32)


def want_select(group_off, score, intron_n, prm):
    """winner of l2r_filter_select: the loop of fo.select over one stand-in record per row (one read name per group) whose
    score_record gives that row's score and intron count: 10^6 M, `intron_n` N operations, NM = 10^6 - score, -v 0 -q 0."""
    L = 1_000_000
    recs, grp = [], []
    for g in range(len(group_off) - 1):
        for k in range(group_off[g], group_off[g + 1]):
            recs.append(_Rec(0, 0, [(1, N)] * int(intron_n[k]) + [(L, M)], L, L - int(score[k]), qname="g%d" % g))
            grp.append(g)
    keep = fo.select(recs, [0] * len(recs), cov_rate=0.0, map_qual=0.0, sec_rat=prm[2], min_intron_n=prm[3])
    win = np.full(len(group_off) - 1, -1, np.int64)
    for k in keep:
        win[grp[k]] = k
    return win


def want_seg(records):
    """(read_start, read_end, ref_start, ref_end, qlen) of l2r_fusion_segments: bam2seg and bam_query_len per record, wrapped to 32 bits
    (they only add and subtract); a row of zeros for an unmapped record."""
    rows = []
    for r in records:
        o = _Rec(r["flag"], r["pos"], r["cigar"])
        s = fr.bam2seg(o, r["tid"], 0)
        rows.append((0, 0, 0, 0, 0) if s is None else tuple(i32(v) for v in (s.read_start, s.read_end, s.ref_start, s.ref_end, fr.query_len(r["cigar"]))))
    return tuple(np.asarray([row[k] for row in rows], np.int32) for k in range(5))


def want_fsel(groups, prm):
    """(first, second) of l2r_fusion_select: check_fusion per group of two rows or more.  groups: [(rlen, [(score, ed, tid, read_start,
    read_end, ref_start, ref_end), ...])]."""
    w1, w2, at = [], [], 0
    for (rlen, rows) in groups:
        sel = None
        if len(rows) >= 2:                                                        # src/bam_fusion.c:181
            segs = [fr.Seg(at + k, r[2], False, r[0], r[1], r[3], r[4], r[5], r[6]) for k, r in enumerate(rows)]
            sel = fr.check_fusion(segs, rlen, ovlp_frac=prm[0], each_cov=prm[1], all_cov=prm[2], dis=prm[3])
        ok = sel is not None and len(sel) == 2                                    # :183
        w1.append(sel[0].row if ok else -1); w2.append(sel[1].row if ok else -1)
        at += len(rows)
    return np.asarray(w1, np.int64), np.asarray(w2, np.int64)


def fsel_columns(groups):
    """group_off, score, ed, tid, read_start, read_end, ref_start, ref_end, rlen_of_group."""
    off = np.cumsum([0] + [len(rows) for (_, rows) in groups]).astype(np.int64)
    cols = [np.asarray([r[k] for (_, rows) in groups for r in rows], np.int32) for k in range(7)]
    return (off, *cols, np.asarray([rlen for (rlen, _) in groups], np.int32))


def want_spans(spans, probes):
    """remove_overlap for a record of chromosome tid that covers [lo, hi] (0-based pos = lo, hi - lo + 1 reference bases)."""
    return np.asarray([1 if fo.remove_overlap(_Rec(0, lo, [(hi - lo + 1, M)]), tid, spans) else 0 for (tid, lo, hi) in probes], np.uint8)


def want_table(spans):
    """The table filter_spans_build has to give, from its definition: per tid from -1 on the transcripts in front of the first one (file
    order) of a larger tid, sorted by (start, end), with the running maximum of the ends; off has n_tid + 2 words."""
    n_tid = max([t + 1 for (t, _, _) in spans] + [0])
    off, start, pmax = [0], [], []
    for v in range(-1, n_tid):
        mine = []
        for (t, s, e) in spans:
            if t > v:
                break
            if t == v:
                mine.append((s, e))
        run = None
        for (s, e) in sorted(mine):
            run = e if run is None else max(run, e)
            start.append(s); pmax.append(run)
        off.append(len(start))
    return n_tid, np.asarray(off, np.int64), np.asarray(start, np.int32), np.asarray(pmax, np.int32)


def want(case: Case):
    i = case.inputs
    if case.kind == "score":
        return want_score(i["records"], i["prm"], i.get("spans"))
    if case.kind == "select":
        return want_select(i["group_off"], i["score"], i["intron_n"], i["prm"])
    if case.kind == "seg":
        return want_seg(i["records"])
    if case.kind == "fsel":
        return want_fsel(i["groups"], i["prm"])
    if case.kind == "spans":
        return want_spans(i["spans"], i["probes"])
    raise ValueError(case.kind)


def kept(case: Case, w) -> List[bool]:
    """Per record / group / probe: kept, chosen, candidate, hit."""
    if case.kind == "score":
        return [d == 0 for d in w[0]]
    if case.kind == "select":
        return [x >= 0 for x in w]
    if case.kind == "fsel":
        return [x >= 0 for x in w[0]]
    if case.kind == "spans":
        return [x != 0 for x in w]
    raise ValueError(case.kind)


def mix_verdicts(mix) -> Dict[str, bool]:
    """The comparison of a family-a input redone in the reference's widths (`ref`), all in float and all in double; True = the record
    is kept / the row is not skipped / the pair is a candidate / the overlap is not over the bound."""
    f32, f64 = np.float32, np.float64
    how, a, b, opt = mix["how"], mix["a"], mix["b"], mix["opt"]
    if how == "ratio_lt":           # dropped where a / b < opt: src/bam_filter.c:77 and src/bam_fusion.c:119, a double ratio against the float option
        return dict(ref=not (f64(a) / f64(b) < f64(f32(opt))), float=not (f32(a) / f32(b) < f32(opt)), double=not (f64(a) / f64(b) < f64(opt)))
    if how == "prod_lt":            # a < opt * b: src/bam_filter.c:81 (dropped where it holds) and :141 (keep_below: kept where it holds), a float
        below = dict(ref=f32(a) < f32(opt) * f32(b), float=f32(a) < f32(opt) * f32(b), double=f64(a) < f64(f32(opt)) * f64(b),        # product against a
                     int=a < float(f32(opt)) * b)                                                                                      # converted int
        return {k: bool(v) == bool(mix.get("keep_below")) for k, v in below.items()}
    if how == "ratio_ge":           # candidate where (float)(a / b) >= opt: src/bam_fusion.c:111,123, a double ratio rounded to float
        return dict(ref=bool(f32(f64(a) / f64(b)) >= f32(opt)), float=bool(f32(a) / f32(b) >= f32(opt)), double=bool(f64(a) / f64(b) >= f64(f32(opt))))
    if how == "ratio_gt":           # over the bound where (float)(a / b) > opt: src/bam_fusion.c:71,76
        return dict(ref=not (f32(f64(a) / f64(b)) > f32(opt)), float=not (f32(a) / f32(b) > f32(opt)), double=not (f64(a) / f64(b) > f64(f32(opt))))
    raise ValueError(how)


# ------------------------------------------------------------------------------------------------ family a: thresholds

FILTER_PRM = (0.67, 0.75, 0.98, 0)                     # -v -q -s -i of the reference
FUSION_PRM = (0.1, 0.1, 0.99, 100000)                  # -o -v -V and the distance


def _cov_rec(qlen, lq, nm=0):
    """qlen of lq bases aligned: a leading soft clip of the rest."""
    return rec(([(lq - qlen, S)] if lq > qlen else []) + [(qlen, M)], l_qseq=lq, nm=nm)


def _split(rlen, cut, second_end=None, tid1=1):
    """Two rows that split a read of rlen bases behind base `cut`: the better row covers (cut, second_end], the other [1, cut]."""
    return (rlen, [(100, 0, 0, cut + 1, rlen if second_end is None else second_end, 1000, 1999), (50, 0, tid1, 1, cut, 5000, 5999)])


def _ovlp(ov):
    """s0 covers [1, 60] of 100 bases, the second row ten bases of which `ov` lie inside s0."""
    a = 60 - ov + 1
    return (100, [(100, 0, 0, 1, 60, 1000, 1059), (50, 0, 1, a, a + 9, 5000, 5009)])


def family_a() -> List[Case]:
    c = []
    add = lambda *a, **k: c.append(Case("a", *a, **k))
    # -- filter coverage: dropped where (double)qlen / (double)l_qseq < (double)cov_rate
    add("cov_0.67_triple", "coverage is a double ratio against the promoted float option: 0.67f = 11240735 / 2^24", "score", triple=(0, 1, 2),
        records=[_cov_rec(11240734, F24), _cov_rec(11240735, F24), _cov_rec(11240736, F24)], prm=(0.67, 0.0, 0.98, 0),
        hand=([1, 0, 0], [0, 11240735, 11240736], [0, 0, 0]))
    add("cov_0.67_of_100", "67 / 100 as a double is below (double)0.67f: dropped; in float alone the two are equal: kept", "score",
        records=[_cov_rec(67, 100), _cov_rec(68, 100)], prm=FILTER_PRM, hand=([1, 0], [0, 68], [0, 0]),
        mix=dict(how="ratio_lt", a=67, b=100, opt=0.67, wrong="float"))
    for v, (q, lq) in ((0.25, (25, 100)), (0.5, (50, 100))):
        add("cov_%s_equal" % v, "coverage exactly at an option that is exact in binary is not below it: kept", "score", triple=(0, 1, 2),
            records=[_cov_rec(q - 1, lq), _cov_rec(q, lq), _cov_rec(q + 1, lq)], prm=(v, 0.0, 0.98, 0), hand=([1, 0, 0], [0, q, q + 1], [0, 0, 0]))
    # -- filter identity: dropped where (float)s < map_qual * (float)qlen
    for q, s in ((10, 8), (5, 4)):
        add("identity_0.8_of_%d" % q, "identity is a float product: 0.8f * %d rounds to %d, %d is not below it: kept; in double the product is above" % (q, s, s),
            "score", triple=(0, 1, 2), records=[_cov_rec(q, q, nm=q - s + 1), _cov_rec(q, q, nm=q - s), _cov_rec(q, q, nm=q - s - 1)], prm=(0.67, 0.8, 0.98, 0),
            hand=([1, 0, 0], [0, s, s + 1], [0, 0, 0]), mix=dict(how="prod_lt", a=s, b=q, opt=0.8, wrong="double"))
    add("identity_beyond_2^24", "(float) rounds s and qlen: 16777217 and 16777216 are one float, 16777215 is below it", "score", triple=(2, 1, 0),
        records=[rec([(F24 + 1, M)], nm=k) for k in (0, 1, 2)], prm=(0.67, 1.0, 0.98, 0), hand=([0, 0, 1], [F24 + 1, F24, 0], [0, 0, 0]),
        mix=dict(how="prod_lt", a=F24, b=F24 + 1, opt=1.0, wrong="int"))
    for v, q in ((0.25, 100), (0.5, 100)):
        s = int(v * q)
        add("identity_%s_equal" % v, "identity exactly at an option that is exact in binary is not below it: kept", "score", triple=(0, 1, 2),
            records=[_cov_rec(q, q, nm=q - s + 1), _cov_rec(q, q, nm=q - s), _cov_rec(q, q, nm=q - s - 1)], prm=(0.1, v, 0.98, 0),
            hand=([1, 0, 0], [0, s, s + 1], [0, 0, 0]))
    # -- filter second score: kept where (float)s_score < sec_rat * (float)b_score
    for b, s in ((100, 98), (50, 49)):
        add("second_0.98_of_%d" % b, "the second score is compared in float: 0.98f * %d rounds to %d, %d is not below it: the read goes; in double it stays" % (b, s, s),
            "select", triple=(2, 1, 0), group_off=[0, 2, 4, 6], score=[b, s - 1, b, s, b, s + 1], intron_n=[0] * 6, prm=FILTER_PRM, hand=[0, -1, -1],
            mix=dict(how="prod_lt", a=s, b=b, opt=0.98, wrong="double", keep_below=True))
    for v in (0.25, 0.5):
        s = int(v * 100)
        add("second_%s_equal" % v, "a second score exactly at sec_rat * best (exact in binary) is not below it: the read goes", "select", triple=(2, 1, 0),
            group_off=[0, 2, 4, 6], score=[100, s - 1, 100, s, 100, s + 1], intron_n=[0] * 6, prm=(0.67, 0.75, v, 0), hand=[0, -1, -1])
    # -- fusion each_cov: a row is skipped where (double)span / (double)rlen < (double)each_cov
    # (0.1f = 13421773 / 2^27: an input exactly at it needs a read of 2^27 bases, which the restatement's bitmap walks base by base; the
    # inputs exactly at an option are those of 0.25 and 0.5 below)
    add("each_cov_0.1_of_100", "10 / 100 as a double is below (double)0.1f: the row is skipped; in float alone it is not", "fsel",
        triple=(0, None, 1), groups=[_split(100, 10), _split(100, 11)], prm=FUSION_PRM, hand=([-1, 2], [-1, 3]), mix=dict(how="ratio_lt", a=10, b=100, opt=0.1, wrong="float"))
    for v in (0.25, 0.5):
        q = int(v * 100)
        add("each_cov_%s_equal" % v, "a span exactly at an option that is exact in binary is not below it: not skipped", "fsel", triple=(0, 1, 2),
            groups=[_split(100, q - 1), _split(100, q), _split(100, q + 1)], prm=(0.1, v, 0.99, 100000), hand=([-1, 2, 4], [-1, 3, 5]))
    # -- fusion all_cov: a candidate where (float)((double)covered / (double)rlen) >= all_cov
    add("all_cov_0.99_of_100", "the covered fraction is rounded to float in front of the comparison: 99 / 100 is 0.99f: a candidate; in double it is below", "fsel",
        triple=(0, 1, 2), groups=[_split(100, 50, 98), _split(100, 50, 99), _split(100, 50, 100)], prm=FUSION_PRM, hand=([-1, 2, 4], [-1, 3, 5]),
        mix=dict(how="ratio_ge", a=99, b=100, opt=0.99, wrong="double"))
    for v in (0.25, 0.5):
        q = int(v * 100)
        add("all_cov_%s_equal" % v, "a covered fraction exactly at an option that is exact in binary is enough (>=)", "fsel", triple=(0, 1, 2),
            groups=[_split(100, 12, q - 1), _split(100, 12, q), _split(100, 12, q + 1)], prm=(0.1, 0.1, v, 100000), hand=([-1, 2, 4], [-1, 3, 5]))
    # -- fusion ovlp_frac: a row goes where (float)((double)overlap / (double)shorter) > ovlp_frac
    add("ovlp_0.7_of_10", "the overlap fraction is rounded to float in front of the comparison: 7 / 10 is 0.7f, not over it; in double it is", "fsel",
        triple=(2, 1, 0), groups=[_ovlp(6), _ovlp(7), _ovlp(8)], prm=(0.7, 0.05, 0.5, 100000), hand=([0, 2, -1], [1, 3, -1]),
        mix=dict(how="ratio_gt", a=7, b=10, opt=0.7, wrong="double"))
    add("ovlp_0.5_equal", "an overlap exactly at an option that is exact in binary is not over it (>): 5 of 10", "fsel", triple=(2, 1, 0),
        groups=[_ovlp(4), _ovlp(5), _ovlp(6)], prm=(0.5, 0.05, 0.5, 100000), hand=([0, 2, -1], [1, 3, -1]))
    add("ovlp_0.25_equal", "an overlap exactly at an option that is exact in binary is not over it (>): 3 of 12", "fsel", triple=(2, 1, 0),
        groups=[(100, [(100, 0, 0, 1, 60, 1000, 1059), (50, 0, 1, 60 - ov + 1, 60 - ov + 12, 5000, 5011)]) for ov in (2, 3, 4)], prm=(0.25, 0.05, 0.5, 100000),
        hand=([0, 2, -1], [1, 3, -1]))
    return c


# ------------------------------------------------------------------------------------------------ family b: CIGAR shapes of k_filter_score

def family_b() -> List[Case]:
    c = []
    add = lambda name, rule, records, hand=None, prm=FILTER_PRM, **k: c.append(Case("b", name, rule, "score", records=records, prm=prm, hand=hand, **k))
    add("no_operation", "a mapped record without a CIGAR: qlen = l_qseq, score = l_qseq - NM", [rec([], l_qseq=100, nm=3), rec([], l_qseq=100, nm=30)],
        ([0, 1], [97, 0], [0, 0]))
    add("one_S", "the only operation is a clip: it is subtracted once (the second subtraction asks for more than one operation)",
        [rec([(10, S)], l_qseq=100), rec([(34, S)], l_qseq=100)], ([0, 1], [90, 0], [0, 0]))
    add("one_H", "the only operation is a hard clip: subtracted once", [rec([(10, H)], l_qseq=100), rec([(34, H)], l_qseq=100)], ([0, 1], [90, 0], [0, 0]))
    add("clips_at_both_ends", "the first and the last operation are clips: both are subtracted",
        [rec([(10, S), (80, M), (10, S)]), rec([(20, S), (60, M), (20, S)]), rec([(10, H), (70, M), (10, S)], l_qseq=100)], ([0, 1, 0], [80, 0, 80], [0, 0, 0]))
    add("H_last", "a hard clip in last place is subtracted from l_qseq although SEQ does not hold it", [rec([(90, M), (10, H)], l_qseq=100), rec([(90, M), (10, H)], l_qseq=90)],
        ([0, 0], [90, 80], [0, 0]))
    add("two_clips_only", "exactly two operations, both clips: both are subtracted", [rec([(10, S), (10, H)], l_qseq=100), rec([(20, H), (20, S)], l_qseq=100)],
        ([0, 1], [80, 0], [0, 0]))
    add("clip_in_the_middle", "a clip that is neither first nor last subtracts nothing", [rec([(40, M), (30, S), (30, M)])], ([0], [100], [0]))
    add("l_qseq_0", "l_qseq 0: 0 / 0 is NaN, which is not below the option: the coverage test passes (score 0); -5 / 0 is below it", [rec([(50, M)], l_qseq=0, nm=0), rec([], l_qseq=0, nm=0), rec([(5, S), (50, M)], l_qseq=0)],
        ([0, 0, 1], [0, 0, 0], [0, 0, 0]))
    add("every_operation", "N counts an intron, D adds to the score, M D N = X (and nothing else, codes 9..15 included) consume the reference",
        [rec([(30, M), (100, N), (20, EQ), (5, D), (10, X), (7, I), (4, P), (33, M)], nm=9),
         rec([(20, M), (50, N), (3, 9), (3, 10), (3, 11), (60, N), (3, 12), (3, 13), (3, 14), (3, 15), (80, M)], nm=0, l_qseq=100),
         rec([(10, M), (7, N), (10, M), (8, N), (10, M), (9, N), (70, M)], nm=0)], ([0, 0, 0], [96, 100, 100], [1, 2, 3]))
    add("nm_above_qlen", "NM greater than qlen: a negative score is below 0 * qlen even with -q 0; deleted bases are added in front of the test",
        [rec([(100, M)], nm=101), rec([(100, M), (50, D)], nm=101)], ([1, 0], [0, 49], [0, 0]), prm=(0.67, 0.0, 0.98, 0))
    add("deletion_lifts_score", "deleted bases are added to the score: NM above qlen is kept where the deletion pays for it",
        [rec([(50, M), (60, D), (50, M)], nm=101), rec([(50, M), (60, D), (50, M)], nm=85)], ([1, 0], [0, 75], [0, 0]))
    add("unmapped", "an unmapped record is dropped, its intron count 0 whatever its CIGAR", [rec([(50, M), (100, N), (50, M)], flag=4), rec([(50, M), (100, N), (50, M)], flag=0),
                                                                                              rec([], l_qseq=30, flag=4 | 1)], ([1, 0, 1], [0, 100, 0], [0, 1, 0]))
    add("dropped_keeps_introns", "the intron count of a mapped record is written whether it is kept or not", [rec([(10, M), (100, N), (10, M), (80, S)]), rec([(50, M), (9, N), (50, M)], nm=50)],
        ([1, 1], [0, 0], [1, 1]))
    # -- the third sum, rlen, shows only through the -r lookup: every record on a chromosome of its own with one transcript
    only_is = [(5, S), (90, I), (5, S)]                  # no reference base: rlen 0, the record covers [pos, pos - 1]
    add("only_I_and_S", "a record of only I and S has rlen 0, hi = pos - 1: a transcript that starts at pos is not met, nor one that ends at pos - 1; one over both is",
        [rec(only_is, tid=0, pos=100), rec(only_is, tid=1, pos=100), rec(only_is, tid=2, pos=100)], ([0, 1, 0], [90, 0, 90], [0, 0, 0]),
        spans=[(0, 100, 200), (1, 99, 100), (2, 50, 99)])
    counted, not_counted = [M, D, N, EQ, X], [I, S, H, P, 9, 10, 11, 12, 13, 14, 15]
    add("rlen_per_operation", "7 bases of one operation between two of 10: the transcript starts at pos + 26, met where the 7 count for rlen: M D N = X, not I S H P 9..15",
        [rec([(10, EQ if op == M else M), (7, op), (10, EQ if op == M else M)], tid=k, pos=100) for k, op in enumerate(counted + not_counted)],
        ([1] * 5 + [0] * 11, [0] * 5 + [27, 27, 20, 20] + [20] * 7, [0, 0, 1, 0, 0] + [0] * 11), spans=[(k, 126, 300) for k in range(16)])
    every = [(30, M), (100, N), (20, EQ), (5, D), (10, X), (7, I), (4, P), (3, 9), (3, 15), (33, M)]      # rlen 198: pos 999 .. 1196
    add("rlen_of_every_operation", "every operation in one record: rlen is 198, a transcript from pos + 197 is met, one from pos + 198 is not",
        [rec(every, tid=0, pos=999, nm=9), rec(every, tid=1, pos=999, nm=9)], ([1, 0], [0, 96], [1, 1]), spans=[(0, 1196, 2000), (1, 1197, 2000)])
    return c


# ------------------------------------------------------------------------------------------------ family c: span table and lookup

def _grid(spans, tids, reach=2):
    """Every (tid, lo, hi) with lo and hi within `reach` of a transcript's start or end, hi >= lo - 1 (a record of no reference base)."""
    marks = sorted({v + d for (_, s, e) in spans for v in (s, e) for d in range(-reach, reach + 1)})
    return [(t, lo, hi) for t in tids for lo in marks for hi in marks if hi >= lo - 1]


def family_c() -> List[Case]:
    c = []

    def add(name, rule, spans, named, tids=None):
        """named: [(tid, lo, hi, answer)] worked by hand; the grid around every transcript's ends follows them."""
        tids = sorted({t for (t, _, _) in spans if t >= 0} | {-1, max([t for (t, _, _) in spans] + [-1]) + 1}) if tids is None else tids
        probes = [p[:3] for p in named] + _grid(spans, tids)
        c.append(Case("c", name, rule, "spans", spans=spans, probes=probes, hand=[p[3] for p in named]))

    add("order_0_2_1_1", "the walk stops at the first larger tid: behind [0, 2] a record of tid 1 meets nothing, one of tid 0 only the first",
        [(0, 100, 200), (2, 100, 200), (1, 100, 200), (1, 300, 400)], [(0, 150, 160, 1), (1, 150, 160, 0), (1, 350, 360, 0), (2, 150, 160, 1), (3, 150, 160, 0)])
    add("order_0_1_0", "a transcript of tid 0 behind one of tid 1 is never reached", [(0, 100, 200), (1, 100, 200), (0, 300, 400)], [(0, 150, 150, 1), (0, 350, 350, 0), (1, 150, 150, 1)])
    add("order_2_0_1", "file order [2, 0, 1]: records of tid 0 and 1 stop at the first transcript", [(2, 100, 200), (0, 100, 200), (1, 100, 200)],
        [(0, 150, 160, 0), (1, 150, 160, 0), (2, 150, 160, 1)])
    add("tid_minus_1", "a transcript of tid -1 stops nothing; tids are compared as numbers: a record of tid -1 meets it where it lies in front of the first tid >= 0",
        [(-1, 100, 200), (0, 100, 200), (-1, 1, 1000), (1, 300, 400)], [(-1, 150, 160, 1), (-1, 250, 260, 0), (0, 150, 160, 1), (1, 350, 360, 1), (0, 350, 360, 0)])
    add("record_tid_minus_1", "a record of tid -1 stops at the first transcript of a chromosome the header knows", [(0, 100, 200), (-1, 100, 200)], [(-1, 150, 160, 0), (0, 150, 160, 1)])
    add("empty_chromosome_between", "a chromosome without a transcript between two that have some", [(0, 100, 200), (2, 300, 400)],
        [(0, 150, 160, 1), (1, 150, 160, 0), (1, 350, 360, 0), (2, 350, 360, 1), (2, 150, 160, 0)])
    add("tid_at_n_tid", "a record of a tid the table does not have (n_tid, beyond it, -1)", [(0, 100, 200), (1, 100, 200)], [(2, 150, 160, 0), (3, 150, 160, 0), (-1, 150, 160, 0), (-2, 150, 160, 0), (1, 150, 160, 1)],
        tids=[-1, 0, 1, 2, 3])
    add("equal_starts", "transcripts with one start: the running maximum holds the longest end", [(0, 100, 300), (0, 100, 120), (0, 100, 200)],
        [(0, 250, 260, 1), (0, 300, 310, 1), (0, 301, 310, 0), (0, 90, 99, 0), (0, 90, 100, 1)])
    add("long_over_short", "a long first transcript covers three short later ones: behind each short end the long one still answers",
        [(0, 100, 1000), (0, 200, 210), (0, 400, 410), (0, 600, 610)], [(0, 211, 215, 1), (0, 411, 415, 1), (0, 611, 615, 1), (0, 1000, 1005, 1), (0, 1001, 1005, 0)])
    add("short_then_long", "short transcripts in front of a long one in file order, not sorted by start", [(0, 600, 610), (0, 200, 210), (0, 100, 1000), (0, 50, 60)],
        [(0, 61, 99, 0), (0, 61, 100, 1), (0, 611, 615, 1), (0, 40, 49, 0), (0, 40, 50, 1)])
    add("hi_at_start", "hi == start meets, hi == start - 1 does not", [(0, 100, 200)], [(0, 90, 100, 1), (0, 90, 99, 0), (0, 100, 99, 0), (0, 101, 100, 1)])
    add("lo_at_end", "lo == end meets, lo == end + 1 does not", [(0, 100, 200)], [(0, 200, 210, 1), (0, 201, 210, 0), (0, 200, 199, 1), (0, 201, 200, 0)])
    add("zero_based_pos", "the 0-based pos against 1-based coordinates, as the reference has it: a read on 1-based 101..190 is pos 100, hi 189",
        [(0, 190, 300), (1, 1, 99), (2, 189, 300), (3, 1, 100)], [(0, 100, 189, 0), (1, 100, 189, 0), (2, 100, 189, 1), (3, 100, 189, 1)])
    add("empty_table", "no transcript", [], [(0, 1, 10, 0), (-1, 1, 10, 0)], tids=[-1, 0, 1])
    add("all_negative", "every transcript on a chromosome the header does not know: n_tid 0, only a record of tid -1 meets them", [(-1, 1, 1000), (-1, 5, 50)], [(0, 1, 10, 0), (-1, 1, 10, 1), (-1, 1001, 1010, 0)], tids=[-1, 0, 1])
    return c


# ------------------------------------------------------------------------------------------------ family d: k_filter_select

def _alternate(n_groups):
    """Groups of one and two rows in turn; odd groups hold two equal scores (dropped), even groups one row of score 7 (kept)."""
    off, score = [0], []
    for g in range(n_groups):
        score += [7] if g % 2 == 0 else [9, 9]
        off.append(len(score))
    return off, score


def family_d() -> List[Case]:
    c = []

    def add(name, rule, group_off, score, intron_n=None, hand=None, prm=(0.67, 0.75, 0.98, 0)):
        c.append(Case("d", name, rule, "select", group_off=group_off, score=score, intron_n=[0] * len(score) if intron_n is None else intron_n, prm=prm, hand=hand))

    add("one_row", "a group of one: score 0 goes (0 < 0.98 * 0 is false), score 1 stays", [0, 1, 2], [0, 1], hand=[-1, 1])
    add("one_row_introns", "a group of one with too few introns goes", [0, 1, 2, 3], [50, 50, 50], [0, 1, 2], hand=[-1, 1, 2], prm=(0.67, 0.75, 0.98, 1))
    add("equal_scores", "two equal scores: the first is the best, the second becomes s_score: the group goes", [0, 2, 4, 7], [90, 90, 90, 80, 70, 90, 90], hand=[-1, 0 + 2, -1])
    add("best_last_fewer_introns", "the intron count is the best row's: best in last place with fewer introns than an earlier row", [0, 2, 4], [50, 90, 90, 50], [2, 0, 2, 0],
        hand=[-1, 2], prm=(0.67, 0.75, 0.98, 1))
    add("rising", "a strictly rising group of five: the last is the best, the one before it the second", [0, 5, 10], [10, 20, 30, 40, 50, 46, 47, 48, 49, 50], hand=[4, -1])
    add("falling", "a strictly falling group of five: the first is the best, the second row the second", [0, 5, 10], [50, 40, 30, 20, 10, 50, 49, 30, 20, 10], hand=[0, -1])
    add("second_behind_best", "a second best behind the best raises s_score", [0, 3, 6], [10, 90, 89, 10, 90, 88], hand=[-1, 4])
    for n in (255, 256, 257):
        off, score = _alternate(n)
        if n % 2 == 0:                                   # the last group is kept in every set
            score[-2:] = [9, 1]
        c.append(Case("d", "%d_groups" % n, "the last workgroup is full, one short and one over; the last group is kept", "select", group_off=off, score=score,
                      intron_n=[0] * len(score), prm=(0.67, 0.75, 0.98, 0)))
    return c


# ------------------------------------------------------------------------------------------------ family e: k_fusion_seg

def _body(n_ops, seed=0):
    """n_ops operations whose three sums depend on every word: M I D N = X and (not in first place) S, lengths all distinct."""
    ops = (M, I, D, N, EQ, X, S)
    return [(3 * k + 1 + seed, ops[(k * 5 + seed) % 7] if k else M) for k in range(n_ops)]


def _both_strands(records):
    return [dict(r, flag=r["flag"] | f) for r in records for f in (0, 16)]


def family_e() -> List[Case]:
    c = []
    add = lambda name, rule, records, hand=None, **k: c.append(Case("e", name, rule, "seg", records=records, hand=hand, **k))
    add("operation_counts", "records of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 4097 operations: the wave form's strided walk and its reduction take every word once",
        _both_strands([rec(_body(n, n % 5), pos=1000 + n) for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)]))
    for n in (1, 3, 4, 5, 257):
        add("%d_records" % n, "a record count that leaves idle waves in the last workgroup of the wave form (4 records a workgroup)",
            [rec(_body(k % 7, k), pos=10 * k, flag=16 * (k & 1)) for k in range(n)])
    add("first_S", "a soft clip in first place shifts the read interval", _both_strands([rec([(10, S), (80, M), (10, S)], pos=99)]),
        ([11, 11], [90, 90], [100, 100], [179, 179], [100, 100]))
    add("first_H", "a hard clip in first place shifts the read interval past a length that does not count it", _both_strands([rec([(10, H), (80, M), (10, S)], pos=99)]),
        ([11, 1], [90, 80], [100, 100], [179, 179], [90, 90]))
    add("only_a_clip", "the only operation is a clip: an empty interval behind it", _both_strands([rec([(10, S)], pos=99), rec([(10, H)], pos=99)]),
        ([11, 1, 11, -9], [10, 0, 10, -10], [100] * 4, [99] * 4, [10, 10, 0, 0]))
    add("clips_elsewhere", "S and H in the middle and at the end shift nothing (S counts for qlen)",
        _both_strands([rec([(30, M), (10, S), (30, M), (10, H), (20, M), (5, S)], pos=0), rec([(30, M), (10, H)], pos=0)]),
        ([1, 16, 1, 1], [80, 95, 30, 30], [1] * 4, [80, 80, 30, 30], [95, 95, 30, 30]))
    add("every_operation", "M = X to both ends, I to the read, D N to the reference, P and the codes 9..15 to nothing",
        _both_strands([rec([(5, S), (30, M), (100, N), (20, EQ), (5, D), (10, X), (7, I), (4, P), (3, 9), (3, 15), (33, M)], pos=999)]),
        ([6, 1], [105, 100], [1000, 1000], [1197, 1197], [105, 105]))
    add("unmapped", "an unmapped record with operations: a row of zeros", [rec([(50, M)], flag=4, pos=77), rec([(50, M)], flag=4 | 16, pos=77), rec([(50, M)], pos=77)],
        ([0, 0, 1], [0, 0, 50], [0, 0, 78], [0, 0, 127], [0, 0, 50]))
    # 17 * (2^28 - 1) = 4563402735 = 2^32 + 268435439
    add("sums_wrap", "32-bit sums that wrap: 17 M operations of 2^28 - 1 bases behind a clip of 5", _both_strands([rec([(5, S)] + [(0xFFFFFFF, M)] * 17, l_qseq=0, pos=100)]),
        ([6, 1], [268435444, 268435439], [101, 101], [268435539, 268435539], [268435444, 268435444]))
    # 9 * (2^28 - 1) = 2415919095 = 2^32 - 1879048201
    add("sums_go_negative", "32-bit sums that pass 2^31: 9 M operations of 2^28 - 1 bases", _both_strands([rec([(0xFFFFFFF, M)] * 9, l_qseq=0, pos=100)]),
        ([1, 1], [-1879048201, -1879048201], [101, 101], [-1879048101, -1879048101], [-1879048201, -1879048201]))
    add("auto_128", "4 records with 128 operations in all: 32 a record is not above the bound: the thread form", [rec(_body(32, k), pos=k) for k in range(4)], auto_wave=0.0)
    add("auto_129", "4 records with 129 operations in all: the wave form", [rec(_body(32 + (k == 2), k), pos=k) for k in range(4)], auto_wave=1.0)
    return c


# ------------------------------------------------------------------------------------------------ family f: k_fusion_select

def family_f() -> List[Case]:
    c = []
    add = lambda name, rule, groups, hand=None, prm=FUSION_PRM: c.append(Case("f", name, rule, "fsel", groups=groups, prm=prm, hand=hand))
    A = (100, 0, 0, 1, 50, 10000, 10049)                # the first part: read 1..50, chromosome 0 10000..10049
    B = (50, 0, 1, 51, 100, 5000, 5049)                 # a second part on another chromosome that passes every test
    add("two_and_three_rows", "groups of one, two and three rows", [(100, [A]), (100, [A, B]), (100, [A, B, (40, 0, 2, 51, 100, 1, 50)]), (100, [B])], ([-1, 1, 3, -1], [-1, 2, 4, -1]))
    DIS = 1000
    for side in ("downstream", "upstream"):
        rows, hand1 = [], []
        for d in (1, DIS - 1, DIS, DIS + 1):
            fs = 10049 + d if side == "downstream" else 10000 - d - 49
            rows.append((100, [A, (50, 0, 0, 51, 100, fs, fs + 49)]))
        add("distance_" + side, "the second part %s of the first on one chromosome at 1, dis - 1, dis and dis + 1: a distance inside (0, dis) goes" % side, rows,
            ([-1, -1, 4, 6], [-1, -1, 5, 7]), prm=(0.1, 0.1, 0.99, DIS))
    for dis in (0, 1, 2):
        add("dis_%d" % dis, "adjacent parts (distance 1) on both sides with dis %d" % dis,
            [(100, [A, (50, 0, 0, 51, 100, 10050, 10099)]), (100, [A, (50, 0, 0, 51, 100, 9950, 9999)])], ([0, 2], [1, 3]) if dis < 2 else ([-1, -1], [-1, -1]), prm=(0.1, 0.1, 0.99, dis))
    add("same_spans_other_chromosome", "the same reference span on another chromosome is no overlap", [(100, [A, (50, 0, 1, 51, 100, 10000, 10049)]), (100, [A, (50, 0, 0, 51, 100, 10000, 10049)])],
        ([0, -1], [1, -1]))
    add("reference_spans_touch", "reference spans that share one base overlap: rejected, on both sides",
        [(100, [A, (50, 0, 0, 51, 100, 9951, 10000)]), (100, [A, (50, 0, 0, 51, 100, 10049, 10098)]), (100, [A, (50, 0, 1, 51, 100, 10049, 10098)])], ([-1, -1, 4], [-1, -1, 5]))
    add("read_overlap_one_base", "ovlp_rat is not symmetric: one shared base counts 1 with the second part to the right, end1 - start2 + 1 = 100 with it to the left",
        [(100, [(100, 0, 0, 1, 50, 10000, 10049), (50, 0, 1, 50, 100, 5000, 5049)]), (100, [(100, 0, 0, 50, 100, 10000, 10049), (50, 0, 1, 1, 50, 5000, 5049)]),
         (100, [(100, 0, 0, 51, 100, 10000, 10049), (50, 0, 1, 1, 50, 5000, 5049)])], ([0, -1, 4], [1, -1, 5]))
    small, over, good = (80, 0, 2, 51, 55, 1, 5), (80, 0, 2, 30, 100, 1, 71), (60, 0, 1, 51, 100, 5000, 5049)
    add("better_row_fails_each_cov", "a better row that fails each_cov does not hide a worse row that passes, in front of s0 and behind it",
        [(100, [small, A, good]), (100, [A, small, good]), (100, [A, good, small])], ([1, 3, 6], [2, 5, 7]))
    add("better_row_fails_overlap", "a better row that fails the overlap test does not hide a worse row that passes, in front of s0 and behind it",
        [(100, [over, A, good]), (100, [A, over, good]), (100, [A, good, over])], ([1, 3, 6], [2, 5, 7]))
    add("tie_for_s0", "equal score and edit distance: the earlier row is s0; a smaller edit distance wins at equal score",
        [(100, [(70, 1, 0, 1, 50, 10000, 10049), (70, 1, 1, 51, 100, 5000, 5049)]), (100, [(70, 1, 0, 1, 50, 10000, 10049), (70, 0, 1, 51, 100, 5000, 5049)])], ([0, 3], [1, 2]))
    add("tie_for_s1", "equal score and edit distance among the second parts: the earlier row; a smaller edit distance wins at equal score",
        [(100, [A, (50, 2, 1, 51, 100, 5000, 5049), (50, 2, 2, 51, 100, 7000, 7049)]), (100, [A, (50, 2, 1, 51, 100, 5000, 5049), (50, 1, 2, 51, 100, 7000, 7049)]),
         (100, [(50, 2, 1, 51, 100, 5000, 5049), (50, 2, 2, 51, 100, 7000, 7049), A])], ([0, 3, 8], [1, 5, 6]))
    add("third_row_would_cover", "the second part passes every test and the two cover too little: no candidate, though a third row covers the rest (the reference returns 3)",
        [(100, [(100, 0, 0, 1, 40, 10000, 10039), (50, 0, 1, 41, 70, 5000, 5029), (40, 0, 2, 71, 100, 7000, 7029)]),
         (100, [(100, 0, 0, 1, 40, 10000, 10039), (40, 0, 1, 41, 70, 5000, 5029), (50, 0, 2, 41, 100, 7000, 7059)])], ([-1, 3], [-1, 5]))
    add("spans_beyond_rlen", "spans past the read's length (hard clips) count inside [1, rlen] only",
        [(100, [A, (50, 0, 1, 51, 120, 5000, 5069)]), (100, [A, (50, 0, 1, 101, 150, 5000, 5049)]), (100, [(100, 0, 0, -9, 50, 10000, 10059), (50, 0, 1, 51, 100, 5000, 5049)]),
         (100, [(100, 0, 0, 1, 48, 10000, 10047), (50, 0, 1, 51, 160, 5000, 5109)])], ([0, -1, 4, -1], [1, -1, 5, -1]))
    add("rlen_0_and_negative", "a group whose read length is 0 or negative is no candidate", [(0, [A, B]), (-7, [A, B]), (100, [A, B])], ([-1, -1, 4], [-1, -1, 5]))
    add("empty_spans", "a second part whose end lies in front of its start covers nothing and fails each_cov", [(100, [A, (50, 0, 1, 60, 50, 5000, 5049), (40, 0, 1, 51, 100, 5000, 5049)])], ([0], [2]))
    for n in (255, 256, 257):
        groups = [(100, [A, B]) if (g % 3 != 1 or g == n - 1) else (100, [A, (50, 0, 0, 51, 100, 10040, 10089)]) for g in range(n)]
        add("%d_groups" % n, "the last workgroup is full, one short and one over; the last group is a candidate", groups)
    return c


# ------------------------------------------------------------------------------------------------ family g: rejected arguments

# The pointers of each entry point in the order tests/filter_dump.hip nulls them by mask bit
POINTERS = {
    "l2r_filter_score": ("ctx", "recs", "prm", "drop", "score", "intron_n", "flag", "tid", "pos", "l_qseq", "nm", "cig_off", "cig"),
    "l2r_filter_select": ("ctx", "prm", "group_off", "score", "intron_n", "winner"),
    "l2r_fusion_segments": ("ctx", "recs", "read_start", "read_end", "ref_start", "ref_end", "qlen", "flag", "pos", "cig_off", "cig"),
    "l2r_fusion_select": ("ctx", "prm", "group_off", "score", "ed", "tid", "read_start", "read_end", "ref_start", "ref_end", "rlen_of_group", "first", "second"),
}
ENTRY_ID = {"l2r_filter_score": 1, "l2r_filter_select": 2, "l2r_fusion_segments": 3, "l2r_fusion_select": 4}


def family_g() -> List[Case]:
    """inputs: entry, n (records or groups), n_cigar, off (cig_off / group_off), null (names of POINTERS handed over as NULL),
    null_spans; hand: the message, or None where the call has to return 0 and leave its outputs alone."""
    c = []

    def add(name, rule, entry, n, off, message, n_cigar=None, null=(), null_spans=False):
        c.append(Case("g", name, rule, "args", entry=entry, n=n, n_cigar=(off[-1] if off else 0) if n_cigar is None else n_cigar, off=list(off), null=tuple(null),
                      null_spans=null_spans, hand=message))

    for entry in ("l2r_filter_score", "l2r_fusion_segments"):
        e = entry[4:]
        add(e + "_ok", "arguments in order", entry, 2, [0, 1, 2], None)
        add(e + "_n_0", "no record: 0, the outputs untouched", entry, 0, [0], None)
        add(e + "_n_0_null_columns", "no record: the columns are not looked at", entry, 0, [], None, null=("flag", "pos", "cig_off", "cig"))
        for p in ("ctx", "recs") + (("prm", "drop", "intron_n") if entry == "l2r_filter_score" else ("read_start", "qlen")):
            add(e + "_null_" + p, "a null argument", entry, 2, [0, 1, 2], "[%s] null argument" % entry, null=(p,))
        add(e + "_negative_n", "a negative record count", entry, -1, [0], "[%s] negative size" % entry)
        add(e + "_negative_n_cigar", "a negative operation count", entry, 2, [0, 1, 2], "[%s] negative size" % entry, n_cigar=-2)
        for p in ("flag", "pos", "cig_off", "cig") + (("tid", "l_qseq", "nm") if entry == "l2r_filter_score" else ()):
            add(e + "_null_column_" + p, "a null column", entry, 2, [0, 1, 2], "[%s] null column" % entry, null=(p,))
        add(e + "_no_cigar_words", "no operation at all: a null cig is in order", entry, 2, [0, 0, 0], None, null=("cig",))
        add(e + "_first_offset", "cig_off that does not start at 0", entry, 2, [1, 2, 3], "[%s] cig_off does not span the CIGAR array" % entry, n_cigar=3)
        add(e + "_last_offset", "cig_off that does not end at n_cigar", entry, 2, [0, 1, 2], "[%s] cig_off does not span the CIGAR array" % entry, n_cigar=3)
        add(e + "_descends", "cig_off [0, 10, 5] with 5 operations: record 0 would read five words beyond the array", entry, 2, [0, 10, 5],
            "[%s] cig_off descends at record 1" % entry, n_cigar=5)
        add(e + "_descends_late", "a descent in the last place of three", entry, 3, [0, 2, 4, 3], "[%s] cig_off descends at record 2" % entry, n_cigar=3)
    add("filter_score_null_span_column", "a span table with transcripts and no columns", "l2r_filter_score", 2, [0, 1, 2], "[l2r_filter_score] null span column", null_spans=True)
    for entry in ("l2r_filter_select", "l2r_fusion_select"):
        e = entry[4:]
        add(e + "_ok", "arguments in order", entry, 2, [0, 1, 3], None)
        add(e + "_n_0", "no group: 0, the outputs untouched", entry, 0, [0], None)
        add(e + "_n_0_null_columns", "no group: the columns are not looked at", entry, 0, [], None, null=("group_off", "score"))
        for p in ("ctx", "prm", "group_off", "score") + (("intron_n", "winner") if entry == "l2r_filter_select" else ("ed", "rlen_of_group", "first", "second")):
            add(e + "_null_" + p, "a null argument", entry, 2, [0, 1, 3], "[%s] bad argument" % entry, null=(p,))
        add(e + "_negative_n", "a negative group count", entry, -1, [0], "[%s] bad argument" % entry)
        add(e + "_negative_offset", "a group offset below 0", entry, 2, [-1, 1, 3], "[%s] negative group offset" % entry)
        add(e + "_empty_group", "an empty group", entry, 3, [0, 1, 1, 3], "[%s] group 1 is empty" % entry)
        add(e + "_descending_group", "group offsets that descend", entry, 3, [0, 2, 3, 1], "[%s] group 2 is empty" % entry)
    return c


def all_cases() -> List[Case]:
    return family_a() + family_b() + family_c() + family_d() + family_e() + family_f() + family_g()


def by_family(*families) -> List[Case]:
    return [c for c in all_cases() if c.family in families]
