"""TEST INFRASTRUCTURE ONLY -- `lr2rmats fusion` (reference src/bam_fusion.c, bam2seg of src/parse_bam.c:543-595) in its LITERAL
form, in plain Python over SAM text: a stable sort with the reference's comparator, the greedy loop of check_fusion() with
check_with_exist() over ALL segments selected so far, and a real coverage bitmap.  The kernel (csrc/l2r_fusion.hip.h) computes the
same decision in two passes (s0, then the first later segment that passes against s0); this file deliberately does not, so that
the tests tie the two forms together.

float / double: numpy.float32 wherever the reference has a `float` (the three options, ovlp_rat's and bam_seg_cov's return
values), Python floats (IEEE double) wherever it has a `double`.

Decisions of the build where the reference is undefined: equal (score, ed) keep file order; scores are
compared by value; the bitmap covers [1, rlen] and positions outside it are not written; rlen <= 0 is not a candidate; the
`printf("debug")` of parse_bam.c:556 is not reproduced.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import filter_oracle as fo

OVLP_FRAC, EACH_COV, ALL_COV, FUSION_DIS = 0.1, 0.1, 0.99, 100000            # src/bam_fusion.h:12-15
SITE_HEADER = "#fusion_id\t1st_chr\t1st_strand\tst_start_site\t1st_end_site\t2nd_chr\t2nd_strand\t2nd_start_site\t2nd_end_site\n"    # :173


class Seg:
    __slots__ = ("row", "tid", "is_rev", "score", "ed", "read_start", "read_end", "ref_start", "ref_end")

    def __init__(self, row, tid, is_rev, score, ed, read_start, read_end, ref_start, ref_end):
        self.row, self.tid, self.is_rev, self.score, self.ed = row, tid, is_rev, score, ed
        self.read_start, self.read_end, self.ref_start, self.ref_end = read_start, read_end, ref_start, ref_end


def aux_int(rec: fo.Record, tag: str) -> int:
    """bam_aux_get + bam_aux2i: the first tag of that name; its value for an integer type, 0 for another type or without the tag."""
    for a in rec.aux:
        if a.startswith(tag + ":"):
            return int(a[5:]) if a[3] == "i" else 0
    return 0


def query_len(cigar) -> int:
    """bam_query_len() src/parse_bam.c:261-270: M I S = X."""
    return sum(l for (l, op) in cigar if op in (0, 1, 4, 7, 8))


def bam2seg(rec: fo.Record, tid: int, row: int) -> Optional[Seg]:
    """src/parse_bam.c:543-595; None for an unmapped record."""
    if rec.flag & 4:
        return None
    rlen, is_rev = query_len(rec.cigar), (rec.flag & 16) != 0
    read_start, read_end, ref_start = 1, 0, rec.pos                            # rec.pos is 1-based = core.pos + 1
    ref_end = ref_start - 1
    for i, (l, op) in enumerate(rec.cigar):
        if op in (0, 7, 8):
            read_end += l; ref_end += l
        elif op == 1:
            read_end += l
        elif op in (2, 3):
            ref_end += l
        elif op in (4, 5):
            if i == 0:
                read_start += l; read_end += l
    if is_rev:
        read_start, read_end = rlen + 1 - read_end, rlen + 1 - read_start
    return Seg(row, tid, is_rev, aux_int(rec, "AS"), aux_int(rec, "NM"), read_start, read_end, ref_start, ref_end)


def seg_cmp(a: Seg, b: Seg) -> int:
    """seg_cmpfunc :61-65, by value."""
    if a.score != b.score:
        return -1 if a.score > b.score else 1
    return (a.ed > b.ed) - (a.ed < b.ed)


def ovlp_rat(start1, end1, start2, end2) -> np.float32:
    """:67-72"""
    if start1 > end2 or start2 > end1:
        return np.float32(0.0)
    overlap_len = end1 - start2 + 1 if end1 - start2 + 1 > 0 else end2 - start1 + 1
    min_len = min(end1 - start1 + 1, end2 - start2 + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(overlap_len) / np.float64(min_len + 0.0))


def check_with_exist1(s1: Seg, s2: Seg, ovlp_frac: np.float32, dis: int) -> bool:
    """:74-87"""
    if ovlp_rat(s1.read_start, s1.read_end, s2.read_start, s2.read_end) > ovlp_frac:
        return False
    if s1.tid == s2.tid:
        if ovlp_rat(s1.ref_start, s1.ref_end, s2.ref_start, s2.ref_end) > 0.0:
            return False
        if 0 < s1.ref_start - s2.ref_end < dis:
            return False
        if 0 < s2.ref_start - s1.ref_end < dis:
            return False
    return True


def bam_seg_cov(segs: Sequence[Seg], rlen: int) -> np.float32:
    """:98-112, the bitmap of calloc(rlen); a position outside [1, rlen] is not written (the reference writes out of bounds)."""
    m = np.zeros(rlen, np.uint8)
    for s in segs:
        for j in range(max(s.read_start, 1), min(s.read_end, rlen) + 1):
            m[j - 1] = 1
    return np.float32((int(m.sum()) + 0.0) / rlen)


def check_fusion(segs: List[Seg], rlen: int, ovlp_frac=OVLP_FRAC, each_cov=EACH_COV, all_cov=ALL_COV, dis=FUSION_DIS) -> Optional[List[Seg]]:
    """:114-129: the selected segments when the loop returns (their number is its return value), None for -1."""
    o, e, a = np.float32(ovlp_frac), np.float32(each_cov), np.float32(all_cov)
    if rlen <= 0:
        return None
    seg = sorted(segs, key=functools.cmp_to_key(seg_cmp))                       # stable: equal elements keep file order
    sel = [seg[0]]
    for s in seg[1:]:
        if (s.read_end - s.read_start + 1) / (rlen + 0.0) < float(e):
            continue
        if all(check_with_exist1(x, s, o, dis) for x in sel):
            sel.append(s)
            if bam_seg_cov(sel, rlen) >= a:
                return sel
    return None


def groups_of(recs: Sequence[fo.Record], tids: Sequence[int]):
    """The loop of bam_fusion() :175-204: [(name, rlen, [Seg...])] for every run of consecutive mapped records with one name."""
    out, lqname = [], None
    for i, rec in enumerate(recs):
        s = bam2seg(rec, tids[i], i)
        if s is None:                                                           # :176 continue
            continue
        if lqname is not None and rec.qname == lqname:
            out[-1][2].append(s)
        else:
            out.append((rec.qname, query_len(rec.cigar), [s]))
            lqname = rec.qname
    return out


def expected(sam_path: str, **opts) -> Tuple[bytes, List[Tuple[int, int]], str, int]:
    """(uncompressed BAM stream, [(record of seg[0], record of seg[1])], text of the -f file, count) of `lr2rmats fusion [opts] sam`."""
    header, refs, recs = fo.parse_sam(sam_path)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    names = [name for (name, _) in refs]
    tids = [-1 if r.rname == "*" else idx[r.rname] for r in recs]
    groups = groups_of(recs, tids)
    pairs, site = [], [SITE_HEADER]
    for gi, (name, rlen, segs) in enumerate(groups):
        if len(segs) < 2:                                                       # :181
            continue
        sel = check_fusion(segs, rlen, **opts)
        if sel is None or len(sel) != 2:                                        # :183
            continue
        pairs.append((sel[0].row, sel[1].row))
        if gi != len(groups) - 1:                                               # :196-204 write no site line for the last group
            l, r = (sel[0], sel[1]) if sel[0].read_start < sel[1].read_start else (sel[1], sel[0])      # fusion_write :132-142
            site.append("%s\t%s\t%s\t%d\t%d\t%s\t%s\t%d\t%d\n" % (name, names[l.tid], "+-"[l.is_rev], l.ref_start, l.ref_end,
                                                                  names[r.tid], "+-"[r.is_rev], r.ref_start, r.ref_end))
    stream = fo.header_bytes(header, refs) + b"".join(fo.encode_record(recs[i], idx) for p in pairs for i in p)
    return stream, pairs, "".join(site), len(pairs)
