"""The novel list of `update-gtf` (l2r_novel_*), restated in plain Python from the rule as include/lr2rmats_hip.h states it and from the
literal loops of the host tail (summary_and_bed, add_gene) -- not from the unit's code: the offers in input order to one
tests/uniq_restatement.merge list, the items of the six lists from the entries' widened chains, and every list's backward scan: an equal
key first, then the stop at a smaller tid (a gene list compares the gene alone).  A read is (tid, info bits, ref, [(start, end, flags),
...]); its strand is the REV bit."""
import numpy as np

from tests import uniq_restatement as ur

KNOWN, KNOWN_SITE, FULL, REV, UNREL, SJ_CHECKED, SJ_PASS = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40      # L2R_INFO_*
NE, ND, NA, NJ, UJ = 1, 2, 4, 8, 16                                                                      # L2R_EXF_*
EXON, DON, ACC, JUNC, GENE, KNOWN_GENE = range(6)
KINDS = ("a tid outside the reference table", "no exon", "ref at or beyond the annotation's transcripts", "a negative coordinate")


def candidate(bits):
    return bool(bits & FULL) and not bits & KNOWN and bool(bits & KNOWN_SITE)


def is_offer(bits, has_sj):
    return candidate(bits) and (not has_sj or bool(bits & SJ_PASS))


def is_split(bits, has_sj, split):
    return candidate(bits) and bool(has_sj) and not bits & SJ_PASS and bool(split)


def bits_of(reads, has_sj=0, split=0):
    """Per read: 1 offer, 2 known, 4 split-route."""
    return [(1 if is_offer(b, has_sj) else 0) | (2 if b & KNOWN else 0) | (4 if is_split(b, has_sj, split) else 0) for _t, b, _r, _c in reads]


def bad_read(reads, n_ref, n_tx, has_sj=0):
    """None, or (the smallest read outside the domain, the first of its kinds)."""
    for i, (tid, bits, ref, chain) in enumerate(reads):
        if tid < 0 or tid >= n_ref:
            return i, KINDS[0]
        if not chain:
            return i, KINDS[1]
        if ref >= n_tx:
            return i, KINDS[2]
        if is_offer(bits, has_sj) and any(s < 0 or e < 0 for s, e, _f in chain):
            return i, KINDS[3]
    return None


def gene(ref, tx_gene, na_gene):
    return int(na_gene) if ref < 0 else int(tx_gene[ref])


def scan(rows, key, gene_list=False):
    """The backward scan of one list: the row that takes the item, or None."""
    for k in range(len(rows) - 1, -1, -1):
        if (rows[k][1] == key[1]) if gene_list else (rows[k][:3] == list(key)):
            return k
        if key[0] > rows[k][0]:
            break
    return None


def novel(reads, tx_gene=(), na_gene=0, has_sj=0, split=0, ref_names=None, **merge):
    """The entries, the kept rows of the six lists ([tid, a, b, score, meta]), the items per list, the eight counts and the BED text."""
    offers = [i for i, r in enumerate(reads) if is_offer(r[1], has_sj)]
    trans = [(reads[i][0], 1 if reads[i][1] & REV else 0, [(s, e) for s, e, _f in reads[i][3]]) for i in offers]
    m = ur.merge(trans, **merge)
    rows = [[] for _ in range(6)]
    items = [0] * 6
    widened = 0
    for e in range(len(m["u_src"])):
        i = offers[int(m["u_src"][e])]
        tid, bits, ref, chain = reads[i]
        n, cov, rev = len(chain), int(m["u_cov"][e]), 1 if bits & REV else 0
        xs, xe, f = [c[0] for c in chain], [c[1] for c in chain], [c[2] for c in chain]
        widened += xs[0] != int(m["u_start"][e]) or xe[-1] != int(m["u_end"][e])
        xs[0], xe[-1] = int(m["u_start"][e]), int(m["u_end"][e])
        items[GENE] += 1
        g = gene(ref, tx_gene, na_gene)
        if scan(rows[GENE], (tid, g, 0), True) is None:
            rows[GENE].append([tid, g, 0, 0, 0])
        for j in range(n):
            if f[j] & NE:
                items[EXON] += 1
                k = scan(rows[EXON], (tid, xs[j], xe[j]))
                if k is not None:
                    rows[EXON][k][3] += cov
                else:
                    rows[EXON].append([tid, xs[j], xe[j], cov, ((0 if j in (0, n - 1) else 1) if n > 1 else 2) | rev << 2])
        for lst, bit in ((DON, ND), (ACC, NA), (JUNC, NJ)):
            for j in range(n - 1):
                if f[j] & bit:
                    items[lst] += 1
                    key = (tid, xe[j], 0) if lst == DON else (tid, xs[j + 1], 0) if lst == ACC else (tid, xe[j], xs[j + 1])
                    if scan(rows[lst], key) is None:
                        rows[lst].append(list(key) + [0, 0])
    for tid, bits, ref, _chain in reads:
        if bits & KNOWN:
            items[KNOWN_GENE] += 1
            g = gene(ref, tx_gene, na_gene)
            if scan(rows[KNOWN_GENE], (tid, g, 0), True) is None:
                rows[KNOWN_GENE].append([tid, g, 0, 0, 0])
    kept = [len(r) for r in rows]
    text = b""
    if ref_names is not None:
        text = b"".join(bytes(ref_names[t]) + ("\t%d\t%d\t%s_exon\t%d\t%s\n" % (s - 1, e, "TIS"[meta & 3], score, "+-"[meta >> 2 & 1])).encode() for t, s, e, score, meta in rows[EXON])
    return {"entries": {"src": [offers[int(k)] for k in m["u_src"]], "start": [int(v) for v in m["u_start"]], "end": [int(v) for v in m["u_end"]], "cov": [int(v) for v in m["u_cov"]]},
            "rows": rows, "items": items, "counts": [kept[GENE], len(m["u_src"]), 0, kept[EXON], kept[DON] + kept[ACC], kept[JUNC], 0, kept[KNOWN_GENE]],
            "bed": text, "hits": int(m["hits"].sum()), "widened": int(widened), "offers": len(offers), "known": items[KNOWN_GENE],
            "split": sum(1 for r in reads if is_split(r[1], has_sj, split))}


def in_order(reads, has_sj=0):
    """(tid, start) does not descend over the offers, tid does not descend over the known reads."""
    o = [(r[0], r[3][0][0]) for r in reads if is_offer(r[1], has_sj)]
    k = [r[0] for r in reads if r[1] & KNOWN]
    return all(o[i - 1] <= o[i] for i in range(1, len(o))) and all(k[i - 1] <= k[i] for i in range(1, len(k)))


def columns(reads):
    """tid, info (the bits and the exon count from bit 8 on), ref_tx, xs, xe, flags."""
    tid = np.asarray([r[0] for r in reads], np.int32)
    info = np.asarray([(r[1] & 0xff) | len(r[3]) << 8 for r in reads], np.uint32)
    ref = np.asarray([r[2] for r in reads], np.int32)
    xs = np.asarray([e[0] for r in reads for e in r[3]], np.int32)
    xe = np.asarray([e[1] for r in reads for e in r[3]], np.int32)
    f = np.asarray([e[2] for r in reads for e in r[3]], np.uint8)
    return tid, info, ref, xs, xe, f
