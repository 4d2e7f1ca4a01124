"""The rule of the detail table of `update-gtf -A` (include/lr2rmats_hip.h, l2r_detail_*), restated in Python from the rule alone: one
line per read, the domain errors in the order they are looked for, and the batch cut.  A case is a dict of ``refs`` (byte strings by tid),
``tid``, ``names`` (a table of NUL-terminated strings) with ``qname`` (byte offsets), the annotation's ``anno`` table with ``tx_gid`` and
``tx_gname``, and the result arrays ``ex_off``, ``xs``, ``xe``, ``f``, ``info`` and ``ref_tx``."""
import json

import numpy as np

BATCH_BYTES = (1 << 32) - 64
NAME_MAX = 254
I_KNOWN, I_KNOWN_SITE, I_REV = 1, 2, 8
F_EXON, F_DON, F_ACC, F_JUNC, F_UNREL = 1, 2, 4, 8, 16
KINDS = ("tid", "qname_id", "qname_long", "qname_nul", "ref", "gene_id", "gene_long", "gene_nul", "noexon", "neg", "big")
KIND_CODE = {k: i + 1 for i, k in enumerate(KINDS)}                                         # DET_E_* of l2r_detailplan.hip.h
KIND_TEXT = {"tid": "a reference outside the table", "qname_id": "a read-name id at or beyond names_len", "qname_long": "a read name of 255 or more bytes",
             "qname_nul": "a read name without a NUL inside the table", "ref": "a transcript index at or beyond the annotation's transcripts",
             "gene_id": "a gene id or gene name id at or beyond anno_names_len", "gene_long": "a gene id or gene name of 255 or more bytes",
             "gene_nul": "a gene id or gene name without a NUL inside the table", "noexon": "a read with no exon", "neg": "a negative exon start or end",
             "big": "its line reaches 2^32 - 64 bytes"}
HEADER = (b"ReadName\tchr\tstrand\tNovel\tGeneID\tGeneName\tExonCount\tExonStart\tExonEnd\tNovelExonCount\tNovelExonIndex\tNovelSiteCount\tNovelSiteIndex\t"
          b"NovelJunctionCount\tNovelJunctionIndex\tUnreliableJunctionCount\tUnreliableJunctionIndex\n")


class Domain(Exception):
    def __init__(self, kind):
        Exception.__init__(self, kind)
        self.kind = kind


def pack_table(strings):
    """(table, ids) of a list of byte strings: every distinct string once, NUL-terminated."""
    table, at, ids = bytearray(), {}, []
    for s in strings:
        s = bytes(s)
        if s not in at:
            at[s] = len(table)
            table += s + b"\0"
        ids.append(at[s])
    return bytes(table), ids


def name_of(table, i, what):
    if i >= len(table):
        raise Domain(what + "_id")
    end = table.find(b"\0", i, i + NAME_MAX + 1)
    if end < 0:
        raise Domain(what + "_long" if i + NAME_MAX + 1 <= len(table) else what + "_nul")
    return table[i:end]


def index_list(members, last):
    """<count>\\t and the members comma separated, or NA; a tab behind it -- behind the last list only where it is empty."""
    if not members:
        return b"0\tNA\t"
    return b"%d\t" % len(members) + b",".join(b"%d" % m for m in members) + (b"" if last else b"\t")


def lists(f, n):
    """The members of L1..L4 over the flags of a read's n exons."""
    l1 = [j for j in range(n) if f[j] & F_EXON]
    l2 = []
    for j in range(n - 1):
        if f[j] & F_DON:
            l2.append(2 * j)
        if f[j] & F_ACC:
            l2.append(2 * j + 1)
    l3 = [j for j in range(n - 1) if f[j] & F_JUNC]
    l4 = [j for j in range(n - 1) if f[j] & F_UNREL]
    return l1, l2, l3, l4


def segments(case, i, sizes_only=False):
    """The seven segments of read i's line (head, starts, ends, L1..L4), or Domain.  sizes_only: a read of millions of exons is not walked
    for its text -- byte counts stand for the coordinate lists (the flags must then be zero)."""
    tid = int(case["tid"][i])
    if tid < 0 or tid >= len(case["refs"]):
        raise Domain("tid")
    q = name_of(case["names"], int(case["qname"][i]), "qname")
    ref = int(case["ref_tx"][i])
    if ref >= len(case["tx_gid"]):
        raise Domain("ref")
    if ref < 0:
        gid = gname = b"NA"
    else:
        gid = name_of(case["anno"], int(case["tx_gid"][ref]), "gene")
        gname = name_of(case["anno"], int(case["tx_gname"][ref]), "gene")
    info = int(case["info"][i])
    n, o = info >> 8, int(case["ex_off"][i])
    if n < 1:
        raise Domain("noexon")
    xs, xe, f = np.asarray(case["xs"][o:o + n]), np.asarray(case["xe"][o:o + n]), np.asarray(case["f"][o:o + n])
    if (xs < 0).any() or (xe < 0).any():
        raise Domain("neg")
    cls = 0 if info & I_KNOWN else 1 if info & I_KNOWN_SITE else 2
    head = b"\t".join([q, case["refs"][tid], b"-" if info & I_REV else b"+", b"%d" % cls, gid, gname, b"%d" % n]) + b"\t"
    if sizes_only and n > 100000:
        assert not f.any()
        digits = lambda a: int(np.char.str_len(a.astype("U")).sum()) + n
        return [len(head), digits(xs), digits(xe), 5, 5, 5, 6]
    l1, l2, l3, l4 = lists(f.tolist(), n)
    return [head, b",".join(b"%d" % v for v in xs.tolist()) + b"\t", b",".join(b"%d" % v for v in xe.tolist()) + b"\t",
            index_list(l1, False), index_list(l2, False), index_list(l3, False), index_list(l4, True) + b"\n"]


def line(case, i):
    s = segments(case, i)
    out = b"".join(s)
    if len(out) >= BATCH_BYTES:
        raise Domain("big")
    return out


def split(case, i):
    """Where the segments 1..6 begin in read i's line."""
    at, out = 0, []
    for s in segments(case, i)[:6]:
        at += len(s)
        out.append(at)
    return out


def texts(case):
    return [line(case, i) for i in range(len(case["tid"]))]


def text(case):
    return b"".join(texts(case))


def error(case, sizes_only=False):
    """(smallest read with a domain error, its kind), or None."""
    for i in range(len(case["tid"])):
        try:
            s = segments(case, i, sizes_only)
            if sum(x if isinstance(x, int) else len(x) for x in s) >= BATCH_BYTES:
                raise Domain("big")
        except Domain as e:
            return i, e.kind
    return None


def cut(lens, first, max_rows, max_bytes):
    """Rows one batch takes from ``first``: within max_rows, their bytes within max_bytes and below 2^32 - 64, but always one."""
    k, total = 0, 0
    while first + k < len(lens) and k < max_rows:
        b = int(lens[first + k])
        if k > 0 and (total + b > max_bytes or total + b >= BATCH_BYTES):
            break
        total += b
        k += 1
    return k


def from_json(path):
    """A hand-written case: reads as dicts of name, chr, info bits, ref, and exons as [start, end, flags]."""
    with open(path) as fh:
        j = json.load(fh)
    refs = [r.encode() for r in j["refs"]]
    anno, ids = pack_table([g.encode() for t in j["transcripts"] for g in t])
    names, qname = pack_table([r["name"].encode() for r in j["reads"]])
    ex = [e for r in j["reads"] for e in r["exons"]]
    off = np.zeros(len(j["reads"]) + 1, np.int64)
    off[1:] = np.cumsum([len(r["exons"]) for r in j["reads"]])
    return {"refs": refs, "tid": np.asarray([j["refs"].index(r["chr"]) for r in j["reads"]], np.int32), "names": names, "qname": np.asarray(qname, np.uint32),
            "anno": anno, "tx_gid": np.asarray(ids[0::2], np.uint32), "tx_gname": np.asarray(ids[1::2], np.uint32), "ex_off": off,
            "xs": np.asarray([e[0] for e in ex], np.int32), "xe": np.asarray([e[1] for e in ex], np.int32), "f": np.asarray([e[2] for e in ex], np.uint8),
            "info": np.asarray([r["info"] | len(r["exons"]) << 8 for r in j["reads"]], np.uint32), "ref_tx": np.asarray([r["ref"] for r in j["reads"]], np.int32)}
