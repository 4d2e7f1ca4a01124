"""Cases of the read lists shared by tests/test_read_lists_cpu.py and tests/test_gpu_read_lists.py: a generator of case dicts in the form
tests/read_list_restatement.py reads, the hand-made piece patterns, names and domain errors, the case file of tests/lists_dump.hip, and
the calls that take a case through capi.Engine."""
import struct

import numpy as np

from lr2rmats_amd import capi
from tests import read_list_restatement as rr

ALPHABET = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.:/-", np.uint8)
# info words of the classes (include/lr2rmats_hip.h: L2R_INFO_*), without the exon count
KNOWN = 0x04 | 0x01
UNRECOG = 0x04
NOVEL_PASS = 0x04 | 0x02 | 0x20 | 0x40 | 0x80
NOVEL_FAIL = 0x04 | 0x02 | 0x20 | 0x10          # the split candidates of a run with a junction table
NOVEL_UNCHECKED = 0x04 | 0x02
PARTIAL = (0x00, 0x01, 0x02, 0x03)              # not FULL: in no list but ALL
REV = 0x08
CLASSES = (KNOWN, UNRECOG, NOVEL_PASS, NOVEL_FAIL, NOVEL_UNCHECKED) + PARTIAL
NJ, UJ = 0x08, 0x10                             # L2R_EXF_NOVEL_JUNC, L2R_EXF_UNREL_JUNC
REFS = (b"c", b"chr2", b"chrUn_KI270302v1_random")      # reference 0: 1 byte; reference 2: 23 bytes


def make_case(seed, exons, info="mixed", flags="random", refs=REFS, n_tx=9, name_len=(1, 24), gene_len=(0, 16), no_ref=0.3, has_sj=True, split=True, tid_name=False,
              coord_max=250000000, src=b"lr2rmats"):
    """A case of len(exons) reads with exons[i] exons each.  info: "mixed", one class word, or a sequence of them (cycled; the strand is
    drawn); flags: "random", "pieces" (junction flags that make pieces likely), or one byte for every exon."""
    rng = np.random.default_rng(seed)
    exons = np.asarray(exons, np.int64)
    n = len(exons)
    ex_off = np.zeros(n + 1, np.int64)
    ex_off[1:] = np.cumsum(exons)
    X = int(ex_off[-1])
    xs, xe = np.zeros(X, np.int32), np.zeros(X, np.int32)
    for i in range(n):
        k = int(exons[i])
        if k:
            steps = rng.integers(1, max(2, coord_max // (2 * k + 1)), 2 * k).astype(np.int64)
            steps[0] = rng.choice([1, 7, 95, 99990, steps[0]])
            c = np.cumsum(steps)
            xs[ex_off[i]:ex_off[i + 1]] = c[0::2]
            xe[ex_off[i]:ex_off[i + 1]] = c[1::2]
    if isinstance(flags, str) and flags == "random":
        dens = rng.choice([0.0, 0.05, 0.5, 1.0], n)
        f = ((rng.random((X, 5)) < np.repeat(dens, exons)[:, None]).astype(np.uint8) @ np.asarray([1, 2, 4, 8, 16], np.uint8)).astype(np.uint8)
    elif isinstance(flags, str):
        f = (rng.choice([0, NJ, 0, NJ, UJ, NJ | UJ], X).astype(np.uint8) | rng.choice([0, 1, 2, 4], X).astype(np.uint8)).astype(np.uint8)
    else:
        f = np.full(X, flags, np.uint8)

    def name(lens):
        return bytes(rng.choice(ALPHABET, int(rng.integers(lens[0], lens[1] + 1))))
    table = [name(name_len) for _ in range(n)] + ([b"T." + name(name_len) for _ in range(n)] if tid_name else [])
    names, ids = rr.pack_table(table)
    anno, gids = rr.pack_table([name(gene_len) for _ in range(2 * n_tx)])
    ref_tx = rng.integers(0, max(n_tx, 1), n).astype(np.int32)
    ref_tx[rng.random(n) < no_ref] = -1
    if n_tx == 0:
        ref_tx[:] = -1
    if isinstance(info, str):
        cls = rng.choice(CLASSES, n)
    else:
        cls = np.resize(np.atleast_1d(np.asarray(info, np.int64)), n)
    word = (cls.astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) * REV) | (exons.astype(np.uint32) << 8)).astype(np.uint32)
    return {"refs": [bytes(r) for r in refs], "src": bytes(src), "tid": rng.integers(0, len(refs), n).astype(np.int32), "names": names,
            "qname": np.asarray(ids[:n], np.uint32), "tid_name": np.asarray(ids[n:], np.uint32) if tid_name else None,
            "anno": anno, "tx_gid": np.asarray(gids[:n_tx], np.uint32), "tx_gname": np.asarray(gids[n_tx:], np.uint32), "ex_off": ex_off, "xs": xs, "xe": xe, "f": f,
            "info": word, "ref_tx": ref_tx, "has_sj": bool(has_sj), "split": bool(split)}


def flag_case(seed, rows, info=NOVEL_FAIL, rev=None, **kw):
    """One read per row of exon flags, all of class ``info``; rev: the strand of every read (None: drawn)."""
    case = make_case(seed, [len(r) for r in rows], info=info, flags=0, **kw)
    case["f"] = np.concatenate([np.asarray(r, np.uint8) for r in rows]) if rows else np.zeros(0, np.uint8)
    if rev is not None:
        case["info"] = ((case["info"] & ~np.uint32(REV)) | np.uint32(REV if rev else 0)).astype(np.uint32)
    return case


# the piece patterns: flags of one read -> its pieces (first, last)
MANY = [NJ, UJ] * 12 + [NJ, 0, 0]                         # 12 two-exon pieces and one of three exons: suffixes .split.0 to .split.12
PATTERNS = [
    ([NJ, 0, NJ, 0, 0], [(0, 4)]),                        # no unreliable junction: the read is one piece
    ([NJ | UJ, UJ, NJ | UJ, UJ, 0], []),                  # every junction unreliable: one-exon remainders only
    ([UJ, NJ, 0, 0], [(1, 3)]),                           # a cut at the first junction
    ([NJ, 0, UJ, 0], [(0, 2)]),                           # a cut at the last junction; the one-exon remainder is dropped
    ([NJ, NJ, NJ, 0], []),                                # only novel junctions
    ([0, 0, 0, 0], []),                                   # only known junctions
    ([NJ, NJ | UJ, 0, 0, UJ, NJ, 0, 0], [(5, 7)]),        # a run of novel junctions only [0, 1] and one of known only [2, 4] are dropped; [5, 7] has both
    ([NJ, 0], []),                                        # two exons: one junction cannot be novel and known
    ([0], []),                                            # one exon
    (MANY, [(2 * k, 2 * k + 1) for k in range(12)] + [(24, 26)]),
]


def pattern_case(rev=None, **kw):
    return flag_case(11, [p for p, _ in PATTERNS], rev=rev, **kw)


def set_names(case, qnames, tid_names=None):
    table = list(qnames) + (list(tid_names) if tid_names is not None else [])
    case["names"], ids = rr.pack_table(table)
    n = len(qnames)
    case["qname"] = np.asarray(ids[:n], np.uint32)
    case["tid_name"] = np.asarray(ids[n:], np.uint32) if tid_names is not None else None


def case_file(case, first=0, max_blocks=1 << 20, max_bytes=1 << 30, sums_only=0):
    """The case file tests/lists_dump.hip reads."""
    n, refs = len(case["tid"]), case["refs"]
    ref_off = np.zeros(len(refs) + 1, np.int64)
    ref_off[1:] = np.cumsum([len(r) for r in refs])
    tn = case.get("tid_name")
    head = struct.pack("<16q", n, len(case["xs"]), len(case["names"]), 0 if tn is None else 1, len(refs), len(case["src"]), len(case["tx_gid"]), len(case["anno"]),
                       int(case["has_sj"]), int(case["split"]), first, max_blocks, max_bytes, sums_only, 0, 0)
    body = [np.asarray(case["tid"], np.int32), np.asarray(case["qname"], np.uint32), np.zeros(0, np.uint32) if tn is None else np.asarray(tn, np.uint32),
            np.frombuffer(case["names"], np.uint8), np.asarray(case["ex_off"], np.int64), np.asarray(case["info"], np.uint32), np.asarray(case["ref_tx"], np.int32),
            np.asarray(case["xs"], np.int32), np.asarray(case["xe"], np.int32), np.asarray(case["f"], np.uint8), ref_off, np.frombuffer(b"".join(refs), np.uint8),
            np.frombuffer(case["src"], np.uint8), np.frombuffer(case["anno"], np.uint8), np.asarray(case["tx_gid"], np.uint32), np.asarray(case["tx_gname"], np.uint32)]
    return head + b"".join(a.tobytes() for a in body)


def result_of(case):
    return capi.Result(np.asarray(case["ex_off"], np.int64), np.asarray(case["xs"], np.int32), np.asarray(case["xe"], np.int32), np.asarray(case["f"], np.uint8),
                       np.asarray(case["info"], np.uint32), np.asarray(case["ref_tx"], np.int32))


def engine_reads(eng, case):
    """begin, anno and reads with the case's results uploaded."""
    eng.gtftext_begin(case["refs"], case["src"], capi.GTX_READ)
    eng.gtftext_anno(case["anno"], case["tx_gid"], case["tx_gname"])
    eng.gtftext_reads(case["tid"], case["names"], case["qname"], case.get("tid_name"), result_of(case), case["has_sj"], case["split"])


def engine_list(eng, lst, max_blocks=1 << 20, max_bytes=1 << 30):
    """One list of the reads last given: (selection as a list of tuples, text, (m, n_lines, n_bytes), the stats after the last batch)."""
    m, n_lines, n_bytes = eng.gtftext_list(lst)
    cols = eng.gtftext_list_out(m)
    sel = list(zip(*[c.tolist() for c in cols])) if m else []
    text = eng.gtftext_all(m, max_blocks, max_bytes)
    return sel, text, (m, n_lines, n_bytes), eng.gtftext_stats()


# ---------------------------------------------------------------------------------------------------- the cases both suites run

def class_cases():
    """Every class alone, mixed and alternating, and has_sj x split over the mixed reads."""
    rng = np.random.default_rng(3)
    exons = rng.choice([1, 2, 2, 3, 5, 8, 13, 40], 90)
    out = [make_case(20 + k, exons[:40], info=c, flags="pieces") for k, c in enumerate((KNOWN, UNRECOG, NOVEL_PASS, NOVEL_FAIL, NOVEL_UNCHECKED, 0))]
    out.append(make_case(30, exons, info=(KNOWN, NOVEL_FAIL), flags="pieces"))                                      # alternating
    out.append(make_case(31, exons, info=(NOVEL_FAIL, UNRECOG, NOVEL_PASS), flags="pieces", tid_name=True))
    for has_sj in (False, True):
        for split in (False, True):
            out.append(make_case(32, exons, flags="pieces", has_sj=has_sj, split=split))
    out.append(make_case(33, exons, flags="random", n_tx=0))                                                        # every ref < 0
    out.append(make_case(34, [], flags=0))                                                                          # no read
    return out


def piece_cases():
    return [pattern_case(), pattern_case(rev=True), pattern_case(rev=False, tid_name=True), pattern_case(has_sj=False), pattern_case(split=False),
            flag_case(12, [[NJ, 0, UJ] * 100]),                                                                     # a split candidate of 300 exons
            flag_case(13, [[NJ, 0, UJ] * 100] + [[NJ, 0, 0]] * 5 + [[0]] * 3, info=(NOVEL_FAIL, KNOWN, NOVEL_FAIL))]


def name_cases():
    out = []
    for k in (0, 1, 254):
        out.append(make_case(40 + k, [1, 3, 2, 70, 1], info=(KNOWN, UNRECOG, NOVEL_PASS), name_len=(k, k), gene_len=(k, k), no_ref=0.0, tid_name=k == 1))
        out.append(make_case(50 + k, [1, 3, 2, 70, 1], info=(KNOWN, UNRECOG, NOVEL_PASS), name_len=(k, k), no_ref=1.0))
    # an empty gene id beside a gene name, and the other way round
    c = make_case(60, [2, 2, 3], info=KNOWN, no_ref=0.0, n_tx=2)
    c["anno"], ids = rr.pack_table([b"", b"GID", b"GNAME", b""])
    c["tx_gid"], c["tx_gname"] = np.asarray(ids[:2], np.uint32), np.asarray(ids[2:], np.uint32)
    c["ref_tx"] = np.asarray([0, 1, -1], np.int32)
    out.append(c)
    # piece names of 99 bytes: `.split.0` behind 91 bytes, `.split.10` behind 90
    p = flag_case(61, [PATTERNS[0][0], MANY])
    set_names(p, [b"q" * 91, b"r" * 90])
    out.append(p)
    p = flag_case(62, [PATTERNS[0][0]], tid_name=True)
    set_names(p, [b"q" * 5], [b"t" * 91])
    out.append(p)
    return out


def error_cases():
    """(case, list, block, kind): one domain error each, and pairs that pin the order of the kinds and the smallest block."""
    out = []

    def base(seed=70, info=KNOWN, **kw):
        return make_case(seed, [2, 3, 1, 4, 2, 5], info=info, no_ref=0.0, name_len=(3, 9), gene_len=(2, 6), **kw)
    c = base(); c["tid"][3] = -1; out.append((c, rr.ALL, 3, "tid"))
    c = base(); c["tid"][4] = len(c["refs"]); out.append((c, rr.KNOWN, 4, "tid"))
    c = make_case(71, [2, 0, 3], info=KNOWN); out.append((c, rr.ALL, 1, "noexon"))
    c = make_case(71, [2, 0, 3], info=KNOWN); c["tid"][1] = 99; out.append((c, rr.ALL, 1, "tid"))                  # tid in front of noexon
    c = base(); c["ref_tx"][2] = len(c["tx_gid"]); out.append((c, rr.ALL, 2, "ref"))
    c = make_case(71, [2, 0, 3], info=KNOWN); c["ref_tx"][1] = 1000; out.append((c, rr.ALL, 1, "noexon"))          # noexon in front of ref
    # the names, each with its three tests: g and G in the annotation's table, t and T in the reads'
    for col, where in (("tx_gid", "anno"), ("tid_name", "names"), ("tx_gname", "anno"), ("qname", "names")):
        for kind in ("name_id", "name_long", "name_nul"):
            c = base(72, tid_name=True)
            table = c[where]
            if kind == "name_id":
                at = len(table)
            elif kind == "name_long":
                at, table = len(table), table + b"L" * 255 + b"\0"
            else:
                at, table = len(table), table + b"noend"
            c[where] = table
            row = 2
            if where == "anno":
                c["ref_tx"][row] = 5
                c[col][5] = at
            else:
                c[col][row] = at
            out.append((c, rr.ALL, row, kind))
    # g in front of T, t in front of G
    c = base(73, tid_name=True); c["ref_tx"][1] = 0; c["tx_gid"][0] = len(c["anno"]); c["names"] += b"x" * 300; c["qname"][1] = len(c["names"]) - 290
    out.append((c, rr.ALL, 1, "name_id"))
    c = base(73, tid_name=True); c["ref_tx"][1] = 0; c["anno"] += b"x" * 300; c["tx_gname"][0] = len(c["anno"]) - 290; c["tid_name"][1] = len(c["names"])
    out.append((c, rr.ALL, 1, "name_id"))
    # a piece name of 100 bytes, through T and through t; with a two-digit suffix only the eleventh piece
    p = flag_case(74, [PATTERNS[0][0], [NJ, 0]]); set_names(p, [b"q" * 92, b"ok"]); out.append((p, rr.NOVEL, 0, "piece_name"))
    p = flag_case(74, [PATTERNS[0][0]], tid_name=True); set_names(p, [b"q"], [b"t" * 92]); out.append((p, rr.NOVEL, 0, "piece_name"))
    p = flag_case(74, [MANY]); set_names(p, [b"q" * 91]); out.append((p, rr.NOVEL, 10, "piece_name"))
    p = flag_case(74, [PATTERNS[0][0]]); set_names(p, [b"q" * 92]); p["xs"][1] = -5; out.append((p, rr.NOVEL, 0, "piece_name"))     # in front of neg
    c = base(); c["xs"][int(c["ex_off"][3]) + 2] = -1; out.append((c, rr.ALL, 3, "neg"))
    c = base(); c["xe"][int(c["ex_off"][5])] = -7; out.append((c, rr.KNOWN, 5, "neg"))
    # the smallest block, whatever its kind; and a list that does not hold the bad read is sound
    c = base(); c["xs"][int(c["ex_off"][2])] = -1; c["tid"][4] = -3; out.append((c, rr.ALL, 2, "neg"))
    c = base(75, info=(KNOWN, UNRECOG)); c["tid"][1] = -3; c["tid"][5] = -3; out.append((c, rr.UNRECOG, 0, "tid"))  # read 1 is block 0 of its list
    # a piece's exons alone are looked at: a negative coordinate outside every piece is no error of the novel list
    return out


def sound_lists(case, lst, block):
    """The lists of an error case that do not hold the bad read."""
    return [l for l in rr.LISTS if l != lst and rr.error(case, l) is None]
