"""The GTF block of `bam2gtf` and `unique-gtf`, restated in plain Python from the rule in include/lr2rmats_hip.h -- independent of the host
routine (csrc/l2r_gtftextplan.hip.h) and of the kernels (csrc/l2r_gtftext.hip.h), which the tests compare with it.

A case is a dict of columns: ``form`` (0 PLAIN, 1 READ), ``source`` and ``refs`` (bytes), per transcript ``tid``, ``rev``, ``ex_off`` (n + 1),
``xs`` / ``xe``, a names ``table`` (bytes, NUL-terminated strings) with the id columns ``gid``, ``tids``, ``gname``, ``tname`` (byte offsets),
and the selection: ``m`` blocks, ``sel`` / ``start`` / ``end`` / ``cov`` (each a list or None).  A golden file (tests/golden/gtf_text/*.json)
holds the names as strings per transcript; ``from_json`` packs them."""
import json

import numpy as np

PLAIN, READ = 0, 1
BATCH_BYTES = (1 << 32) - 64
KEYS = (b"gene_id", b"transcript_id", b"gene_name", b"transcript_name")
# kind -> what l2r_last_error() says of it
KIND_TEXT = {
    "sel": "a selection index outside the transcripts", "tid": "a reference outside the table", "noexon": "a transcript with no exon",
    "name_id": "a name id at or beyond names_len", "name_long": "a name of 255 or more bytes", "name_nul": "a name without a NUL inside the table",
    "neg": "a negative start, end, exon coordinate or coverage", "big": "its text reaches 2^32 - 64 bytes",
}


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


def from_json(path):
    with open(path) as fh:
        j = json.load(fh)
    n = len(j["tid"])
    cols = [j["gid"], j["tids"], j.get("gname") or [""] * n, j.get("tname") or [""] * n]
    table, ids = pack_table([s.encode() for c in cols for s in c])
    case = {"form": j["form"], "source": j["source"].encode(), "refs": [r.encode() for r in j["refs"]], "tid": j["tid"], "rev": j["rev"],
            "ex_off": j["ex_off"], "xs": j["xs"], "xe": j["xe"], "table": table,
            "gid": ids[:n], "tids": ids[n:2 * n], "gname": ids[2 * n:3 * n], "tname": ids[3 * n:],
            "sel": j.get("sel"), "start": j.get("start"), "end": j.get("end"), "cov": j.get("cov")}
    case["m"] = len(case["sel"]) if case["sel"] is not None else j.get("m", n)
    return case


def name_of(table, i):
    if i >= len(table):
        raise Domain("name_id")
    end = table.find(b"\0", i, i + 255)
    if end < 0:
        raise Domain("name_long" if i + 255 <= len(table) else "name_nul")
    return table[i:end]


def _pieces(case, q):
    """Block q: (ref, strand, A, C, S, E, exon pairs as printed, in the order printed) -- or Domain."""
    form = case["form"]
    t = q if case.get("sel") is None else int(case["sel"][q])
    if t < 0 or t >= len(case["tid"]):
        raise Domain("sel")
    tid = int(case["tid"][t])
    if tid < 0 or tid >= len(case["refs"]):
        raise Domain("tid")
    lo, hi = int(case["ex_off"][t]), int(case["ex_off"][t + 1])
    if hi - lo < 1:
        raise Domain("noexon")
    names = [name_of(case["table"], int(case[c][t])) for c in (("gid", "tids", "gname", "tname") if form == READ else ("gid", "tids"))]
    xs = np.asarray(case["xs"][lo:hi], np.int64).copy()
    xe = np.asarray(case["xe"][lo:hi], np.int64).copy()
    if case.get("start") is not None:
        xs[0] = int(case["start"][q])
    if case.get("end") is not None:
        xe[-1] = int(case["end"][q])
    cov = 1 if case.get("cov") is None else int(case["cov"][q])
    if xs[0] < 0 or xe[-1] < 0 or cov < 0 or (xs < 0).any() or (xe < 0).any():
        raise Domain("neg")
    rev = bool(case["rev"][t])
    if form == PLAIN:
        attr = b'gene_id "%s"; transcript_id "%s";' % (names[0], names[1])
        tail = b""
    else:
        attr = b"".join(b' %s "%s";' % (k, s) for k, s in zip(KEYS, names) if s)[1:]
        tail = b' transcript_cov "%d";' % cov
        if rev:
            xs, xe = xs[::-1], xe[::-1]
    S, E = (int(xs[-1]), int(xe[0])) if (form == READ and rev) else (int(xs[0]), int(xe[-1]))
    return case["refs"][tid], b"-" if rev else b"+", attr, tail, S, E, xs, xe


def block_bytes(case, q):
    """The bytes of block q without building its lines (a block of millions of exons)."""
    ref, strand, attr, tail, S, E, xs, xe = _pieces(case, q)
    src = case["source"]
    fixed = len(b"%s\t%s\texon\t\t\t.\t%s\t.\t%s\n" % (ref, src, strand, attr))
    head = len(b"%s\t%s\ttranscript\t%d\t%d\t.\t%s\t.\t%s%s\n" % (ref, src, S, E, strand, attr, tail))
    digits = lambda v: len(v) + int(sum((v >= 10 ** k).sum() for k in range(1, 10)))      # %d of 0 .. 2147483647
    total = head + fixed * len(xs) + digits(xs) + digits(xe)
    if total >= BATCH_BYTES:
        raise Domain("big")
    return total


def block_text(case, q):
    ref, strand, attr, tail, S, E, xs, xe = _pieces(case, q)
    src = case["source"]
    out = [b"%s\t%s\ttranscript\t%d\t%d\t.\t%s\t.\t%s%s\n" % (ref, src, S, E, strand, attr, tail)]
    for s, e in zip(xs.tolist(), xe.tolist()):
        out.append(b"%s\t%s\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (ref, src, s, e, strand, attr))
    text = b"".join(out)
    if len(text) >= BATCH_BYTES:
        raise Domain("big")
    return text


def error(case, sizes_only=False):
    """None, or (smallest bad block, kind)."""
    for q in range(case["m"]):
        try:
            block_bytes(case, q) if sizes_only else block_text(case, q)
        except Domain as d:
            return q, d.kind
    return None


def texts(case):
    """The text of every block."""
    return [block_text(case, q) for q in range(case["m"])]


def text(case):
    return b"".join(texts(case))


def cut(lengths, first, max_blocks, max_bytes):
    """Blocks one batch takes from ``first``: within max_blocks, their summed bytes within max_bytes and below 2^32 - 64; always one."""
    k, total = 0, 0
    while first + k < len(lengths) and k < max_blocks:
        b = int(lengths[first + k])
        if k > 0 and (total + b > max_bytes or total + b >= BATCH_BYTES):
            break
        total += b
        k += 1
    return k
