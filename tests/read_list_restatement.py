"""The read lists of `update-gtf -a / -k / -v / -u` restated in Python from the rule in include/lr2rmats_hip.h: which blocks a list holds
(the classes, the pieces of a split candidate), the text of a block, its domain error, and the batch cut.  It shares no code with the
engine's host routine (lr2rmats_amd/csrc/l2r_readlistplan.hip.h); tests/test_read_lists_cpu.py and tests/test_gpu_read_lists.py compare
both routes with it.

A case is a dict: ``refs`` (reference names by tid), ``src``, ``tid``, ``names`` (bytes: NUL-terminated strings), ``qname``, ``tid_name``
(byte offsets, or None), ``anno``, ``tx_gid``, ``tx_gname`` (the annotation's gene tables), the arrays of a download (``ex_off``, ``xs``,
``xe``, ``f``, ``info``, ``ref_tx``), and the scalars ``has_sj`` and ``split``."""

ALL, KNOWN, NOVEL, UNRECOG = 0, 1, 2, 3
LISTS = (ALL, KNOWN, NOVEL, UNRECOG)
I_KNOWN, I_KNOWN_SITE, I_FULL, I_REV, I_SJ_PASS = 0x01, 0x02, 0x04, 0x08, 0x40
F_NOVEL_JUNC, F_UNREL_JUNC = 0x08, 0x10
NAME_MAX = 254
PIECE_NAME_MAX = 100
BATCH_BYTES = (1 << 32) - 64

KINDS = ("tid", "noexon", "ref", "name_id", "name_long", "name_nul", "piece_name", "neg", "big")
KIND_CODE = {k: i + 1 for i, k in enumerate(KINDS)}                                         # RL_E_* of l2r_readlistplan.hip.h
KIND_TEXT = {"tid": "a reference outside the table", "noexon": "a read with no exon", "ref": "an annotation transcript at or beyond n_tx",
             "name_id": "a name id at or beyond its table", "name_long": "a name of 255 or more bytes", "name_nul": "a name without a NUL inside the table",
             "piece_name": "a piece name of 100 or more bytes", "neg": "a negative exon coordinate", "big": "its text reaches 2^32 - 64 bytes"}


class DomainError(Exception):
    def __init__(self, kind):
        Exception.__init__(self, kind)
        self.kind = kind


def pack_table(strings):
    """(table, offsets): the strings NUL-terminated one behind the other."""
    off, at = [], 0
    for s in strings:
        off.append(at)
        at += len(s) + 1
    return b"".join(bytes(s) + b"\0" for s in strings), off


def pieces(flags):
    """The (first, last) exon ranges of the pieces of a read with these exon flags, in ascending order."""
    n, out = len(flags), []
    first, novel, known = 0, False, False
    for j in range(n):
        end = j == n - 1
        if not end:
            if flags[j] & F_NOVEL_JUNC:
                novel = True
            else:
                known = True
        if end or flags[j] & F_UNREL_JUNC:
            if novel and known and j - first >= 1:
                out.append((first, j))
            first, novel, known = j + 1, False, False
    return out


def select(case, lst):
    """The blocks of list ``lst`` in read order: (read, first exon, exon count, piece or -1)."""
    out = []
    for i, info in enumerate(int(v) for v in case["info"]):
        n = info >> 8
        whole = (i, 0, n, -1)
        if lst == ALL:
            out.append(whole)
            continue
        if not info & I_FULL:
            continue
        if info & I_KNOWN:
            cls = KNOWN
        elif info & I_KNOWN_SITE:
            cls = NOVEL
        else:
            cls = UNRECOG
        if cls != lst:
            continue
        if cls != NOVEL or not case["has_sj"] or info & I_SJ_PASS:
            out.append(whole)
        elif case["split"]:
            off = int(case["ex_off"][i])
            for k, (a, b) in enumerate(pieces([int(v) for v in case["f"][off:off + n]])):
                out.append((i, a, b - a + 1, k))
    return out


def _name(table, at):
    """The string at byte ``at`` of a table, with the id / 255-byte / NUL tests in that order."""
    if at >= len(table):
        raise DomainError("name_id")
    end = table.find(b"\0", at, at + NAME_MAX + 1)
    if end < 0:
        raise DomainError("name_long" if len(table) - at >= NAME_MAX + 1 else "name_nul")
    return table[at:end]


def block_text(case, block):
    """The text of one block; DomainError with the first kind that applies."""
    i, first, count, piece = block
    refs, src = case["refs"], bytes(case.get("src", b"lr2rmats"))
    tid = int(case["tid"][i])
    if not 0 <= tid < len(refs):
        raise DomainError("tid")
    if count < 1:
        raise DomainError("noexon")
    ref = int(case["ref_tx"][i])
    if ref >= len(case["tx_gid"]):
        raise DomainError("ref")
    info = int(case["info"][i])
    rev = bool(info & I_REV)
    tid_name = case["qname"] if case.get("tid_name") is None else case["tid_name"]
    g = b"NA" if ref < 0 else _name(case["anno"], int(case["tx_gid"][ref]))
    t = _name(case["names"], int(tid_name[i]))
    G = b"NA" if ref < 0 else _name(case["anno"], int(case["tx_gname"][ref]))
    T = _name(case["names"], int(case["qname"][i]))
    if piece >= 0:
        t, T = t + b".split.%d" % piece, T + b".split.%d" % piece
        if len(t) >= PIECE_NAME_MAX or len(T) >= PIECE_NAME_MAX:
            raise DomainError("piece_name")
    off = int(case["ex_off"][i]) + first
    xs, xe = [int(v) for v in case["xs"][off:off + count]], [int(v) for v in case["xe"][off:off + count]]
    if min(xs) < 0 or min(xe) < 0:
        raise DomainError("neg")
    attr = b" ".join(b'%s "%s";' % (key, s) for key, s in ((b"gene_id", g), (b"transcript_id", t), (b"gene_name", G), (b"transcript_name", T)) if s)
    strand = b"-" if rev else b"+"
    if piece < 0:
        head = b"%s\t%s\ttranscript\t%d\t%d\t.\t%s\t.\t%s transcript_cov \"1\";\n" % (refs[tid], src, xs[0], xe[-1], strand, attr)
        order = range(count - 1, -1, -1) if rev else range(count)
    else:                                                   # Q2: the transcript line of a piece stands on reference 0, 0 .. 0, `+`; its exons ascend
        head = b"%s\t%s\ttranscript\t0\t0\t.\t+\t.\t%s transcript_cov \"1\";\n" % (refs[0], src, attr)
        order = range(count)
    out = head + b"".join(b"%s\t%s\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (refs[tid], src, xs[j], xe[j], strand, attr) for j in order)
    if len(out) >= BATCH_BYTES:
        raise DomainError("big")
    return out


def texts(case, lst):
    return [block_text(case, b) for b in select(case, lst)]


def text(case, lst):
    return b"".join(texts(case, lst))


def error(case, lst):
    """(block, kind) of the smallest block of the list with a domain error, or None."""
    for q, b in enumerate(select(case, lst)):
        try:
            block_text(case, b)
        except DomainError as e:
            return q, e.kind
    return None


def cut(lens, first, max_blocks, max_bytes):
    """How many blocks from ``first`` one batch takes: within max_blocks, the summed bytes within max_bytes and below 2^32 - 64; always one."""
    k, total = 0, 0
    while first + k < len(lens) and k < max_blocks:
        b = lens[first + k]
        if k > 0 and (total + b > max_bytes or total + b >= BATCH_BYTES):
            break
        total += b
        k += 1
    return k
