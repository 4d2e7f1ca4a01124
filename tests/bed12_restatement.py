"""The rule of `bam2bed` (include/lr2rmats_hip.h, l2r_bed_lines) in plain Python: a loop and %d.  It shares no code with the product; the
tests take their expected bytes from here.

A record is (flag, tid, pos, mapq, name, cigar) with name a byte string and cigar a list of (length, op) -- op an index into "MIDNSHP=X".
"""
OPS = "MIDNSHP=X"
POS_MAX = 2147483647


class BedDomainError(Exception):
    def __init__(self, record, kind):
        Exception.__init__(self, "record %d: %s" % (record, kind))
        self.record, self.kind = record, kind


def blocks(cigar):
    """(sizes, starts, span) of a CIGAR."""
    cur, length, sizes, starts = 0, 0, [], [0]
    for n, op in cigar:
        if op > 8:
            raise ValueError("op")
        c = OPS[op]
        if c in "M=XD":
            cur += n
            length += n
        elif c == "N":
            sizes.append(length)
            cur += n
            starts.append(cur)
            length = 0
    sizes.append(length)
    return sizes, starts, cur


def line(record, ref_names, color=b"255,0,0", index=0):
    """The line of one record (b"" for an unmapped one)."""
    flag, tid, pos, mapq, name, cigar = record
    if flag & 4:
        return b""
    if tid < 0 or tid >= len(ref_names):
        raise BedDomainError(index, "tid")
    if pos < 0:
        raise BedDomainError(index, "pos")
    try:
        sizes, starts, span = blocks(cigar)
    except ValueError:
        raise BedDomainError(index, "op")
    if pos + span > POS_MAX:
        raise BedDomainError(index, "end")
    suffix = b"/1" if flag & 0x40 else b"/2" if flag & 0x80 else b""
    cols = [ref_names[tid], b"%d" % pos, b"%d" % (pos + span), name + suffix, b"%d" % mapq, b"-" if flag & 16 else b"+", b"%d" % pos,
            b"%d" % (pos + span), color, b"%d" % len(sizes), b",".join(b"%d" % v for v in sizes), b",".join(b"%d" % v for v in starts)]
    return b"\t".join(cols) + b"\n"


def text(records, ref_names, color=b"255,0,0"):
    """The text of the records; a domain error names the smallest bad record."""
    return b"".join(line(r, ref_names, color, i) for i, r in enumerate(records))


KIND_TEXT = {"tid": "with reference", "pos": "at position", "op": "operation code above 8", "end": "is beyond 2147483647"}


def parse_cigar(s):
    """"5S10M" -> [(5, 4), (10, 0)]; "*" -> []."""
    out, n = [], 0
    if s == "*":
        return out
    for ch in s:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append((n, OPS.index(ch)))
            n = 0
    return out


def read_sam(path):
    """(ref_names, records) of a SAM file with @SQ lines: the columns the rule reads."""
    refs, recs = [], []
    with open(path, "rb") as fh:
        for ln in fh.read().split(b"\n"):
            if not ln:
                continue
            if ln.startswith(b"@"):
                if ln.startswith(b"@SQ"):
                    refs.append([f[3:] for f in ln.split(b"\t") if f.startswith(b"SN:")][0])
                continue
            f = ln.split(b"\t")
            tid = -1 if f[2] == b"*" else refs.index(f[2])
            recs.append((int(f[1]), tid, int(f[3]) - 1, int(f[4]), f[0], parse_cigar(f[5].decode())))
    return refs, recs


def columns(records):
    """The records as the columns of Engine.bed_lines: flag, tid, pos, mapq, (cig_off, cig), names."""
    import numpy as np
    flag = np.array([r[0] for r in records], np.uint16)
    tid = np.array([r[1] for r in records], np.int32)
    pos = np.array([r[2] for r in records], np.int32)
    mapq = np.array([r[3] for r in records], np.uint8)
    cig_off = np.zeros(len(records) + 1, np.int64)
    if records:
        cig_off[1:] = np.cumsum([len(r[5]) for r in records])
    cig = np.array([(n << 4) | op for r in records for n, op in r[5]], np.uint32)
    return flag, tid, pos, mapq, (cig_off, cig), [r[4] for r in records]
