"""The GTF order of include/lr2rmats_hip.h (l2r_gtf_order, `sort-gtf`), restated in plain Python from a dict and a ``sorted``, and the
text generators the CPU and GPU tests share.

Lines end at b"\\n", a last line without one counts, line numbers start at 1.  Fields are runs of bytes other than space and tab.  A line
is kept iff byte 0 is not "#" and field three contains "transcript" or equals "exon"; it is a transcript line iff field three equals
"transcript".  A transcript line sets the key (rank of field one, field four, field five); every kept line carries the key of the last
transcript line at or before it, (0, 0, 0) before the first; kept lines are ordered by (key, line number) and written as their first
nine tab-separated columns."""
import re

TABLE = {b"chr%d" % k: k for k in range(1, 23)}
TABLE.update({b"chrX": 23, b"chrY": 24, b"chrM": 25})
DIGITS = re.compile(rb"[0-9]+\Z")


class GtfDomainError(Exception):
    def __init__(self, line, kind):
        Exception.__init__(self, "line %d: %s" % (line, kind))
        self.line, self.kind = line, kind                 # kind: "NUL", "fields", "start", "end"


def split_lines(text: bytes):
    """[(start, length)] of every line."""
    out, p = [], 0
    while p < len(text):
        q = text.find(b"\n", p)
        q = len(text) if q < 0 else q
        out.append((p, q - p))
        p = q + 1
    return out


def fields(line: bytes):
    return [f for f in re.split(rb"[ \t]+", line) if f]


def gtf_order(text: bytes, _keys=False):
    """(rows, stats): rows = [(start, length, line number)] in the order; stats = the words of l2r_gtf_stats that do not depend on the
    route.  Raises GtfDomainError for the smallest bad line."""
    rank, beyond, names = dict(TABLE), 0, set()
    key, rows, keys = (0, 0, 0), [], []
    n_tx = heads = 0
    prev_name = None
    lines = split_lines(text)
    for no, (p, n) in enumerate(lines, 1):
        line = text[p:p + n]
        if b"\0" in line:
            raise GtfDomainError(no, "NUL")
        f = fields(line)
        if line[:1] == b"#" or len(f) < 3 or not (b"transcript" in f[2] or f[2] == b"exon"):
            continue
        if f[2] == b"transcript":
            if len(f) < 5:
                raise GtfDomainError(no, "fields")
            for k, kind in ((3, "start"), (4, "end")):
                if not DIGITS.match(f[k]) or int(f[k]) > 4294967295:
                    raise GtfDomainError(no, kind)
            if f[0] not in rank:
                beyond += 1
                rank[f[0]] = 25 + beyond
            names.add(f[0])
            heads += n_tx == 0 or f[0] != prev_name
            prev_name = f[0]
            n_tx += 1
            key = (rank[f[0]], int(f[3]), int(f[4]))
        rows.append((p, n, no))
        keys.append(key)
    order = sorted(range(len(rows)), key=lambda i: (keys[i], rows[i][2]))
    stats = {"bytes": len(text), "lines": len(lines), "rows": len(rows), "transcripts": n_tx, "heads": heads, "names_beyond_table": beyond,
             "identity": int(order == list(range(len(rows)))), "names": len(names)}
    return [rows[i] + ((keys[i],) if _keys else ()) for i in order], stats


def first_descent(text: bytes):
    """The line number of the first kept line whose key is below its predecessor's (in line order), None where there is none."""
    rows, _ = gtf_order(text, _keys=True)
    rows.sort(key=lambda r: r[2])
    for a, b in zip(rows, rows[1:]):
        if b[3] < a[3]:
            return b[2]
    return None


def write_rows(text: bytes, rows) -> bytes:
    out = []
    for p, n, _ in rows:
        cols = text[p:p + n].split(b"\t")[:9]
        out.append(b"\t".join(cols + [b""] * (9 - len(cols))) + b"\n")
    return b"".join(out)


def sort_gtf(text: bytes) -> bytes:
    return write_rows(text, gtf_order(text)[0])


# ------------------------------------------------------------------------------------------------ generators

ATTR = b'gene_id "G%d"; transcript_id "T%d";'


def tx_line(chrom, s, e, k=0, feature=b"transcript", sep=b"\t"):
    return sep.join([chrom, b"src", feature, b"%d" % s, b"%d" % e, b".", b"+", b".", ATTR % (k, k)])


def transcript_block(rng, chrom, k, max_exons=4, lo=1, hi=200000):
    """One transcript line and 0..max_exons exon lines behind it."""
    s = int(rng.integers(lo, hi))
    e = s + int(rng.integers(0, 5000))
    out = [tx_line(chrom, s, e, k)]
    for _ in range(int(rng.integers(0, max_exons + 1))):
        a = int(rng.integers(s, e + 1))
        out.append(tx_line(chrom, a, int(rng.integers(a, e + 1)), k, b"exon"))
    return out


def blocks_with_rows(rng, n_rows, chroms=(b"chr1", b"chr2", b"chrX", b"scaffold_9", b"chr10", b"KI270728.1")):
    """Transcript blocks with exactly n_rows kept lines in all, whole transcripts shuffled."""
    blocks, left, k = [], n_rows, 0
    while left > 0:
        b = transcript_block(rng, chroms[int(rng.integers(0, len(chroms)))], k)[:left]
        blocks.append(b)
        left -= len(b)
        k += 1
    rng.shuffle(blocks)
    return blocks


def text_of(blocks, final_newline=True) -> bytes:
    lines = [ln for b in blocks for ln in b]
    t = b"\n".join(lines)
    return t + b"\n" if lines and final_newline else t


NOISE = [b"", b"#comment line", b" #x\ty\ttranscript\t5\t9", b"chr1\tsrc\tgene\t1\t9\t.\t+\t.\tg", b"chr1\tsrc\tCDS\t1\t9\t.\t+\t0\tg",
         b"chr2\tsrc\texons\t1\t9", b"chr2\tsrc\tprimary_transcript\tx\ty\t.\t+\t.\tid 5", b"chr3 src exon -5 1e3", b"  \t chrM\t\tsrc  transcript \t 0007\t4294967295\t.\t+\t.\ta\tb\tc\td",
         b"one", b"one two", b"chrQ\tsrc\ttranscripts\tjunk\tjunk", b"chrQ\tsrc\tTranscript\t1\t2", b"scaf src transcript 12 34", b"chr5\tsrc\texon\t12.5\t\t.\t+"]


def random_text(rng, n_lines=30) -> bytes:
    """A small text inside the domain: transcript blocks on a few names, noise lines of every kind between them, sometimes no final newline."""
    names = [b"chr1", b"chr10", b"chr1_random", b"chr", b"chrX", b"chrM", b"u2", b"u1", b"c" * 40]
    lines = []
    k = 0
    while len(lines) < n_lines:
        r = int(rng.integers(0, 10))
        if r < 5:
            lines += transcript_block(rng, names[int(rng.integers(0, len(names)))], k, hi=int(rng.choice([50, 100000])))
            k += 1
        else:
            lines.append(NOISE[int(rng.integers(0, len(NOISE)))])
    t = b"\n".join(lines)
    return t + (b"\n" if rng.integers(0, 4) else b"")
