"""Inputs the bam2sj tests share (CPU: the restatement against hand-worked answers; GPU: the CLI against the restatement)."""
import gzip

import numpy as np

from oracle import filter_oracle as fo

HDR = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:2000000\n@SQ\tSN:chr2\tLN:1500000\n@SQ\tSN:chr3\tLN:900000\n"
NAMES = ["chr1", "chr2", "chr3"]


def sam_line(qname, flag, rname, pos, cigar, aux=()):
    return "\t".join([qname, str(flag), rname, str(pos), "60", cigar, "*", "0", "0", "*", "*"] + list(aux)) + "\n"


# FLAG 3 = paired + proper pair.  POS is 1-based: `end` starts at POS - 1 and every M = X D N adds its length; an N of at least
# -i (3) bases gives don = end + 1, acc = end + length BEFORE end grows.
HAND = [
    # name   flag chrom   pos   cigar                  aux            rows (tid, don, acc, uniq_c, multi_c)
    ("r01", 3, "chr1", 101, "10M3N10M", ["NH:i:1"]),            # end 100 -> 110; 3N = -i: kept           (0, 111, 113, 1, 0)
    ("r02", 3, "chr1", 101, "10M2N10M", ["NH:i:1"]),            # 2N = -i - 1: only grows end             none
    ("r03", 3, "chr1", 201, "5M2D5M100N5M", ["NH:i:1"]),        # 200 + 5 + 2 (D) + 5 = 212               (0, 213, 312, 1, 0)
    ("r04", 3, "chr1", 201, "4=3X6M100N5M", ["NH:i:1"]),        # 200 + 4 (=) + 3 (X) + 6 = 213           (0, 214, 313, 1, 0)
    ("r05", 3, "chr1", 301, "3H5S5M2I1P5M50N5M", ["NH:i:1"]),   # H S I P add nothing: 300 + 5 + 5 = 310  (0, 311, 360, 1, 0)
    ("r06", 3, "chr1", 401, "10M20N10M30N10M", ["NH:i:1"]),     # 410 -> (411, 430); 430 + 10 = 440 -> (441, 470): two rows
    ("r07", 3, "chr1", 501, "40N10M", ["NH:i:1"]),              # N first: end 500                        (0, 501, 540, 1, 0)
    ("r08", 3, "chr1", 601, "10M25N10M", ["NH:i:1"]),           # 610                                     (0, 611, 635, 1, 0) }
    ("r09", 3, "chr1", 601, "10M25N10M", ["NH:i:3"]),           # the same junction, multi-mapped         (0, 611, 635, 0, 1) } -> 1, 1
    ("r10", 3, "chr1", 701, "10M25N10M", []),                   # no NH: multi-mapped, one message        (0, 711, 735, 0, 1)
    ("r11", 3, "chr1", 801, "10M25N10M", ["NH:i:2"]),           #                                         (0, 811, 835, 0, 1)
    ("r12", 3, "chr1", 901, "10M25N10M", ["NH:Z:1"]),           # not an integer type: value 0            (0, 911, 935, 0, 1)
    ("r13", 1, "chr1", 1001, "10M25N10M", ["NH:i:1"]),          # paired, not proper: skipped, -p or not  none
    ("r14", 0, "chr1", 1001, "10M25N10M", []),                  # no FLAG & 2: skipped -- behind the NH test: a second message
    ("r15", 7, "chr1", 1101, "10M25N10M", []),                  # unmapped (FLAG & 4): skipped in front of the NH test, no message
    ("r16", 3, "chr2", 51, "10M1000N10M", ["NH:i:1"]),          # 50 + 10 = 60                            (1, 61, 1060, 1, 0)
    ("r17", 4, "*", 0, "*", []),                                # unmapped, nowhere
]
HAND_TABLE = [
    (0, 111, 113, 1, 0), (0, 213, 312, 1, 0), (0, 214, 313, 1, 0), (0, 311, 360, 1, 0), (0, 411, 430, 1, 0), (0, 441, 470, 1, 0),
    (0, 501, 540, 1, 0), (0, 611, 635, 1, 1), (0, 711, 735, 0, 1), (0, 811, 835, 0, 1), (0, 911, 935, 0, 1), (1, 61, 1060, 1, 0),
]
HAND_NO_NH_MESSAGES = 2


def hand_sam():
    return HDR + "".join(sam_line(*r) for r in HAND)


def no_junction_sam():
    """Mapped, properly paired records without a qualifying N."""
    return HDR + sam_line("a", 3, "chr1", 11, "50M", ["NH:i:1"]) + sam_line("b", 3, "chr1", 21, "20M2N20M", ["NH:i:1"]) + \
        sam_line("c", 3, "chr2", 5, "10M5D10M", ["NH:i:1"])


def sam_to_bam_bytes(sam_text):
    """The SAM text as a BGZF BAM file (the independent encoder of oracle/filter_oracle.py)."""
    header = [l + "\n" for l in sam_text.splitlines() if l.startswith("@")]
    refs = []
    for h in header:
        if h.startswith("@SQ"):
            d = dict(x.split(":", 1) for x in h.rstrip("\n").split("\t")[1:])
            refs.append((d["SN"], int(d["LN"])))
    idx = {n: i for i, (n, _) in enumerate(refs)}
    recs = [fo.Record(l) for l in sam_text.splitlines() if l and not l.startswith("@")]
    return fo.bgzf_blocks(fo.header_bytes(header, refs) + b"".join(fo.encode_record(r, idx) for r in recs))


def write_inputs(tmp, tag, sam_text):
    """(sam, gzip sam, bam) paths of one SAM text."""
    p = [str(tmp / (tag + ext)) for ext in (".sam", ".sam.gz", ".bam")]
    with open(p[0], "w") as fh:
        fh.write(sam_text)
    with gzip.open(p[1], "wt") as fh:
        fh.write(sam_text)
    with open(p[2], "wb") as fh:
        fh.write(sam_to_bam_bytes(sam_text))
    return p


def tids_0_1_0_sam():
    """tids 0, 1, 0: the reference's backward search stops inside the chr2 block (a smaller donor there ends it whatever the tid),
    so its list is not the sorted table."""
    return HDR + \
        sam_line("a", 3, "chr1", 101, "10M50N10M", ["NH:i:1"]) + \
        sam_line("b", 3, "chr2", 1, "10M50N10M", ["NH:i:1"]) + \
        sam_line("c", 3, "chr2", 501, "10M50N10M", ["NH:i:2"]) + \
        sam_line("d", 3, "chr1", 301, "10M50N10M", ["NH:i:1"]) + \
        sam_line("e", 3, "chr1", 101, "10M50N10M", []) + \
        sam_line("f", 3, "chr1", 1, "10M50N10M", ["NH:i:1"])


def synth_records(n, seed, n_chrom=5, span=400000, n_intron=1000):
    """Record columns for the size tests: tids never decrease over `n_chrom` chromosomes, 1-10 CIGAR operations, about a third of the
    records carry one to three N (consecutive introns of `n_intron` fixed ones per chromosome, so about n_chrom * n_intron distinct
    junctions result and every one repeats), 2 % unmapped, 5 % without FLAG & 2, NH absent / 1 / 2..9 (a multi-mapped record
    either way).  Positions are in no order inside a chromosome.  Returns dict(flag, tid, pos, uniq, cig_off, cig)."""
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.integers(0, n_chrom, n)).astype(np.int32)
    sites = np.sort(rng.integers(1000, span, (n_chrom, 2 * n_intron)), axis=1)      # intron j = sites[2j] .. sites[2j + 1]
    flag = np.full(n, 3, np.uint16)
    flag[rng.random(n) < 0.05] = 1
    flag[rng.random(n) < 0.02] |= 4
    uniq = (rng.integers(0, 3, n) == 1).astype(np.uint8)              # absent, 1, 2..9
    pos = np.zeros(n, np.int32)
    cig, off = [], [0]
    spliced = rng.random(n) < 0.34
    for i in range(n):
        ops = []
        if spliced[i]:
            k = int(rng.integers(1, 4))
            j0 = int(rng.integers(0, n_intron - k + 1))
            pts = sites[tid[i], 2 * j0:2 * (j0 + k)]
            pos[i] = max(int(pts[0]) - int(rng.integers(5, 60)), 0)
            end = int(pos[i])
            if rng.random() < 0.3:
                ops.append((int(rng.integers(1, 20)), 4))
            for j in range(k):
                don, acc = int(pts[2 * j]), int(pts[2 * j + 1])
                gap = don - end
                if gap > 6 and j == 0 and rng.random() < 0.3:
                    ops += [(gap // 2, 0), (int(rng.integers(1, 4)), 1), (gap - gap // 2, 0)]
                elif gap > 0:
                    ops.append((gap, 0))
                ops.append((max(acc - don, 1), 3))
                end = max(end, don) + max(acc - don, 1)
            ops.append((int(rng.integers(5, 60)), 0))
        else:
            pos[i] = int(rng.integers(0, span))
            ops.append((int(rng.integers(20, 150)), 0))
            if rng.random() < 0.2:
                ops += [(int(rng.integers(1, 3)), 2), (int(rng.integers(5, 50)), 0)]
            if rng.random() < 0.1:
                ops += [(2, 3), (int(rng.integers(5, 50)), 0)]        # an N below -i
        cig += [(l << 4) | op for l, op in ops]
        off.append(len(cig))
    return dict(flag=flag, tid=tid, pos=pos, uniq=uniq, cig_off=np.asarray(off, np.int64), cig=np.asarray(cig, np.uint32))


def subset(rec, idx):
    """The records `idx` (ascending) of synth_records()'s columns."""
    idx = np.asarray(idx)
    lens = np.diff(rec["cig_off"])[idx]
    cig = np.concatenate([rec["cig"][rec["cig_off"][i]:rec["cig_off"][i + 1]] for i in idx]) if len(idx) else np.zeros(0, np.uint32)
    return dict(flag=rec["flag"][idx], tid=rec["tid"][idx], pos=rec["pos"][idx], uniq=rec["uniq"][idx],
                cig_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), cig=cig)


def records_sam(rec, nh_seed=0):
    """The columns of synth_records() as SAM text (NH: absent or 2..9 for a multi-mapped record)."""
    rng = np.random.default_rng(nh_seed)
    out = [HDR.replace("@SQ\tSN:chr3\tLN:900000\n", "@SQ\tSN:chr3\tLN:900000\n@SQ\tSN:chr4\tLN:900000\n@SQ\tSN:chr5\tLN:900000\n")]
    ops = "MIDNSHP=XB"
    for i in range(len(rec["flag"])):
        c = rec["cig"][rec["cig_off"][i]:rec["cig_off"][i + 1]]
        cigar = "".join("%d%s" % (w >> 4, ops[w & 15]) for w in c)
        aux = ["NH:i:1"] if rec["uniq"][i] else ([] if rng.random() < 0.5 else ["NH:i:%d" % int(rng.integers(2, 10))])
        out.append(sam_line("q%d" % i, int(rec["flag"][i]), "chr%d" % (rec["tid"][i] + 1), int(rec["pos"][i]) + 1, cigar, aux))
    return "".join(out)


def heavy_digit_rows(n, seed):
    """(five row columns, key bytes that differ) for the radix passes: about 80 % of the n shuffled rows share the lowest byte of acc and
    the lowest byte of tid -- in those two passes one digit value holds far more than 256 rows of every tile, so a row's rank crosses
    waves and rounds -- and differ in the bytes above and in don; the other rows are spread over every byte in use; a tenth of the keys
    comes twice.  A pass runs per key byte (tid, don, acc: twelve) that is not one value in every row."""
    rng = np.random.default_rng(seed)
    heavy = rng.random(n) < 0.8
    acc = np.where(heavy, 0x2a | (rng.integers(0, 4096, n) << 8), rng.integers(0, 1 << 20, n)).astype(np.int32)
    don = rng.integers(1, 60000, n).astype(np.int32)
    tid = np.where(heavy, 7 | (rng.integers(0, 3, n) << 8), rng.integers(0, 700, n)).astype(np.int32)
    for c in (tid, don, acc):
        c[n - n // 10:] = c[:n // 10]                                      # one key in ten comes twice, a tile or more apart
    rows = [tid, don, acc, rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32)]
    differ = sum(len(np.unique((c.astype(np.int64) >> (8 * b)) & 0xff)) > 1 for c in (tid, don, acc) for b in range(4))
    return rows, int(differ)
