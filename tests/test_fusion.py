"""`lr2rmats fusion` (reference src/bam_fusion.c, bam2seg of src/parse_bam.c:543-595): a hand-worked table for the literal
restatement (tests/fusion_restatement.py), the host's grouping against it (CPU), and the HIP path through the CLI and the C-ABI
against the restatement (GPU)."""
import gzip
import os

import numpy as np
import pytest

from lr2rmats_amd import hostlib
from oracle import filter_oracle as fo

from tests import fusion_restatement as fr

HDR = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:2000000\n@SQ\tSN:chr2\tLN:1500000\n@SQ\tSN:chr3\tLN:900000\n@PG\tID:aligner\tPN:x\n"
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _line(qname, flag, rname, pos, cigar, seq, aux=(), mapq=60):
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, "*", "0", "0", seq, "*"] + list(aux)) + "\n"


def _seq_len(cigar):
    return sum(l for (l, op) in fo.parse_cigar(cigar) if op in (0, 1, 4, 7, 8))


def _aux(score, nm=None):
    return (["AS:i:%d" % score] if score is not None else []) + (["NM:i:%d" % nm] if nm is not None else [])


# ---------------------------------------------------------------------------------------------------- hand-worked table
# Every read has 100 query bases.  (name, [(flag, chrom, pos, cigar, AS, NM)...], written pair as indices into the read's records
# -- seg[0] first -- or None, site line or None).  Worked from src/bam_fusion.c:61-142 and src/parse_bam.c:543-595.
A = (0, "chr1", 1000, "60M40S", 60, None)             # read 1..60, chr1 1000..1059
HAND = [
    # s1 read 61..100 on chr2: no overlap, another chromosome, cover 100/100
    ("fus", [A, (2048, "chr2", 5000, "60S40M", 40, None)], (0, 1), "fus\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5039\n"),
    # reverse strand: 40M60S is read 1..40 in front of the swap, 101 - 40 = 61 .. 101 - 1 = 100 behind it
    ("rev", [A, (2064, "chr2", 5000, "40M60S", 40, None)], (0, 1), "rev\tchr1\t+\t1000\t1059\tchr2\t-\t5000\t5039\n"),
    # same chromosome: 50000 - 1059 = 48941, 0 < 48941 < 100000
    ("near", [A, (2048, "chr1", 50000, "60S40M", 40, None)], None, None),
    # 200000 - 1059 = 198941 >= 100000
    ("far", [A, (2048, "chr1", 200000, "60S40M", 40, None)], (0, 1), "far\tchr1\t+\t1000\t1059\tchr1\t+\t200000\t200039\n"),
    # read 71..100: cover 90/100 = 0.90 < 0.99 and no further segment: -1
    ("gap", [A, (2048, "chr2", 5000, "70S30M", 40, None)], None, None),
    # read 62..100: cover 99/100, (float)0.99 >= 0.99f
    ("cov99", [A, (2048, "chr2", 5000, "61S39M", 40, None)], (0, 1), "cov99\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5038\n"),
    # 10/100 = 0.1 < (double)0.1f = 0.10000000149...: the segment is skipped
    ("tenth", [(0, "chr1", 1000, "90M10S", 60, None), (2048, "chr2", 5000, "90S10M", 40, None)], None, None),
    ("eleven", [(0, "chr1", 1000, "89M11S", 60, None), (2048, "chr2", 5000, "89S11M", 40, None)], (0, 1),
     "eleven\tchr1\t+\t1000\t1088\tchr2\t+\t5000\t5010\n"),
    # read 1..60 and 51..100: (60 - 51 + 1) / min(60, 50) = 0.2 > 0.1
    ("ovl", [A, (2048, "chr2", 5000, "50S50M", 40, None)], None, None),
    # 1..40, then 41..70 (cover 0.70), then 71..100 (cover 1.00): the loop returns 3, nothing is written
    ("three", [(0, "chr1", 1000, "40M60S", 40, None), (2048, "chr2", 5000, "40S30M30S", 30, 0), (2048, "chr3", 7000, "70S30M", 30, 2)], None, None),
    # the better score is the second record of the file: it is seg[0] and written first; the site line starts with the smaller read_start
    ("order", [(0, "chr1", 1000, "60M40S", 40, None), (2048, "chr2", 5000, "60S40M", 60, None)], (1, 0),
     "order\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5039\n"),
    # equal AS: NM 1 sorts in front of NM 5.  seg[0] = record 1 (read 1..50); record 0 (1..60) overlaps it 50/50; record 2 (51..100) fits.
    # (with record 0 as seg[0]: record 1 overlaps 60/50, record 2 overlaps 10/50 = 0.2 -- no candidate)
    ("tie", [(0, "chr1", 1000, "60M40S", 50, 5), (2048, "chr2", 5000, "50M50S", 50, 1), (2048, "chr3", 7000, "50S50M", 30, None)], (1, 2),
     "tie\tchr2\t+\t5000\t5049\tchr3\t+\t7000\t7049\n"),
    # the middle record is read 56..60: 5/100 < 0.1, skipped; 1..55 + 56..100
    ("small", [(0, "chr1", 1000, "55M45S", 55, None), (2048, "chr2", 5000, "55S5M40S", 50, None), (2048, "chr3", 7000, "55S45M", 45, None)], (0, 2),
     "small\tchr1\t+\t1000\t1054\tchr3\t+\t7000\t7044\n"),
    # an unmapped record of another name between the two: skipped in front of the name comparison -- one group of two
    ("unm", [A, ("y", 4), (2048, "chr2", 5000, "60S40M", 40, None)], (0, 2), "unm\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5039\n"),
    # OUR rule, not a pin of the reference (which writes outside its bitmap here): rlen = 60 (H is not counted), the second record
    # is read 61..100, outside [1, 60]; clipped cover 60/60
    ("hard", [(0, "chr1", 1000, "60M40H", 60, None), (2048, "chr2", 5000, "60H40M", 40, None)], (0, 1), "hard\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5039\n"),
    # the final group of the file: in the BAM and in the count, never in the site file
    ("last", [A, (2048, "chr2", 5000, "60S40M", 40, None)], (0, 1), None),
]
HAND_WITH_O_025 = {"ovl": (0, 1)}       # -o 0.25: 0.2 > 0.25 is false


def _hand_sam(path):
    """Writes the table; returns {name: index of the read's first record}."""
    rng = np.random.default_rng(1)
    first, n = {}, 0
    with open(path, "w") as fh:
        fh.write(HDR)
        for (name, recs, _, _) in HAND:
            first[name] = n
            for rec in recs:
                if len(rec) == 2:
                    fh.write("\t".join([rec[0], "4", "*", "0", "0", "*", "*", "0", "0", _seq(rng, 100), "*"]) + "\n")
                else:
                    flag, chrom, pos, cigar, score, nm = rec
                    fh.write(_line(name, flag, chrom, pos, cigar, _seq(rng, _seq_len(cigar)), _aux(score, nm)))
                n += 1
    return first


def _hand_expect(first, extra=None):
    pairs, site = [], [fr.SITE_HEADER]
    for (name, _, pair, line) in HAND:
        pair = (extra or {}).get(name, pair)
        if pair is not None:
            pairs.append((first[name] + pair[0], first[name] + pair[1]))
        if line is not None:
            site.append(line)
    return pairs, "".join(site)


def test_restatement_hand_worked_table(tmp_path):
    sam = str(tmp_path / "hand.sam")
    first = _hand_sam(sam)
    stream, pairs, site, count = fr.expected(sam)
    want_pairs, want_site = _hand_expect(first)
    assert pairs == want_pairs and count == len(want_pairs) == 11
    assert site == want_site
    # the stream: header, then seg[0] and seg[1] of every candidate
    header, refs, recs = fo.parse_sam(sam)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    assert stream == fo.header_bytes(header, refs) + b"".join(fo.encode_record(recs[i], idx) for p in want_pairs for i in p)
    # every option moves exactly one read of the table:
    #   -o 0.25   `ovl`: 0.2 > 0.25 is false (`tie`: record 0 still overlaps seg[0] 50/50)
    #   -v 0.05   `tenth`: 0.1 < 0.05... is false (`small`: 5/100 = 0.05 < (double)0.05f = 0.05000000074..., still skipped)
    #   -V 0.9    `gap`: (float)0.90 >= 0.9f (`three`: 1..40 + 41..70 cover 0.70, it still ends at three segments)
    for kw, extra in ((dict(ovlp_frac=0.25), HAND_WITH_O_025), (dict(each_cov=0.05), {"tenth": (0, 1)}), (dict(all_cov=0.9), {"gap": (0, 1)})):
        _, pairs, site, count = fr.expected(sam, **kw)
        assert pairs == _hand_expect(first, extra)[0] and count == 12 and site.count("\n") == 12, kw
    assert "ovl\tchr1\t+\t1000\t1059\tchr2\t+\t5000\t5049\n" in fr.expected(sam, ovlp_frac=0.25)[2]


# ---------------------------------------------------------------------------------------------------- synthetic input

def _part_cigar(rng, L, s, e, clip):
    """One alignment of query positions [s, e] (1-based, forward orientation of the CIGAR) of a read of L bases; insertions,
    deletions and introns inside; clip 'S' or 'H'."""
    body, ops = e - s + 1, []
    left = body
    while left > 0:
        m = left if rng.random() < 0.5 or left < 8 else int(rng.integers(1, left))
        ops.append("%d%s" % (m, "M=X"[int(rng.choice([0, 0, 0, 1, 2]))]))
        left -= m
        if left > 2 and rng.random() < 0.5:
            i = int(rng.integers(1, min(left, 4)))
            ops.append("%dI" % i); left -= i
        if left > 0:
            ops.append("%d%s" % (int(rng.integers(1, 3000)), "DN"[int(rng.integers(0, 2))]))
    return ("%d%s" % (s - 1, clip) if s > 1 else "") + "".join(ops) + ("%d%s" % (L - e, clip) if e < L else "")


def make_sam(path, n_reads, seed):
    """Reads of 1..5 alignments: two parts that split the read at a point, with an overlap / a gap / a part length / a distance at the
    option boundaries +- 1, plus further parts; soft and hard clips, both strands, three chromosomes, AS ties, missing AS / NM,
    unmapped records, names that come back."""
    rng = np.random.default_rng(seed)
    chroms = ["chr1", "chr2", "chr3"]
    lines = []
    for r in range(n_reads):
        name = "read%05d" % r
        L = 100 * int(rng.integers(1, 4))                    # 100, 200, 300: 0.1 L and 0.99 L are whole numbers
        k = int(rng.choice([1, 2, 2, 2, 3, 3, 4, 5]))
        kind = int(rng.integers(0, 6))
        cut = int(rng.integers(L // 5, 4 * L // 5))
        parts = [(1, cut), (cut + 1, L)]
        if kind == 1:                                        # second part exactly 0.1 L - 1, 0.1 L, 0.1 L + 1 long
            n2 = L // 10 + int(rng.integers(-1, 2)); parts = [(1, L - n2), (L - n2 + 1, L)]
        elif kind == 2:                                      # cover 0.99 L - 1, 0.99 L, 0.99 L + 1
            miss = L // 100 + int(rng.integers(-1, 2)); parts = [(1, cut), (cut + 1 + miss, L)]
        elif kind == 3:                                      # read overlap around 0.1 of the shorter part
            n2 = L - cut; ov = max(0, n2 // 10 + int(rng.integers(-1, 2))); parts = [(1, cut + ov), (cut + 1, L)] if cut + ov < L else parts
        for extra in range(k - 2):
            a = int(rng.integers(1, L)); b = min(L, a + int(rng.integers(1, L // 2)))
            parts.append((a, b))
        parts = parts[:k]
        c0 = int(rng.integers(0, 3)); p0 = int(rng.integers(1000, 500000))
        tie = rng.random() < 0.15
        for a, (s, e) in enumerate(parts):
            if rng.random() < 0.03:
                lines.append("\t".join(["other%d" % r if rng.random() < 0.5 else name, "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]) + "\n")
            clip = "H" if rng.random() < 0.15 else "S"
            rev = rng.random() < 0.4
            cig = _part_cigar(rng, L, L + 1 - e, L + 1 - s, clip) if rev else _part_cigar(rng, L, s, e, clip)
            chrom = chroms[c0] if (a == 0 or rng.random() < 0.5) else chroms[int(rng.integers(0, 3))]
            pos = p0
            if a and chrom == chroms[c0]:
                # behind the first part by 100000 - 1, 100000, 100000 + 1 (measured from its end), or overlapping, or far
                ref0 = sum(l for (l, op) in fo.parse_cigar(first_cig) if op in (0, 2, 3, 7, 8))
                pos = p0 + ref0 - 1 + int(rng.choice([99999, 100000, 100001, 5, 300000, -50]))
            if a == 0:
                first_cig = cig
            score = 50 if tie else int((e - s + 1) * rng.uniform(0.6, 1.0)) - a
            aux = _aux(None if rng.random() < 0.05 else score, None if rng.random() < 0.2 else int(rng.integers(0, 9)))
            seq = _seq(rng, _seq_len(cig)) if r % 4 == 0 else "*"
            lines.append(_line(name, (16 if rev else 0) | (2048 if a else 0), chrom, max(1, pos), cig, seq, aux))
        if r % 19 == 0 and r:                                 # an earlier name again: a group of its own
            lines.append(_line("read%05d" % (r - 1), 0, "chr1", 5, "50M50S", "*", _aux(50, 1)))
            lines.append(_line("read%05d" % (r - 1), 2048, "chr3", 5, "50S50M", "*", _aux(45, 0)))
    with open(path, "w") as fh:
        fh.write(HDR)
        fh.writelines(lines)
    return len(lines)


SYNTH_OPTS = [([], {}), (["-o", "0.02", "-v", "0.2", "-V", "0.95"], dict(ovlp_frac=0.02, each_cov=0.2, all_cov=0.95)),
              (["--ovlp-frac", "0.3", "--each-cov", "0.05", "--all-cov", "1.0"], dict(ovlp_frac=0.3, each_cov=0.05, all_cov=1.0))]
_synth = {}


def _synth_case(tmp_path_factory):
    """The synthetic file and the restatement's answers for the three option sets, made once."""
    if not _synth:
        sam = str(tmp_path_factory.mktemp("fusion_synth") / "in.sam")
        make_sam(sam, 4000, 11)
        _synth["sam"] = sam
        _synth["want"] = [fr.expected(sam, **kw) for (_, kw) in SYNTH_OPTS]
    return _synth


def _groups_of_file(sam):
    header, refs, recs = fo.parse_sam(sam)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    return fr.groups_of(recs, [-1 if r.rname == "*" else idx[r.rname] for r in recs]), recs


def _check_host_groups(sam):
    groups, recs = _groups_of_file(sam)
    got = hostlib.fusion_groups(sam)
    assert got["rows"].tolist() == [s.row for (_, _, segs) in groups for s in segs]
    assert got["group_off"].tolist() == np.concatenate([[0], np.cumsum([len(segs) for (_, _, segs) in groups])]).tolist()
    assert got["rlen"].tolist() == [rlen for (_, rlen, _) in groups]
    # the two tags of every record as the reader leaves them (bam_aux2i, 0 without the tag)
    assert got["as_score"].tolist() == [fr.aux_int(r, "AS") for r in recs]
    assert got["nm"].tolist() == [fr.aux_int(r, "NM") for r in recs]
    return groups


def test_host_groups_equal_the_restatement(tmp_path, tmp_path_factory):
    """h_fusion_groups (no GPU): the rows, the groups and their rlen of the hand file and of the synthetic file; the share of
    candidates the restatement finds in the synthetic file is what the GPU tests rely on."""
    sam = str(tmp_path / "hand.sam")
    _hand_sam(sam)
    groups = _check_host_groups(sam)
    assert [(name, len(segs)) for (name, _, segs) in groups][13] == ("unm", 2) and dict((g[0], g[1]) for g in groups)["hard"] == 60
    case = _synth_case(tmp_path_factory)
    groups = _check_host_groups(case["sam"])
    for (_, _, _, count) in case["want"]:
        assert 0.05 * len(groups) <= count <= 0.80 * len(groups), (count, len(groups))


# ---------------------------------------------------------------------------------------------------- the HIP path (CLI)

def _inflate(raw):
    assert raw[-28:] == EOF_BLOCK, "no BGZF end-of-file block"
    return gzip.decompress(raw)


def _run_fusion(args, site=None):
    r = hostlib.run_cli(["fusion"] + (["-f", site] if site else []) + args)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return _inflate(r.stdout), r.stderr.decode()


def _as_inputs(tmp_path, sam):
    """The SAM file, the same as gzip SAM and as BAM (independent encoder + BGZF blocks)."""
    header, refs, recs = fo.parse_sam(sam)
    idx = {name: i for i, (name, _) in enumerate(refs)}
    bam, samgz = str(tmp_path / "in.bam"), str(tmp_path / "in.sam.gz")
    open(bam, "wb").write(fo.bgzf_blocks(fo.header_bytes(header, refs) + b"".join(fo.encode_record(r, idx) for r in recs)))
    with open(sam, "rb") as fi, gzip.open(samgz, "wb", compresslevel=1) as fz:
        fz.write(fi.read())
    return [sam, samgz, bam]


@pytest.mark.gpu
def test_hip_fusion_hand_worked_table(tmp_path):
    sam, site = str(tmp_path / "hand.sam"), str(tmp_path / "site.txt")
    first = _hand_sam(sam)
    inputs = _as_inputs(tmp_path, sam)
    for args, kw in (([], {}), (["-o", "0.25"], dict(ovlp_frac=0.25)), (["-v", "0.05"], dict(each_cov=0.05)), (["-V", "0.9"], dict(all_cov=0.9)),
                     (["--ovlp-frac", "0.25"], dict(ovlp_frac=0.25))):
        want, pairs, want_site, count = fr.expected(sam, **kw)
        for path in inputs if not args else inputs[:1]:
            got, err = _run_fusion(args + [path], site)
            assert got == want, (args, path)
            assert open(site).read() == want_site
            assert err.endswith("[bam_fusion] Candidate gene-fusion transcripts: %d\n" % count)
    assert fr.expected(sam)[1] == _hand_expect(first)[0]


@pytest.mark.gpu
def test_hip_fusion_usage_and_quirks(tmp_path):
    sam = str(tmp_path / "hand.sam")
    _hand_sam(sam)
    for args in (["-d", "5", sam], ["--dis", "5", sam], ["-g", "x", sam], ["--fusion-site", "x", sam], [], [sam, sam]):
        r = hostlib.run_cli(["fusion"] + args, cwd=str(tmp_path))
        assert r.returncode == 1 and r.stdout == b"" and b"Usage:" in r.stderr, args
    assert not os.path.exists(str(tmp_path / "x"))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SYNTH_OPTS)))
def test_hip_fusion_equals_the_restatement(tmp_path, tmp_path_factory, k):
    case = _synth_case(tmp_path_factory)
    want, pairs, want_site, count = case["want"][k]
    site = str(tmp_path / "site.txt")
    for path in (_as_inputs(tmp_path, case["sam"]) if k == 0 else [case["sam"]]):
        got, err = _run_fusion(SYNTH_OPTS[k][0] + [path], site)
        assert got == want, path
        assert open(site).read() == want_site
        assert "[bam_fusion] Candidate gene-fusion transcripts: %d\n" % count in err
    n_groups = len(hostlib.fusion_groups(case["sam"])["rlen"])
    assert 0.05 * n_groups <= count <= 0.80 * n_groups


@pytest.mark.gpu
def test_hip_fusion_empty_and_no_candidate(tmp_path):
    """Header only, and records without a candidate: the header and the end-of-file block, a count of 0."""
    empty, none = str(tmp_path / "empty.sam"), str(tmp_path / "none.sam")
    open(empty, "w").write(HDR)
    with open(none, "w") as fh:
        fh.write(HDR)
        fh.write(_line("a", 0, "chr1", 1000, "60M40S", "*", _aux(60)))
        fh.write(_line("b", 0, "chr1", 1000, "60M40S", "*", _aux(60)))
        fh.write(_line("b", 2048, "chr1", 2000, "60S40M", "*", _aux(40)))
        fh.write("\t".join(["c", "4", "*", "0", "0", "*", "*", "0", "0", "*", "*"]) + "\n")
    for path in (empty, none):
        want, pairs, _, count = fr.expected(path)
        header, refs, _ = fo.parse_sam(path)
        assert pairs == [] and want == fo.header_bytes(header, refs)
        got, err = _run_fusion([path])
        assert got == want and "Candidate gene-fusion transcripts: 0\n" in err


@pytest.mark.gpu
def test_hip_fusion_long_cigar_record(tmp_path):
    """A record of 66 000 operations (stored in the CG tag of a BAM file) as one of the two segments of a candidate, as SAM and as BAM."""
    n_pairs = 33_000
    cigar = "1M1I" * n_pairs + "%dS" % (n_pairs // 2)                             # read 1..66000 of 82500
    tail = "%dS%dM" % (2 * n_pairs, n_pairs // 2)                                 # read 66001..82500
    sam = str(tmp_path / "long.sam")
    with open(sam, "w") as fh:
        fh.write(HDR)
        fh.write(_line("long", 0, "chr1", 1000, cigar, "*", _aux(60000, 7)))
        fh.write(_line("long", 2048, "chr2", 1000, tail, "*", _aux(16000, 0)))
        fh.write(_line("z", 0, "chr2", 50, "20M", "*", _aux(20, 0)))
    want, pairs, _, count = fr.expected(sam)
    assert pairs == [(0, 1)] and b"CGBI" in want
    for path in _as_inputs(tmp_path, sam)[::2]:
        got, _ = _run_fusion([path])
        assert got == want


# ---------------------------------------------------------------------------------------------------- the C-ABI at size

def _random_records(rng, n, ops_lo, ops_hi):
    n_ops = rng.integers(ops_lo, ops_hi + 1, n)
    off = np.zeros(n + 1, np.int64); np.cumsum(n_ops, out=off[1:])
    ops = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint32), size=int(off[-1]))
    lens = rng.integers(1, 400, size=int(off[-1])).astype(np.uint32)
    first = off[:-1]
    clip = rng.random(n)
    ops[first[clip < 0.3]] = 4; ops[first[(clip >= 0.3) & (clip < 0.4)]] = 5
    flag = (np.where(rng.random(n) < 0.03, 4, 0) | np.where(rng.random(n) < 0.5, 16, 0)).astype(np.uint16)
    pos = rng.integers(0, 3_000_000, n).astype(np.int32)
    return flag, pos, off, (lens << 4) | ops


def _segments_numpy(flag, pos, off, cig):
    """bam2seg as sums (only the first word is special)."""
    n = len(flag)
    ops, lens = (cig & 15).astype(np.int64), (cig >> 4).astype(np.int64)
    rid = np.repeat(np.arange(n), np.diff(off))

    def total(which):
        return np.bincount(rid, weights=np.where(np.isin(ops, which), lens, 0), minlength=n).astype(np.int64)

    q_al, r_al, qlen = total([0, 1, 7, 8]), total([0, 2, 3, 7, 8]), total([0, 1, 4, 7, 8])
    w0 = cig[off[:-1]]
    clip0 = np.where(((w0 & 15) == 4) | ((w0 & 15) == 5), (w0 >> 4).astype(np.int64), 0)
    rs, re = 1 + clip0, clip0 + q_al
    rev = (flag & 16) != 0
    rs, re = np.where(rev, qlen + 1 - re, rs), np.where(rev, qlen + 1 - rs, re)
    fs, fe = pos.astype(np.int64) + 1, pos.astype(np.int64) + r_al
    un = (flag & 4) != 0
    return tuple(np.where(un, 0, x).astype(np.int32) for x in (rs, re, fs, fe, qlen))


@pytest.mark.gpu
@pytest.mark.parametrize("n,ops_lo,ops_hi,auto_wave", [(200_000, 1, 12, 0.0), (20_000, 200, 400, 1.0)])
def test_c_abi_fusion_segments_at_size(monkeypatch, n, ops_lo, ops_hi, auto_wave):
    """l2r_fusion_segments: the thread form and the wave form give the same rows, both equal the numpy sums; left to itself the
    engine takes the wave form above 32 operations a record."""
    from lr2rmats_amd import capi
    flag, pos, off, cig = _random_records(np.random.default_rng(n), n, ops_lo, ops_hi)
    want = _segments_numpy(flag, pos, off, cig)
    eng = capi.Engine(0)
    try:
        for wave in ("0", "1", None):
            if wave is None:
                monkeypatch.delenv("L2R_FUSION_WAVE", raising=False)
            else:
                monkeypatch.setenv("L2R_FUSION_WAVE", wave)
            got = eng.fusion_segments(flag, pos, off, cig)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)
            assert eng.fusion_stats()["wave_form"] == (auto_wave if wave is None else float(wave))
    finally:
        eng.close()


def _select_case():
    """Groups of 1..6 rows and one of 3 000: in most the first two rows split the read at a point (+- an overlap, a gap at the end, the
    second part 100000 - 1 / + 0 / + 1 behind the first on one chromosome); rlen 0 and negative, spans with end < start, ends past rlen."""
    rng = np.random.default_rng(5)
    gl = np.concatenate([rng.integers(1, 7, 6000), [3000], rng.integers(1, 7, 50)])
    goff = np.concatenate([[0], np.cumsum(gl)]).astype(np.int64)
    R, G = int(goff[-1]), len(gl)
    rlen = (100 * rng.integers(1, 4, G)).astype(np.int32)
    rlen[::97] = 0; rlen[5::101] = -7
    L = np.repeat(np.maximum(rlen, 100), gl)
    rs = rng.integers(1, L).astype(np.int32)
    re = np.minimum(rs + rng.integers(0, L), L + rng.integers(0, 3, R)).astype(np.int32)
    head = goff[:-1]
    cut = rng.integers(20, 80, G)
    two = gl >= 2                                            # most groups: the first two rows split the read at a point, +- an overlap
    rs[head[two]] = 1; re[head[two]] = (cut * np.maximum(rlen, 100) // 100)[two]
    rs[head[two] + 1] = re[head[two]] + 1 - rng.choice([0, 0, 0, 1, 5, 20], two.sum()); re[head[two] + 1] = np.maximum(rlen, 100)[two] - rng.choice([0, 0, 0, 1, 2, 3], two.sum())
    neg = rng.random(R) < 0.02
    re[neg] = rs[neg] - rng.integers(1, 5, neg.sum())                            # end < start
    score = rng.integers(0, 6, R).astype(np.int32) * 10; ed = rng.integers(0, 3, R).astype(np.int32)
    score[head[two]] += 100; score[head[two] + 1] += 50
    tid = rng.integers(0, 3, R).astype(np.int32)
    fs = rng.integers(1, 400_000, R).astype(np.int32); fe = (fs + rng.integers(-2, 3000, R)).astype(np.int32)
    same = two & (rng.random(G) < 0.3)                       # same chromosome, second part 100000 -1 / +0 / +1 behind the first
    tid[head[same] + 1] = tid[head[same]]
    fs[head[same] + 1] = fe[head[same]] + rng.choice([99999, 100000, 100001], same.sum())
    fe[head[same] + 1] = fs[head[same] + 1] + 500
    return goff, score, ed, tid, rs, re, fs, fe, rlen


def _select_literal(goff, score, ed, tid, rs, re, fs, fe, rlen):
    G = len(goff) - 1
    w1, w2 = np.full(G, -1, np.int64), np.full(G, -1, np.int64)
    for g in range(G):
        a, b = int(goff[g]), int(goff[g + 1])
        if b - a < 2:
            continue
        segs = [fr.Seg(k, int(tid[k]), False, int(score[k]), int(ed[k]), int(rs[k]), int(re[k]), int(fs[k]), int(fe[k])) for k in range(a, b)]
        sel = fr.check_fusion(segs, int(rlen[g]))
        if sel is not None and len(sel) == 2:
            w1[g], w2[g] = sel[0].row, sel[1].row
    return w1, w2


@pytest.mark.gpu
def test_c_abi_fusion_select_equals_the_literal_loop():
    """l2r_fusion_select on groups of 1..6 rows, one group of 3 000 rows, rlen 0 / negative and spans with end < start, against
    check_fusion() of the restatement; empty groups and null arguments are rejected."""
    from lr2rmats_amd import capi
    goff, score, ed, tid, rs, re, fs, fe, rlen = _select_case()
    G = len(goff) - 1
    prm = capi.CFusionParams(0.1, 0.1, 0.99, 100000)
    eng = capi.Engine(0)
    try:
        first, second = eng.fusion_select(goff, score, ed, tid, rs, re, fs, fe, rlen, prm)
        w1, w2 = _select_literal(goff, score, ed, tid, rs, re, fs, fe, rlen)
        np.testing.assert_array_equal(first, w1)
        np.testing.assert_array_equal(second, w2)
        assert 0.05 * G < (w1 >= 0).sum() < 0.8 * G
        # argument checks, as l2r_filter_select
        bad = goff.copy(); bad[3] = bad[2]
        with pytest.raises(capi.L2RError, match="group 2 is empty"):
            eng.fusion_select(bad, score, ed, tid, rs, re, fs, fe, rlen, prm)
        lib = eng.lib
        assert lib.l2r_fusion_select(eng.ctx, G, goff.ctypes.data, None, ed.ctypes.data, tid.ctypes.data, rs.ctypes.data, re.ctypes.data, fs.ctypes.data,
                                     fe.ctypes.data, rlen.ctypes.data, None, first.ctypes.data, second.ctypes.data) != 0
        assert b"l2r_fusion_select" in lib.l2r_last_error()
        assert lib.l2r_fusion_segments(eng.ctx, None, None, None, None, None, None) != 0 and b"l2r_fusion_segments" in lib.l2r_last_error()
    finally:
        eng.close()
