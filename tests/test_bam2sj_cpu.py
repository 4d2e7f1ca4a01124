"""`lr2rmats bam2sj` without a GPU: hand-worked answers for the restatement (tests/sj_restatement.py), the host's FASTA reader,
its record source and its literal junction list (lr2rmats_amd/host/sj.c through ctypes)."""
import gzip

import numpy as np
import pytest

from lr2rmats_amd import hostlib
from tests import sj_cases as sc
from tests import sj_restatement as sr


def _rows(line, min_intron=3):
    _, recs = sr.records_from_sam(sc.HDR + line)
    return sr.rows_in_record_order(recs, min_intron)


# ---------------------------------------------------------------------------------------------------- hand-worked answers
# POS is 1-based; `end` starts at POS - 1, grows by M = X D N; an N of >= -i bases emits (end + 1, end + len) first.

def test_intron_length_threshold():
    # POS 101: end 100, 10M -> 110; 3N: 3 >= 3 kept -> (111, 113); 2N: 2 < 3 only grows end
    assert _rows(sc.sam_line("a", 3, "chr1", 101, "10M3N10M", ["NH:i:1"])) == [(0, 111, 113, 1, 0)]
    assert _rows(sc.sam_line("a", 3, "chr1", 101, "10M2N10M", ["NH:i:1"])) == []
    # -i 4: the 3N is below it; the short N still moves the next junction: 110 + 3 + 5 = 118 -> (119, 128)
    assert _rows(sc.sam_line("a", 3, "chr1", 101, "10M3N5M10N5M", ["NH:i:1"]), 4) == [(0, 119, 128, 1, 0)]
    # -i 2 keeps the 2N: (111, 112)
    assert _rows(sc.sam_line("a", 3, "chr1", 101, "10M2N10M", ["NH:i:1"]), 2) == [(0, 111, 112, 1, 0)]


def test_operations_that_move_the_donor_and_those_that_do_not():
    # D: 200 + 5 + 2 + 5 = 212 -> (213, 312)
    assert _rows(sc.sam_line("a", 3, "chr1", 201, "5M2D5M100N5M", ["NH:i:1"])) == [(0, 213, 312, 1, 0)]
    # = and X: 200 + 4 + 3 + 6 = 213 -> (214, 313)
    assert _rows(sc.sam_line("a", 3, "chr1", 201, "4=3X6M100N5M", ["NH:i:1"])) == [(0, 214, 313, 1, 0)]
    # H S I P (and B) add nothing: 300 + 5 + 5 = 310 -> (311, 360)
    assert _rows(sc.sam_line("a", 3, "chr1", 301, "3H5S5M2I1P5M50N5M", ["NH:i:1"])) == [(0, 311, 360, 1, 0)]
    assert _rows(sc.sam_line("a", 3, "chr1", 301, "5M4B5M50N5M", ["NH:i:1"])) == [(0, 311, 360, 1, 0)]


def test_two_introns_and_an_intron_first():
    # 400 + 10 = 410 -> (411, 430); end 430 + 10 = 440 -> (441, 470)
    assert _rows(sc.sam_line("a", 3, "chr1", 401, "10M20N10M30N10M", ["NH:i:1"])) == [(0, 411, 430, 1, 0), (0, 441, 470, 1, 0)]
    # N as the first op: end = 500 -> (501, 540)
    assert _rows(sc.sam_line("a", 3, "chr1", 501, "40N10M", ["NH:i:1"])) == [(0, 501, 540, 1, 0)]


def test_nh_verdicts():
    j = "10M25N10M"                                        # POS 601: (611, 635)
    assert _rows(sc.sam_line("a", 3, "chr1", 601, j, ["NH:i:1"])) == [(0, 611, 635, 1, 0)]
    assert _rows(sc.sam_line("a", 3, "chr1", 601, j, ["NH:i:2"])) == [(0, 611, 635, 0, 1)]
    assert _rows(sc.sam_line("a", 3, "chr1", 601, j, [])) == [(0, 611, 635, 0, 1)]             # missing: multi-mapped
    assert _rows(sc.sam_line("a", 3, "chr1", 601, j, ["NH:Z:1"])) == [(0, 611, 635, 0, 1)]     # not an integer: value 0
    assert _rows(sc.sam_line("a", 3, "chr1", 601, j, ["NM:i:1", "NH:i:1"])) == [(0, 611, 635, 1, 0)]
    # one junction from a uniquely and a multiply mapped record: uniq_c 1, multi_c 1
    two = sc.sam_line("a", 3, "chr1", 601, j, ["NH:i:1"]) + sc.sam_line("b", 3, "chr1", 601, j, ["NH:i:3"])
    assert sr.literal_list(_rows(two)) == [(0, 611, 635, 1, 1)]
    assert sr.sorted_table(_rows(two)) == [(0, 611, 635, 1, 1)]


def test_record_filter():
    j = "10M25N10M"
    assert _rows(sc.sam_line("a", 1, "chr1", 601, j, ["NH:i:1"])) == []      # paired, not proper: skipped (with and without -p:
    assert _rows(sc.sam_line("a", 0, "chr1", 601, j, ["NH:i:1"])) == []      #  the restatement has no switch, as the reference has none)
    assert _rows(sc.sam_line("a", 7, "chr1", 601, j, ["NH:i:1"])) == []      # unmapped
    assert _rows(sc.sam_line("a", 3, "chr1", 601, "*", ["NH:i:1"])) == []    # no CIGAR: treated as unmapped
    assert _rows(sc.sam_line("a", 0x63, "chr1", 601, j, ["NH:i:1"])) == [(0, 611, 635, 1, 0)]
    # 'No "NH" tag.' comes for a mapped record without the tag, also one the pair test skips afterwards; not for an unmapped one
    text = sc.HDR + sc.sam_line("a", 3, "chr1", 601, j, []) + sc.sam_line("b", 0, "chr1", 601, j, []) + sc.sam_line("c", 7, "chr1", 601, j, [])
    assert sr.missing_nh_messages(text) == 2


def test_hand_file_table_and_bytes():
    names, recs = sr.records_from_sam(sc.hand_sam())
    assert names == sc.NAMES
    rows = sr.rows_in_record_order(recs)
    assert sr.literal_list(rows) == sc.HAND_TABLE == sr.sorted_table(rows)
    assert sr.missing_nh_messages(sc.hand_sam()) == sc.HAND_NO_NH_MESSAGES
    out = sr.expected_stdout(sc.hand_sam()).decode().splitlines()
    assert out[:4] == sr.HEADER.splitlines() and len(out) == 4 + len(sc.HAND_TABLE)
    assert out[4] == "chr1\t111\t113\t0\t1\t1\t0\t0" and out[11] == "chr1\t611\t635\t0\t1\t1\t1\t0" and out[-1] == "chr2\t61\t1060\t0\t1\t1\t0\t0"
    assert sr.expected_stdout(sc.no_junction_sam()) == sr.HEADER.encode()


def test_motifs_of_the_restatement():
    #            1234567890123456
    seqs = ["AAGTCCCCAGAAgtccagTT", "ACGT"]
    assert sr.motif_of(seqs, 0, 3, 10) == (1, 1)           # bases 3,4 = GT, 9,10 = AG
    assert sr.motif_of(seqs, 0, 13, 18) == (1, 1)          # lower case is upper-cased
    assert sr.motif_of(seqs, 0, 3, 9) == (0, 0)            # GT..CA
    assert sr.motif_of(seqs, 0, 3, 20) == (0, 0)           # GT..TT, acceptor on the last base
    assert sr.motif_of(seqs, 0, 3, 21) == (0, 0)           # acceptor beyond the sequence: matches nothing
    assert sr.motif_of(None, 5, 3, 10) == (0, 0)           # no -g
    with pytest.raises(sr.UnknownTid):
        sr.motif_of(seqs, 2, 1, 2)


def test_numpy_form_equals_the_literal_one():
    rec = sc.synth_records(3000, 11, n_intron=60)          # 300 introns: every junction repeats
    _, recs = sr.records_from_sam(sc.records_sam(rec))
    rows = sr.rows_in_record_order(recs)
    got = sr.table_numpy(*sr.rows_numpy(rec["flag"], rec["tid"], rec["pos"], rec["uniq"], rec["cig_off"], rec["cig"]))
    assert [tuple(int(c[i]) for c in got) for i in range(len(got[0]))] == sr.literal_list(rows)
    assert len(got[0]) > 200 and len(rows) > 2 * len(got[0])


def test_heavy_digit_rows_and_the_restatement():
    """The input of the GPU tests of the scatter's rank across waves and rounds: what it promises, and that the restatement takes it."""
    tile = 4096
    n = 3 * tile + 17
    for seed in (5, 6):
        rows, differ = sc.heavy_digit_rows(n, seed)
        assert differ == 7
        for col in (rows[2], rows[0]):                                      # the lowest byte of acc, of tid
            low = col & 0xff
            assert np.bincount(low).max() > 0.75 * n and min(np.bincount(low[t:t + tile]).max() for t in (0, tile, 2 * tile)) > 10 * 256
        got = sr.table_numpy(*rows)
        assert len(got[0]) == n - n // 10 == len(np.unique(np.stack(rows[:3], axis=1), axis=0))
        assert int(got[3].sum()) == int(rows[3].sum()) and int(got[4].sum()) == int(rows[4].sum())
        key = [tuple(int(c[i]) for c in got[:3]) for i in range(len(got[0]))]
        assert key == sorted(key)


# ---------------------------------------------------------------------------------------------------- host library

FASTA = ">chrB second in the header\nACGTacgt\nNNNN\n\n>chrA\r\nGGGG\r\nCC\n>empty\n>chrC desc\tx\nTTTTTTTTTT\nAC"      # no newline at the end
FASTA_SEQS = [("chrB", "ACGTacgtNNNN"), ("chrA", "GGGGCC"), ("empty", ""), ("chrC", "TTTTTTTTTTAC")]


@pytest.mark.parametrize("gz", [False, True])
def test_fasta_reader(tmp_path, gz):
    path = str(tmp_path / ("g.fa.gz" if gz else "g.fa"))
    with (gzip.open(path, "wt", newline="") if gz else open(path, "w", newline="")) as fh:
        fh.write(FASTA)
    names, off, bases = hostlib.read_fasta(path)
    # file order, not the order of any header; lower case kept as it is (the motif lookup upper-cases); wrapped lines joined
    assert names == [n for n, _ in FASTA_SEQS]
    assert off.tolist() == np.cumsum([0] + [len(s) for _, s in FASTA_SEQS]).tolist()
    assert bytes(bases).decode() == "".join(s for _, s in FASTA_SEQS)


def test_fasta_reader_empty_file(tmp_path):
    path = str(tmp_path / "e.fa")
    open(path, "w").close()
    names, off, bases = hostlib.read_fasta(path)
    assert names == [] and off.tolist() == [0] and len(bases) == 0


def test_literal_list_of_the_host_on_decreasing_tids():
    _, recs = sr.records_from_sam(sc.tids_0_1_0_sam())
    rows = sr.rows_in_record_order(recs)
    want = sr.literal_list(rows)
    assert want != sr.sorted_table(rows)                   # the case is real: the reference's list is no sort here
    assert want == [(0, 11, 60, 1, 0), (0, 111, 160, 1, 0), (1, 11, 60, 1, 0), (0, 111, 160, 0, 1), (0, 311, 360, 1, 0), (1, 511, 560, 0, 1)]
    got = hostlib.sj_literal(*[np.array(c, np.int32) for c in zip(*rows)])
    assert [tuple(int(c[i]) for c in got) for i in range(len(got[0]))] == want


def test_literal_list_of_the_host_at_size():
    # non-decreasing tids: the list is the sorted table; then the same rows with the chromosomes in falling order
    rec = sc.synth_records(4000, 3)
    rows = sr.rows_numpy(rec["flag"], rec["tid"], rec["pos"], rec["uniq"], rec["cig_off"], rec["cig"])
    got = hostlib.sj_literal(*rows)
    want = sr.table_numpy(*rows)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    back = [np.asarray(c)[::-1] for c in rows]
    lit = sr.literal_list(list(zip(*[c.tolist() for c in back])))
    got = hostlib.sj_literal(*back)
    assert [tuple(int(c[i]) for c in got) for i in range(len(got[0]))] == lit
    assert hostlib.sj_literal(*[np.zeros(0, np.int32)] * 5)[0].size == 0


@pytest.mark.parametrize("batch", [1, 7, 1 << 20])
def test_record_source_reads_every_format(tmp_path, batch):
    text = sc.hand_sam()
    _, recs = sr.records_from_sam(text)
    for path in sc.write_inputs(tmp_path, "hand", text):
        got = hostlib.sj_read_records(path, batch)
        assert got["names"] == sc.NAMES
        assert got["flag"].tolist() == [r["flag"] for r in recs]
        assert got["tid"].tolist() == [r["tid"] for r in recs] and got["pos"].tolist() == [r["pos"] for r in recs]
        assert got["uniq"].tolist() == [int(r["uniq"]) for r in recs] and got["nh_seen"].tolist() == [int(r["has_nh"]) for r in recs]
        assert got["cig_off"].tolist() == np.cumsum([0] + [len(r["cigar"]) for r in recs]).tolist()
        assert got["cig"].tolist() == [(l << 4) | op for r in recs for l, op in r["cigar"]]


def test_record_source_long_lines_and_last_line_without_newline(tmp_path):
    # a 300-operation CIGAR and a record whose line is longer than one read of the stream; no newline at the end of the file
    cigar = "".join("%dM%dN" % (3 + k % 5, 3 + k % 7) for k in range(150)) + "5M"
    text = sc.HDR + sc.sam_line("long", 3, "chr1", 11, cigar, ["XX:Z:" + "x" * (5 << 20), "NH:i:1"]) + sc.sam_line("b", 3, "chr2", 5, "4M", ["NH:i:1"])[:-1]
    path = str(tmp_path / "l.sam")
    with open(path, "w") as fh:
        fh.write(text)
    got = hostlib.sj_read_records(path, 1)
    assert got["cig_off"].tolist() == [0, 301, 302] and got["uniq"].tolist() == [1, 1] and got["tid"].tolist() == [0, 1]
    assert got["cig"][:2].tolist() == [(3 << 4) | 0, (3 << 4) | 3] and got["cig"][-1] == (4 << 4)
