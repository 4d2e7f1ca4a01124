"""`lr2rmats sjtab` on the GPU: the overhang column, the annotated flag and the filter through the C-ABI against the restatement
(tests/sjtab_restatement.py), every column equal; the command against the restatement byte for byte; its output given to `update-gtf -j`."""
import os
import re

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import sj_cases as sc
from tests import sj_restatement as sr
from tests import sjtab_restatement as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ("tid", "don", "acc", "strand", "motif", "anno", "uniq_c", "multi_c", "max_over")
ZEROS = "0,0,0,0,0"


def _cli(args, env=None):
    p = hostlib.run_cli(["sjtab"] + list(args), env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def _sort_tile():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    return int(re.search(r"#define\s+L2R_SJ_SORT_TILE\s+(\d+)", text).group(1))


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def _six(t):
    return (t.tid, t.don, t.acc, t.uniq_c, t.multi_c, t.max_over)


def _assert_six(got, want):
    for g, w, name in zip(_six(got), want, ("tid", "don", "acc", "uniq_c", "multi_c", "max_over")):
        assert np.array_equal(g.astype(np.int64), np.asarray(w, np.int64)), name


def _records(recs):
    """[(flag, tid, pos, uniq, cigar text)] -> the columns of sj_add."""
    cig, off = [], [0]
    for r in recs:
        cig += [(ln << 4) | op for ln, op in sr.parse_cigar(r[4])]
        off.append(len(cig))
    return dict(flag=np.array([r[0] for r in recs], np.uint16), tid=np.array([r[1] for r in recs], np.int32), pos=np.array([r[2] for r in recs], np.int32),
                uniq=np.array([r[3] for r in recs], np.uint8), cig_off=np.array(off, np.int64), cig=np.array(cig, np.uint32))


def _add(eng, r, a=0, b=None):
    b = len(r["flag"]) if b is None else b
    c0, c1 = r["cig_off"][a], r["cig_off"][b]
    eng.sj_add(r["flag"][a:b], r["tid"][a:b], r["pos"][a:b], r["uniq"][a:b], r["cig_off"][a:b + 1] - c0, r["cig"][c0:c1])


def _table_of_records(eng, r, min_intron=3, pair_only=False, cuts=None):
    eng.sj_begin_tab(min_intron=min_intron, pair_only=pair_only)
    cuts = cuts or [0, len(r["flag"])]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _add(eng, r, a, b)
    got = eng.sj_finish()
    want = st.table_numpy(*st.rows_numpy(r["flag"], r["tid"], r["pos"], r["uniq"], r["cig_off"], r["cig"], min_intron, pair_only))
    _assert_six(got, want)
    assert not got.anno.any() and not got.strand.any() and not got.motif.any()
    return got


# ---------------------------------------------------------------------------------------------------- 1: overhangs

def test_empty_one_row_and_no_junctions(eng):
    eng.sj_begin_tab()
    t = eng.sj_finish()
    assert isinstance(t, capi.SjTab) and all(getattr(t, n).size == 0 for n in NINE)
    assert eng.sj_filter_rows().tid.size == 0
    eng.sj_begin_tab()
    eng.sj_add_rows_over([2], [10], [20], [3], [4], [17])
    t = eng.sj_finish()
    assert [getattr(t, n).tolist() for n in NINE] == [[2], [10], [20], [0], [0], [0], [3], [4], [17]]
    # rows without the column get overhang 0 and merge with rows that carry it
    eng.sj_begin_tab()
    eng.sj_add_rows([2, 3], [10, 10], [20, 20], [1, 1], [0, 0])
    eng.sj_add_rows_over([2], [10], [20], [0], [5], [9])
    t = eng.sj_finish()
    assert [c.tolist() for c in _six(t)] == [[2, 3], [10, 10], [20, 20], [1, 1], [5, 0], [9, 0]]
    r = _records([(3, 0, 10, 1, "50M"), (3, 0, 20, 1, "20M2N20M"), (3, 1, 4, 1, "10M5D10M"), (4, 0, 4, 1, "10M50N10M")])
    assert _table_of_records(eng, r).tid.size == 0


def test_hand_cigars(eng):
    recs = [(3, 0, 1000 * (k + 1), 1, c[1]) for k, c in enumerate(st.HAND_CIGARS) if c[2] == 3]
    want_over = [o for c in st.HAND_CIGARS if c[2] == 3 for o in c[3]]
    got = _table_of_records(eng, _records(recs))
    assert got.max_over.tolist() == want_over                              # (one record per 1000 bases: the rows come out in record order)
    assert want_over[:6] == [7, 5, 5, 9, 0, 7]
    # -i 2: the 2N of the long one is a junction of its own
    got = _table_of_records(eng, _records([(3, 0, 100, 1, "3S8M2I4M2D3M2N6M50N9M")]), min_intron=2)
    assert got.max_over.tolist() == [6, 6]
    # three records at one junction with overhangs 4, 31 and 12; -p drops the one without FLAG & 2
    r = _records([(3, 0, 996, 1, "4M100N50M"), (3, 0, 960, 0, "40M100N31M"), (3, 0, 988, 1, "12M100N12M"), (0, 0, 940, 1, "60M100N60M")])
    assert [c.tolist() for c in _six(_table_of_records(eng, r))] == [[0], [1001], [1100], [3], [1], [60]]
    assert [c.tolist() for c in _six(_table_of_records(eng, r, pair_only=True))] == [[0], [1001], [1100], [2], [1], [31]]


def test_long_cigar(eng):
    ops = []
    for k in range(100):
        ops += [(5 + (k * 7) % 11, 0), (1, 1) if k % 2 else (2, 2), (10 + k, 3)]
    cig = np.array([(l << 4) | op for l, op in ops], np.uint32)
    r = dict(flag=np.array([3, 3], np.uint16), tid=np.zeros(2, np.int32), pos=np.array([100, 100], np.int32), uniq=np.array([1, 0], np.uint8),
             cig_off=np.array([0, 300, 600], np.int64), cig=np.concatenate([cig, cig]))
    got = _table_of_records(eng, r)
    block = [5 + (k * 7) % 11 for k in range(100)] + [0]                    # the last N is the last operation
    assert got.tid.size == 100 and got.max_over.tolist() == [min(block[k], block[k + 1]) for k in range(100)]
    assert got.uniq_c.tolist() == [1] * 100 and got.multi_c.tolist() == [1] * 100 and len(set(got.max_over.tolist())) > 5


def test_one_key_from_5000_records(eng):
    n = 5000
    over = (np.arange(n) * 37) % 1000
    over[2777] = 1500                                                      # the single largest: inside a wave, away from any workgroup edge
    assert 2777 % 64 not in (0, 63) and 2777 % 256 not in (0, 255) and (over == over.max()).sum() == 1
    left = 2000
    recs = [(3, 4, 100000 - left, i % 2, "%dM100N%s" % (left, "%dM" % over[i] if over[i] else "")) for i in range(n)]
    got = _table_of_records(eng, _records(recs))
    assert [c.tolist() for c in _six(got)] == [[4], [100001], [100100], [n // 2], [n // 2], [1500]]
    # the same through add_rows_over: counts are column sums
    eng.sj_begin_tab()
    eng.sj_add_rows_over(np.full(n, 4), np.full(n, 1000), np.full(n, 2000), np.full(n, 3), np.arange(n) % 2, over)
    t = eng.sj_finish()
    assert [c.tolist() for c in _six(t)] == [[4], [1000], [2000], [15000], [2500], [1500]]


def _rows_table(eng, rows, pieces=1):
    cols = [np.asarray(c, np.int32) for c in rows]
    eng.sj_begin_tab()
    cut = np.linspace(0, len(cols[0]), pieces + 1).astype(int)
    for a, b in zip(cut[:-1], cut[1:]):
        eng.sj_add_rows_over(*[c[a:b] for c in cols])
    got = eng.sj_finish()
    _assert_six(got, st.table_numpy(*cols))
    return got


def test_runs_across_tile_boundaries(eng):
    tile = _sort_tile()
    n = 3 * tile + 17
    rng = np.random.default_rng(2)
    key = np.arange(n, dtype=np.int64)
    for b in (tile, 2 * tile, 3 * tile):
        key[b - 300:b + 300] = b                                           # a 600-row run across the boundary
        key[b - 700:b - 636] = b - 700                                     # a 64-row run inside
    key[n - 10:] = n                                                       # a run that ends the table
    k = key[rng.permutation(n)]
    rows = [(k >> 20).astype(np.int32), ((k >> 8) & 0xfff).astype(np.int32) + 1, (k & 0xff).astype(np.int32) * 3 + 5,
            rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 100000, n).astype(np.int32)]
    got = _rows_table(eng, rows)
    assert got.tid.size == len(np.unique(key)) < n and eng.sj_stats()["rows_in"] == n
    # numpy's np.maximum.at, spelled out
    _, inv = np.unique(np.stack(rows[:3], axis=1).astype(np.int64), axis=0, return_inverse=True)
    mx = np.zeros(got.tid.size, np.int64)
    np.maximum.at(mx, inv.reshape(-1), rows[5].astype(np.int64))
    assert np.array_equal(got.max_over.astype(np.int64), mx)
    os.environ["L2R_SJ_COMPACT_ROWS"] = "1000"
    try:
        again = _rows_table(eng, rows, pieces=7)
        assert eng.sj_stats()["rounds"] > 2
    finally:
        del os.environ["L2R_SJ_COMPACT_ROWS"]
    assert all(np.array_equal(getattr(got, c), getattr(again, c)) for c in NINE)


def test_one_digit_value_holds_most_of_a_tile(eng):
    """The six-column scatter's rank across waves and rounds: two of the passes see one digit value in four rows of five."""
    tile = _sort_tile()
    n = 3 * tile + 17
    rows, differ = sc.heavy_digit_rows(n, 6)
    rows.append(np.random.default_rng(7).integers(0, 100000, n).astype(np.int32))
    low = rows[2] & 0xff
    assert differ == 7 and np.bincount(low).max() > 0.75 * n and np.bincount(low[:tile]).max() > 10 * 256
    for pieces in (1, 7):
        got = _rows_table(eng, rows, pieces=pieces)                         # (the maximum overhang per key: st.table_numpy)
        stats = eng.sj_stats()
        assert stats["rows_in"] == n and stats["rounds"] == 1 and stats["radix_passes"] == differ
    assert got.tid.size == n - n // 10 and len(set(got.max_over.tolist())) > 1000


# ---------------------------------------------------------------------------------------------------- 2: at size; filter

@pytest.fixture(scope="module")
def records200k():
    # n_intron 4000: about 19 000 junctions, of which the default filter keeps about 80 % (chosen with the restatement, see test_filter)
    return sc.synth_records(200000, 5, n_intron=4000)


@pytest.fixture(scope="module")
def table200k(records200k):
    r = records200k
    return st.table_numpy(*st.rows_numpy(r["flag"], r["tid"], r["pos"], r["uniq"], r["cig_off"], r["cig"]))


def test_table_at_size(eng, records200k, table200k):
    r = records200k
    assert len(table200k[0]) > 10000 and len(set(table200k[5].tolist())) > 50
    runs = [_table_of_records(eng, r, cuts=cuts) for cuts in ([0, 200000], [0, 1, 70000, 70001, 199999, 200000])]
    for got in runs:
        _assert_six(got, table200k)
    assert all(np.array_equal(getattr(runs[0], c), getattr(runs[1], c)) for c in NINE)


def _genome():
    rng = np.random.default_rng(9)
    off = (np.arange(6) * 400000).astype(np.int64)
    return off, np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, int(off[-1]))]


def _anno_of_rows(tid, don, acc):
    """Two-exon transcripts whose intron is the given row."""
    n = len(tid)
    ex_start = np.stack([don - 50, acc + 1], axis=1).reshape(-1)
    ex_end = np.stack([don - 1, acc + 50], axis=1).reshape(-1)
    return np.asarray(tid, np.int32), (2 * np.arange(n + 1)).astype(np.int64), ex_start.astype(np.int32), ex_end.astype(np.int32)


def test_filter(eng, records200k, table200k):
    r = records200k
    off, bases = _genome()
    want = table200k
    strand, motif = sr.motifs_numpy(off, bases, want[0], want[1], want[2])
    sel = np.arange(len(want[0])) % 5 == 0
    a = _anno_of_rows(want[0][sel], want[1][sel], want[2][sel])
    introns = st.annotation_introns(*a)
    anno = st.anno_numpy(introns, want[0], want[1], want[2])
    assert np.array_equal(anno != 0, sel)
    nine = (want[0], want[1], want[2], strand, motif, anno, want[3], want[4], want[5])
    cat = st.category_numpy(anno, motif)
    assert np.bincount(cat, minlength=5).min() > 0                          # all five categories occur

    def table():
        eng.sj_begin_tab(genome=(off, bases))
        _add(eng, r)
        t = eng.sj_finish()
        eng.sj_annotate(*a)
        return t

    def check(got, keep):
        for name, w in zip(NINE, nine):
            assert np.array_equal(getattr(got, name).astype(np.int64), np.asarray(w, np.int64)[keep]), name

    t = table()
    assert np.array_equal(t.strand, strand) and np.array_equal(t.motif, motif) and not t.anno.any()      # (downloaded in front of the annotate)
    keep = st.keep_numpy(anno, motif, want[3], want[4], want[5])
    assert 0.1 < keep.mean() < 0.9
    check(eng.sj_filter_rows(), keep)
    stt = eng.sj_stats()
    assert stt["rows_dropped"] == (~keep).sum() and stt["anno_introns"] == len(introns)
    # a second filter works on what the first left
    tight = ((40,) * 5, (0,) * 5, (0,) * 5)
    check(eng.sj_filter_rows(*tight), keep & st.keep_numpy(anno, motif, want[3], want[4], want[5], tight))
    table()
    check(eng.sj_filter_rows(*st.KEEP_ALL), np.ones(len(keep), bool))
    assert eng.sj_stats()["rows_dropped"] == 0
    table()
    none = eng.sj_filter_rows((1 << 30,) * 5, (0,) * 5, (0,) * 5)
    assert all(getattr(none, n).size == 0 for n in NINE) and eng.sj_stats()["rows_dropped"] == len(keep)
    # the first and the last row are the only survivors: two rows in front of and behind everything else, alone above the thresholds
    eng.sj_begin_tab(genome=(off, bases))
    _add(eng, r)
    big = 1 << 20
    far = 1 << 29
    eng.sj_add_rows_over([0, 4], [1, far], [5, far + 10], [big, big], [0, 7], [big, big + 1])
    n_all = eng.sj_finish().tid.size
    assert n_all == len(keep) + 2
    two = eng.sj_filter_rows((big,) * 5, (big,) * 5, (0x7fffffff,) * 5)
    assert [c.tolist() for c in _six(two)] == [[0, 4], [1, far], [5, far + 10], [big, big], [0, 7], [big, big + 1]]
    assert eng.sj_stats()["rows_dropped"] == n_all - 2


# ---------------------------------------------------------------------------------------------------- 3: annotation

def test_annotation(eng):
    af = synth.make_annotation(8000, 7).in_file_order()
    a = (af.tx_tid, af.tx_ex_off, af.ex_start, af.ex_end)
    introns = st.annotation_introns(*a)
    assert len(introns) > 2000
    own = np.array(sorted(introns), np.int64)
    rng = np.random.default_rng(4)
    m = 5000
    pick = own[rng.integers(0, len(own), m)]
    # random rows: the annotation's own introns with one coordinate moved by one, and rows anywhere
    near = np.stack([pick[:, 0], pick[:, 1] + rng.integers(0, 2, m), pick[:, 2] + 1], axis=1)
    far = np.stack([rng.integers(0, 30, m), rng.integers(1, 1 << 28, m), rng.integers(1, 1 << 28, m)], axis=1)
    rows = np.concatenate([own, near, far])
    rows = rows[rng.permutation(len(rows))]
    cols = [rows[:, 0], rows[:, 1], rows[:, 2], np.ones(len(rows)), np.zeros(len(rows)), rng.integers(0, 100, len(rows))]

    def table():
        eng.sj_begin_tab()
        eng.sj_add_rows_over(*cols)
        return eng.sj_finish()

    t = table()
    assert not t.anno.any()                                                # l2r_sj_annotate never called
    eng.sj_annotate(*a)
    got = eng.sj_download_tab(t.tid.size)
    want = st.anno_numpy(introns, got.tid, got.don, got.acc)
    assert np.array_equal(got.anno, want) and 0 < int(want.sum()) < len(want) and int(want.sum()) == len(introns)
    assert eng.sj_stats()["anno_introns"] == len(introns)
    _assert_six(got, st.table_numpy(*cols))
    # annotated rows stay under thresholds that drop every other row
    only = eng.sj_filter_rows((0, 1000, 1000, 1000, 1000), (0,) * 5, (0,) * 5)
    assert only.anno.all() and only.tid.size == len(introns)
    # no multi-exon transcript; a transcript without a tid
    table()
    first = af.tx_ex_off[:-1]
    eng.sj_annotate(af.tx_tid, np.arange(len(first) + 1), af.ex_start[first], af.ex_end[first])
    assert not eng.sj_download_tab(t.tid.size).anno.any() and eng.sj_stats()["anno_introns"] == 0
    eng.sj_annotate(np.full(len(af.tx_tid), -1, np.int32), af.tx_ex_off, af.ex_start, af.ex_end)
    assert not eng.sj_download_tab(t.tid.size).anno.any()
    eng.sj_annotate(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert not eng.sj_download_tab(t.tid.size).anno.any()


# ---------------------------------------------------------------------------------------------------- 4: the plain table; order of calls

def test_plain_table_refuses_the_new_calls(eng):
    eng.sj_begin()
    eng.sj_add_rows([1], [2], [3], [1], [0])
    with pytest.raises(capi.L2RError, match="l2r_sj_begin_tab"):
        eng.sj_add_rows_over([1], [2], [3], [1], [0], [5])
    t = eng.sj_finish()
    assert type(t) is capi.SjTable and t.tid.tolist() == [1]
    z = (np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    for call in (lambda: eng.sj_annotate(*z), lambda: eng.sj_filter_rows(), lambda: eng.sj_download_tab(1)):
        with pytest.raises(capi.L2RError, match="l2r_sj_begin_tab"):
            call()
    assert eng.sj_finish().tid.tolist() == [1]                             # the table is what it was
    # out of order: in front of l2r_sj_finish
    eng.sj_begin_tab()
    eng.sj_add_rows_over([1], [2], [3], [1], [0], [5])
    for call in (lambda: eng.sj_annotate(*z), lambda: eng.sj_filter_rows(), lambda: eng.sj_download_tab(1)):
        with pytest.raises(capi.L2RError, match="l2r_sj_finish comes first"):
            call()
    with pytest.raises(capi.L2RError, match="negative overhang"):
        eng.sj_add_rows_over([1], [2], [3], [1], [0], [-1])
    assert eng.sj_finish().max_over.tolist() == [5]
    # a plain table after one with the column is the plain table
    eng.sj_begin()
    eng.sj_add_rows([1, 1], [2, 2], [3, 3], [1, 2], [0, 4])
    t = eng.sj_finish()
    assert type(t) is capi.SjTable and t.uniq_c.tolist() == [3] and t.multi_c.tolist() == [4]
    assert len(eng.sj_stats()) > 15 and eng.sj_stats()["rows_dropped"] == 0


# ---------------------------------------------------------------------------------------------------- 5: the command

GTF_LINE = '%s\tsynth\texon\t%d\t%d\t.\t+\t.\tgene_id "%s"; transcript_id "%s"; gene_name "%s"; transcript_name "%s";\n'


def _write_gtf(path, transcripts):
    """transcripts: [(chrom name, [(start, end) ...])]."""
    with open(path, "w") as fh:
        for k, (chrom, exons) in enumerate(transcripts):
            for s, e in exons:
                fh.write(GTF_LINE % (chrom, s, e, "G%d" % k, "T%d" % k, "g%d" % k, "t%d" % k))


def _hand_inputs(tmp_path):
    extra = [("x1", 3, "chr1", 671, "40M25N40M", ["NH:i:1"]),              # (0, 711, 735) again with overhang 40: CT/AC
             ("x2", 3, "chr1", 1466, "35M100N35M", ["NH:i:1"]), ("x3", 3, "chr1", 1466, "35M100N30M", ["NH:i:2"]),
             ("x4", 0, "chr1", 1471, "30M100N60M", []),                    # (0, 1501, 1600): non-canonical, three reads, overhang 35 (30 with -p)
             ("x5", 3, "chr1", 771, "40M25N40M", ["NH:i:1"])]              # (0, 811, 835) with overhang 40: GC/AG
    text = sc.hand_sam() + "".join(sc.sam_line(*x) for x in extra)
    seqs = [list("A" * 1700), list("A" * 1100), list("A" * 60)]
    for t, d, a, b in [(0, 611, 635, "GTAG"), (0, 711, 735, "CTAC"), (0, 811, 835, "gcag"), (0, 911, 935, "ATAC"), (1, 61, 1060, "GTAT")]:
        seqs[t][d - 1], seqs[t][d], seqs[t][a - 2], seqs[t][a - 1] = b
    seqs = ["".join(s) for s in seqs]
    fa = str(tmp_path / "g.fa")
    with open(fa, "w") as fh:
        for name, s in zip(sc.NAMES, seqs):
            fh.write(">%s\n%s\n" % (name, s))
    tx = [("chr1", [(601, 610), (636, 700), (1036, 1100)]),                # introns (611, 635) and (701, 1035)
          ("chr1", [(451, 500), (541, 560)]),                              # (501, 540): the row whose overhang is 0
          ("chrUn", [(101, 110), (114, 150)]),                             # not in the header: no tid, skipped ((111, 113) on chr1 stays novel)
          ("chr2", [(1, 60), (1061, 1100)]), ("chr2", [(1, 60), (1061, 1090)])]
    gtf = str(tmp_path / "a.gtf")
    _write_gtf(gtf, tx)
    names = {n: i for i, n in enumerate(sc.NAMES)}
    tid = [names.get(c, -1) for c, _ in tx]
    ex = [e for _, exons in tx for e in exons]
    off = np.concatenate([[0], np.cumsum([len(exons) for _, exons in tx])])
    introns = st.annotation_introns(tid, off, [e[0] for e in ex], [e[1] for e in ex])
    assert introns == {(0, 611, 635), (0, 701, 1035), (0, 501, 540), (1, 61, 1060)}
    return text, seqs, fa, gtf, introns


def test_cli_hand_file(tmp_path):
    text, seqs, fa, gtf, introns = _hand_inputs(tmp_path)
    want = st.expected_stdout(text, seqs, introns)
    lines = want.decode().splitlines()
    assert lines == ["chr1\t611\t635\t1\t1\t1\t1\t1\t10", "chr1\t711\t735\t2\t2\t0\t1\t1\t40", "chr1\t811\t835\t1\t3\t0\t1\t1\t40",
                     "chr1\t1501\t1600\t0\t0\t0\t1\t2\t35", "chr2\t61\t1060\t2\t6\t1\t1\t0\t10"]
    paths = sc.write_inputs(tmp_path, "hand", text)
    for path in paths:
        rc, out, err = _cli(["-g", fa, "-G", gtf, path])
        assert rc == 0 and out == want, path
        assert "%d records without an NH tag" % st.missing_nh(text) in err
    sam = paths[0]
    base = ["-g", fa, "-G", gtf]
    w = st.expected_stdout(text, seqs, introns, pair_only=True)
    assert _cli(base + ["-p", sam])[1] == w != want and b"chr1\t1501\t1600\t0\t0\t0\t1\t1\t35\n" not in w
    w = st.expected_stdout(text, seqs, introns, min_intron=4, filt=st.KEEP_ALL)
    assert _cli(base + ["-i", "4", "-a", ZEROS, "-U", ZEROS, "-A", ZEROS, sam])[1] == w and b"chr1\t111\t113" not in w
    everything = st.expected_stdout(text, seqs, introns, filt=st.KEEP_ALL)
    assert everything.count(b"\n") == 14 and b"chr1\t111\t113\t0\t0\t0\t1\t0\t10\n" in everything and b"chr1\t501\t540\t0\t0\t1\t1\t0\t0\n" in everything
    for env in (None, {"L2R_SJ_BATCH": 1}, {"L2R_SJ_BATCH": 64}):
        assert _cli(base + ["-a", ZEROS, "-U", ZEROS, "-A", ZEROS, sam], env=env)[1] == everything
        assert _cli(base + [sam], env=env)[1] == want
    # without -G nothing is annotated, without -g nothing has a motif; -o writes the file
    assert _cli(["-g", fa, sam])[1] == st.expected_stdout(text, seqs)
    assert _cli(["-G", gtf, sam])[1] == st.expected_stdout(text, None, introns)
    o = str(tmp_path / "out.tab")
    rc, out, err = _cli(base + ["-o", o, sam])
    assert rc == 0 and out == b"" and open(o, "rb").read() == want
    # nothing survives: an empty file and exit 0
    rc, out, err = _cli(["-a", "1000,1000,1000,1000,1000", sam])
    assert rc == 0 and out == b""
    rc, out, err = _cli([sc.write_inputs(tmp_path, "none", sc.no_junction_sam())[2]])
    assert rc == 0 and out == b""
    # the genome lacks chr2 and chr3: bam2sj's message
    one = str(tmp_path / "one.fa")
    with open(one, "w") as fh:
        fh.write(">chr1\n%s\n" % seqs[0])
    rc, out, err = _cli(["-g", one, sam])
    assert rc == 1 and out == b"" and "[intr_deri_str] unknown tid: 1" in err


def test_cli_descending_tids_are_sorted(tmp_path):
    text = sc.tids_0_1_0_sam()
    want = st.expected_stdout(text, filt=st.KEEP_ALL)
    assert want == (b"chr1\t11\t60\t0\t0\t0\t1\t0\t10\nchr1\t111\t160\t0\t0\t0\t1\t1\t10\nchr1\t311\t360\t0\t0\t0\t1\t0\t10\n"
                    b"chr2\t11\t60\t0\t0\t0\t1\t0\t10\nchr2\t511\t560\t0\t0\t0\t0\t1\t10\n")
    for path in sc.write_inputs(tmp_path, "dec", text):
        for env in (None, {"L2R_SJ_BATCH": 2}):
            rc, out, err = _cli(["-a", ZEROS, "-U", ZEROS, "-A", ZEROS, path], env=env)
            assert rc == 0 and out == want, path
            assert "host" not in err


def test_cli_usage(tmp_path):
    sam = sc.write_inputs(tmp_path, "none", sc.no_junction_sam())[0]
    for args in (["-a", "1,2,3", sam], ["-U", "1,2,3,4,5,6", sam], ["-A", "0:0:0:0:0", sam], [], [sam, sam], ["-x", sam]):
        rc, out, err = _cli(args)
        assert rc == 1 and out == b"" and "Usage:" in err and "sjtab" in err, args
    rc, out, err = _cli(["-g", str(tmp_path / "missing.fa"), sam])
    assert rc == 1 and out == b"" and "Can not open genome file" in err
    p = hostlib.run_cli([])
    assert p.returncode == 1 and b"sjtab" in p.stderr and b"bam2sj" in p.stderr


def test_cli_output_feeds_update_gtf(tmp_path):
    """Closing the loop: the file `sjtab` writes is the -j file of update-gtf; a file the restatement writes gives the same outputs."""
    anno = synth.make_annotation(8000, 7)
    af = anno.in_file_order()
    reads = synth.make_reads(anno, 5000, 5, 7)
    sam, gtf, short = str(tmp_path / "reads.sam"), str(tmp_path / "anno.gtf"), str(tmp_path / "short.sam")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    # the short reads: the long reads' own alignments as properly paired records, every third one multi-mapped
    lines = ["@HD\tVN:1.6\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (c, reads.chrom_len) for c in reads.chrom_names]
    for i in range(reads.n):
        lines.append(sc.sam_line("s%d" % i, 3, reads.chrom_names[int(reads.tid[i])], int(reads.pos[i]) + 1, reads.cigar_string(i),
                                 ["NH:i:1"] if i % 3 else ["NH:i:4"]))
    text = "".join(lines)
    with open(short, "w") as fh:
        fh.write(text)
    introns = st.annotation_introns(af.tx_tid, af.tx_ex_off, af.ex_start, af.ex_end)
    want = st.expected_stdout(text, None, introns)
    tabs = [str(tmp_path / "cli.tab"), str(tmp_path / "restated.tab")]
    rc, out, err = _cli(["-G", gtf, "-o", tabs[0], short])
    assert rc == 0, err
    with open(tabs[1], "wb") as fh:
        fh.write(want)
    assert open(tabs[0], "rb").read() == want and 1000 < want.count(b"\n")
    kept_anno = sum(1 for l in want.decode().splitlines() if l.split("\t")[5] == "1")
    assert 0 < kept_anno < want.count(b"\n")
    outs = []
    for k, tab in enumerate(tabs):
        o = {n: str(tmp_path / ("%d.%s" % (k, n))) for n in ("updated.gtf", "detail.txt", "novel_exon.bed", "summary.txt")}
        p = hostlib.run_cli(["update-gtf", "-l", "3", "-J", "1", "-j", tab, "-A", o["detail.txt"], "-E", o["novel_exon.bed"], "-y", o["summary.txt"],
                             "-o", o["updated.gtf"], sam, gtf])
        assert p.returncode == 0, p.stderr.decode()
        outs.append({n: open(path, "rb").read() for n, path in o.items()})
    for n in outs[0]:
        assert outs[0][n] == outs[1][n] and len(outs[0][n]) > 0, n
    # what the table decided, read back from the command's file
    cols = [[], [], [], [], []]
    for l in open(tabs[0]).read().splitlines():
        f = l.split("\t")
        for c, v in zip(cols, (reads.chrom_names.index(f[0]), f[1], f[2], f[6], f[7])):
            c.append(int(v))
    e = capi.Engine(0)
    try:
        e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        e.set_junctions(tuple(np.array(c, np.int32) for c in cols))
        res = e.classify(reads, capi.default_params(full_level=3, min_sj_cnt=1))
    finally:
        e.close()
    checked = (res.info & capi.INFO_SJ_CHECKED) != 0
    passed = (res.info & capi.INFO_SJ_PASS) != 0
    assert checked.sum() >= 100 and 0 < passed.sum() < checked.sum()
