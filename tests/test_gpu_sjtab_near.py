"""The second filter stage of `sjtab` on the GPU (l2r_sj_filter_rows2, `sjtab -d / -m / -s`): every column of the result against the
restatement (tests/sjtab_near_restatement.py), the command byte for byte, its output given to `update-gtf -j`."""
import os
import re

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import sj_cases as sc
from tests import sj_restatement as sr
from tests import sjtab_near_restatement as nr
from tests import sjtab_restatement as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ("tid", "don", "acc", "strand", "motif", "anno", "uniq_c", "multi_c", "max_over")
MOTIF_BASES = {1: "GTAG", 2: "CTAC", 3: "GCAG", 4: "CTGC", 5: "ATAC", 6: "GTAT"}
ONE_CLASS = ((0, 5, 5, 5, 5), (0,) * 5, (0,) * 5)          # stage 1 of the shape tests: an overhang of 5 outside the annotation
DIST10 = (0, 10, 10, 10, 10)


def _cli(args, env=None):
    p = hostlib.run_cli(["sjtab"] + list(args), env=env)
    return p.returncode, p.stdout, p.stderr.decode()


def _sort_tile():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    return int(re.search(r"#define\s+L2R_SORT_TILE\s+(\d+)", text).group(1))


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def _anno_of_rows(tid, don, acc):
    """Two-exon transcripts whose intron is the given row."""
    tid = np.asarray(tid, np.int64); don = np.asarray(don, np.int64); acc = np.asarray(acc, np.int64)
    ex_start = np.stack([don - 50, acc + 1], axis=1).reshape(-1)
    ex_end = np.stack([don - 1, acc + 50], axis=1).reshape(-1)
    return tid.astype(np.int32), (2 * np.arange(len(tid) + 1)).astype(np.int64), ex_start.astype(np.int32), ex_end.astype(np.int32)


def _genome_for(tid, don, acc, motif, lens):
    """Sequences of 'A' with the four bases of every row's motif written at its ends, in row order (a later row may overwrite an
    earlier one's: the tests take the motifs from sr.motifs_numpy, whatever they come to).  -> (seq_off, bases, the sequences as text)."""
    seqs = [bytearray(b"A" * n) for n in lens]
    for t, d, a, m in zip(tid, don, acc, motif):
        if int(m):
            b = MOTIF_BASES[int(m)].encode()
            s = seqs[int(t)]
            s[int(d) - 1], s[int(d)], s[int(a) - 2], s[int(a) - 1] = b
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8), [s.decode() for s in seqs]


class Table:
    """A table for the engine and what the restatement says of it: six input columns (tid, don, acc, uniq_c, multi_c, max_over) with
    distinct keys in any order, an optional genome (seq_off, bases) and the rows to annotate."""

    def __init__(self, six, genome=None, anno_mask=None):
        six = [np.asarray(c, np.int64) for c in six]
        order = np.lexsort((six[2], six[1], six[0]))
        self.six = [c[order] for c in six]
        assert len(np.unique(np.stack(self.six[:3], axis=1), axis=0)) == len(order) or len(order) == 0
        self.genome = genome
        n = len(order)
        anno = np.zeros(n, np.int64) if anno_mask is None else np.asarray(anno_mask, np.int64)[order]
        self.anno_rows = _anno_of_rows(self.six[0][anno != 0], self.six[1][anno != 0], self.six[2][anno != 0]) if anno.any() else None
        if genome is not None and n:
            strand, motif = sr.motifs_numpy(genome[0], genome[1], self.six[0], self.six[1], self.six[2])
        else:
            strand, motif = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.nine = [self.six[0], self.six[1], self.six[2], np.asarray(strand, np.int64), np.asarray(motif, np.int64), anno, self.six[3], self.six[4], self.six[5]]

    def load(self, eng, shuffle_seed=None):
        cols = self.six
        if shuffle_seed is not None and len(cols[0]):
            p = np.random.default_rng(shuffle_seed).permutation(len(cols[0]))
            cols = [c[p] for c in cols]
        eng.sj_begin_tab(genome=self.genome)
        eng.sj_add_rows_over(*cols)
        t = eng.sj_finish()
        if self.anno_rows is not None:
            eng.sj_annotate(*self.anno_rows)
        return t

    def check(self, got, keep):
        for name, w in zip(NINE, self.nine):
            assert np.array_equal(getattr(got, name).astype(np.int64), np.asarray(w, np.int64)[keep]), name

    def run(self, eng, filt, dist_min, intron_max, shuffle_seed=None):
        """Load, filter, compare every column and the counters; -> (what the restatement says, the engine's counters)."""
        want = nr.filter2_numpy(self.nine, filt, dist_min, intron_max)
        self.load(eng, shuffle_seed)
        got = eng.sj_filter_rows2(*filt, dist_min=dist_min, intron_max=intron_max)
        self.check(got, want["keep"])
        stt = eng.sj_stats()
        n = len(self.six[0])
        assert stt["rows_dropped"] == n - int(want["keep"].sum()) and stt["rows_dropped_near"] == want["n_near"] and stt["rows_dropped_long"] == want["n_long"]
        return want, stt


@pytest.fixture(scope="module")
def random_table():
    """About 10 000 rows over four references, motifs from a genome that is written for them."""
    cols = nr.random_rows(11, 10000)
    lens = [int(cols[2].max()) + 100] * 4
    genome = _genome_for(cols[0], cols[1], cols[2], cols[4], lens)
    return Table([cols[0], cols[1], cols[2], cols[6], cols[7], cols[8]], genome[:2], cols[5])


RANDOM_FILTER = ((0, 20, 5, 5, 5), (0, 2, 1, 1, 1), (0, 2, 1, 1, 1))
RANDOM_DIST = (0, 10, 8, 5, 10)
RANDOM_INTRON_MAX = (15000, 24000)


# ---------------------------------------------------------------------------------------------------- 1: switched off

def test_switched_off_is_filter_rows(eng, random_table):
    t = random_table
    t.load(eng)
    a = eng.sj_filter_rows(*RANDOM_FILTER)
    dropped = eng.sj_stats()["rows_dropped"]
    for kw in (dict(), dict(dist_min=(0,) * 5, intron_max=())):
        t.load(eng)
        b = eng.sj_filter_rows2(*RANDOM_FILTER, **kw)
        assert all(np.array_equal(getattr(a, c), getattr(b, c)) for c in NINE) and 0 < b.tid.size < t.six[0].size
        stt = eng.sj_stats()
        assert stt["rows_dropped"] == dropped > 0 and stt["rows_dropped_near"] == 0 and stt["acc_radix_passes"] == 0 and stt["rows_dropped_long"] == 0
    t.check(b, st.keep_numpy(t.nine[5], t.nine[4], t.nine[6], t.nine[7], t.nine[8], RANDOM_FILTER))
    # a null second struct
    import ctypes as C
    t.load(eng)
    f = capi.CSjFilter(*[(C.c_int32 * 5)(*v) for v in RANDOM_FILTER])
    n = C.c_int64(0)
    assert eng.lib.l2r_sj_filter_rows2(eng.ctx, C.byref(f), None, C.byref(n)) == 0 and n.value == a.tid.size
    c = eng.sj_download_tab(n.value)
    assert all(np.array_equal(getattr(a, k), getattr(c, k)) for k in NINE)


# ---------------------------------------------------------------------------------------------------- 2: the hand table

def _hand_table(rows=nr.HAND_ROWS):
    cols = nr.columns(rows)
    lens = [700000, 2000, 2000]
    genome = _genome_for(cols[0], cols[1], cols[2], cols[4], lens)
    t = Table([cols[0], cols[1], cols[2], cols[6], cols[7], cols[8]], genome[:2], cols[5])
    assert [tuple(int(c[i]) for c in t.nine) for i in range(len(rows))] == list(rows)      # the genome gives the motifs the table names
    return t, genome[2]


def test_hand_table(eng):
    t, _ = _hand_table()
    t.load(eng)
    got = eng.sj_filter_rows2(*nr.HAND_FILTER, dist_min=nr.HAND_DIST, intron_max=nr.HAND_INTRON_MAX)
    rows = [tuple(int(getattr(got, c)[i]) for c in NINE) for i in range(got.tid.size)]
    assert rows == [r for r, s in zip(nr.HAND_ROWS, nr.HAND_STAYS) if s]
    stt = eng.sj_stats()
    assert stt["rows_dropped_long"] == nr.HAND_N_LONG and stt["rows_dropped_near"] == nr.HAND_N_NEAR and stt["rows_dropped"] == nr.HAND_STAYS.count(False)
    t.run(eng, nr.HAND_FILTER, nr.HAND_DIST, nr.HAND_INTRON_MAX, shuffle_seed=3)


# ---------------------------------------------------------------------------------------------------- 3: edges of the table

def test_edges_of_the_table(eng):
    star = dict(dist_min=nr.STAR_DIST, intron_max=nr.STAR_INTRON_MAX)
    eng.sj_begin_tab()
    eng.sj_finish()
    assert all(getattr(eng.sj_filter_rows2(**star), n).size == 0 for n in NINE)
    one = Table([[2], [10], [20], [3], [4], [40]])
    want, _ = one.run(eng, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    assert want["keep"].tolist() == [True] and want["dd"].tolist() == [nr.FAR]
    # two rows on one reference, close at one end each; the same on two references
    for acc, keep in (([500, 900], [False, False]), ([500, 505], [False, False]), ([500, 510], [True, True])):
        don = [100, 103] if acc[1] == 900 else [100, 300]
        want, _ = Table([[1, 1], don, acc, [3, 3], [0, 0], [40, 40]]).run(eng, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
        assert want["keep"].tolist() == keep
    want, stt = Table([[1, 2], [100, 100], [500, 500], [3, 3], [0, 0], [40, 40]]).run(eng, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    assert want["keep"].tolist() == [True, True] and stt["acc_radix_passes"] == 0
    # stage 1 leaves nothing
    t = Table([[0, 0, 1], [100, 103, 100], [500, 900, 500], [3, 3, 3], [0, 0, 0], [4, 4, 4]])
    want, stt = t.run(eng, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    assert not want["keep"].any() and stt["rows_dropped"] == 3 and stt["rows_dropped_near"] == 0
    # every row annotated: neighbours all, dropped none -- the intron-size rule passes them by as well
    t = Table([[0, 0, 0], [100, 103, 103], [500, 900, 80000], [1, 1, 1], [0, 0, 0], [40, 40, 40]], anno_mask=[1, 1, 1])
    want, stt = t.run(eng, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    assert want["keep"].all() and want["dd"].tolist() == [3, 0, 0]


# ---------------------------------------------------------------------------------------------------- 4: the bound itself

def test_distance_at_the_bound_in_every_category(eng):
    dist = (0, 7, 4, 5, 6)
    rows, anno, expect = [], [], []
    base = 0
    for c, motif in ((1, 0), (2, 1), (3, 3), (4, 5), (2, 2), (3, 4), (4, 6)):
        for side in ("don", "acc"):
            for d in (dist[c], dist[c] - 1):
                base += 10000
                rows.append((0, base, base + 500, motif)); anno.append(0); expect.append(d >= dist[c])
                rows.append((0, base + d, base + 2000, 0) if side == "don" else (0, base - 300, base + 500 - d, 0)); anno.append(1); expect.append(True)
    r = np.array(rows, np.int64)
    genome = _genome_for(r[:, 0], r[:, 1], r[:, 2], r[:, 3], [base + 10000])
    n = len(rows)
    t = Table([r[:, 0], r[:, 1], r[:, 2], np.full(n, 5), np.zeros(n), np.full(n, 40)], genome[:2], anno)
    target = t.nine[5] == 0
    assert sorted(t.nine[4][target].tolist()) == sorted(m for (_, _, _, m), a in zip(rows, anno) if not a)      # the targets have their motifs
    want, _ = t.run(eng, st.KEEP_ALL, dist, ())
    by_key = {(int(a), int(b)): bool(k) for a, b, k in zip(t.nine[1], t.nine[2], want["keep"])}
    assert [by_key[(row[1], row[2])] for row in rows] == expect and expect.count(False) == 14


# ---------------------------------------------------------------------------------------------------- 5: wave, workgroup and tile edges

def _sizes():
    tile = _sort_tile()
    return [63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1]


def _edge_table(n, split):
    """n rows that stage 1 leaves, 50 bases apart at both ends, the acceptor order the reverse of the donor order, and at every edge b
    (wave 64, workgroup 256, tile, two tiles) rows b - 1 and b three bases apart -- in the donor order and in the acceptor order.
    split: the reference changes at every edge instead, so the two are no neighbours and the first and the last row of a reference sit
    there; close pairs are then ten rows behind the edge.  Seven more rows that stage 1 drops sit one base beside survivors."""
    edges = [b for b in (64, 256, _sort_tile(), 2 * _sort_tile()) if b < n]
    i = np.arange(n)
    tid = np.searchsorted(np.array(edges, np.int64), i, side="right") if split else np.zeros(n, np.int64)
    step = np.full(n, 50); step[0] = 0
    pairs = [b for b in edges] + ([b + 11 for b in edges if b + 11 < n] if split else [])
    step[pairs] = 3
    don = 1000 + np.cumsum(step)
    accv = int(don[-1]) + 1000 + np.cumsum(step)                            # by rank in the acceptor order
    seg0 = np.array([0] + edges, np.int64)[tid] if split else np.zeros(n, np.int64)
    seg1 = np.array(edges + [n], np.int64)[tid] if split else np.full(n, n)
    acc = accv[seg0 + (seg1 - 1 - i)]                                       # rank inside the reference: reversed
    six = [tid, don, acc, np.full(n, 3), np.zeros(n), np.full(n, 40)]
    extra = np.linspace(0, n - 1, 7).astype(int)
    six = [np.concatenate([c, e]) for c, e in zip(six, (tid[extra], don[extra] + 1, acc[extra] + 1, np.full(7, 3), np.zeros(7), np.zeros(7)))]
    return Table(six), edges


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("k", range(10))
def test_neighbours_across_wave_workgroup_and_tile(eng, k, split):
    n = _sizes()[k]
    t, edges = _edge_table(n, split)
    want, stt = t.run(eng, ONE_CLASS, DIST10, (), shuffle_seed=k)
    assert int(want["s1"].sum()) == n and len(t.six[0]) == n + 7
    tid, don, acc = (c[want["s1"]] for c in t.nine[:3])
    rank = np.lexsort((acc, tid))
    for b in edges:
        same = tid[b - 1] == tid[b]
        assert same != split and don[b] - don[b - 1] == 3 and acc[rank[b]] - acc[rank[b - 1]] == 3 and (tid[rank[b]] == tid[rank[b - 1]]) == same
        near_d = want["dd"][[b - 1, b]] < 10
        near_a = want["da"][rank[[b - 1, b]]] < 10
        assert near_d.all() == near_a.all() == same and near_d.any() == near_a.any() == same
    kept1 = want["keep"][want["s1"]]
    assert int((~kept1).sum()) == len(set(np.flatnonzero(want["dd"] < 10)) | set(np.flatnonzero(want["da"] < 10)))
    assert int((~kept1).sum()) <= 4 * len(edges)
    if [b for b in edges if not split or b + 11 < n]:
        assert int((~kept1).sum()) >= 2
    assert stt["acc_radix_passes"] >= 1                                     # (the acceptor order is the donor order reversed)


# ---------------------------------------------------------------------------------------------------- 6: the acceptor order

def test_acceptor_order_is_another_order(eng):
    rng = np.random.default_rng(5)
    n = 3000
    tid = rng.integers(0, 3, n)
    don = rng.integers(1000, 400000, n)
    acc = don + rng.integers(30, 300000, n)                                 # three bytes of acc differ
    t = Table([tid, don, acc, np.full(n, 3), np.zeros(n), np.full(n, 40)])
    rank = np.lexsort((t.six[2], t.six[0]))
    assert (rank != np.arange(n)).mean() > 0.9 and int(t.six[2].max()) >> 16 > 0
    want, stt = t.run(eng, ONE_CLASS, (0, 150, 0, 0, 0), ())
    assert stt["acc_radix_passes"] >= 3 and 0.1 < want["keep"].mean() < 0.9
    only_acc = (want["da"] < 150) & (want["dd"] >= 150)
    assert only_acc.sum() > 100
    os.environ["L2R_SORT_FORCE"] = "1"
    try:
        want2, stt2 = t.run(eng, ONE_CLASS, (0, 150, 0, 0, 0), ())
    finally:
        del os.environ["L2R_SORT_FORCE"]
    assert stt2["acc_radix_passes"] == 8 and np.array_equal(want["keep"], want2["keep"])


def test_acceptors_in_order_run_no_pass(eng):
    n = 1000
    don = 1000 + np.cumsum(np.random.default_rng(6).integers(1, 30, n))
    t = Table([np.zeros(n), don, don + 777, np.full(n, 3), np.zeros(n), np.full(n, 40)])
    want, stt = t.run(eng, ONE_CLASS, DIST10, ())
    assert stt["acc_radix_passes"] == 0 and 0.1 < want["keep"].mean() < 0.9 and np.array_equal(want["dd"], want["da"])


# ---------------------------------------------------------------------------------------------------- 7: at size

def test_random_table(eng, random_table):
    t = random_table
    n = len(t.six[0])
    want = nr.filter2_numpy(t.nine, RANDOM_FILTER, RANDOM_DIST, RANDOM_INTRON_MAX)
    cat = nr.category_numpy(t.nine[5], t.nine[4])
    s1 = want["s1"]
    lim = np.asarray(RANDOM_DIST)[cat[s1]]
    don_only = (want["dd"] < lim) & (want["da"] >= lim)
    acc_only = (want["da"] < lim) & (want["dd"] >= lim)
    print("rows %d, stage 1 left %d, donor side only %d, acceptor side only %d, intron size %d, left %d" %
          (n, s1.sum(), don_only.sum(), acc_only.sum(), want["n_long"], want["keep"].sum()))
    assert 9000 < n <= 10000 and len(set(t.nine[0].tolist())) == 4 and np.bincount(cat, minlength=5).min() > 0
    assert don_only.sum() >= 0.10 * s1.sum() and acc_only.sum() >= 0.10 * s1.sum()
    assert want["n_long"] >= 0.05 * n and want["keep"].sum() >= 0.20 * n
    got, stt = t.run(eng, RANDOM_FILTER, RANDOM_DIST, RANDOM_INTRON_MAX, shuffle_seed=1)
    assert stt["acc_radix_passes"] >= 3
    # a second call works on what the first left
    again = eng.sj_filter_rows2(*RANDOM_FILTER, dist_min=RANDOM_DIST, intron_max=RANDOM_INTRON_MAX)
    left = [c[want["keep"]] for c in t.nine]
    want2 = nr.filter2_numpy(left, RANDOM_FILTER, RANDOM_DIST, RANDOM_INTRON_MAX)
    for name, w in zip(NINE, left):
        assert np.array_equal(getattr(again, name).astype(np.int64), w[want2["keep"]]), name


# ---------------------------------------------------------------------------------------------------- 8: records

SHORT_READS = [
    # flag, tid, pos (0-based), uniq, CIGAR
    (3, 0, 960, 1, "40M100N40M"), (3, 0, 960, 1, "40M100N40M"), (3, 0, 965, 0, "35M100N40M"),       # (0, 1001, 1100) three reads
    (3, 0, 960, 1, "40M300N40M"), (3, 0, 960, 1, "40M300N35M"), (3, 0, 970, 1, "30M300N40M"),       # (0, 1001, 1300): the same donor
    (3, 0, 2960, 1, "40M500N40M"), (3, 0, 2960, 1, "40M500N40M"), (3, 0, 2960, 0, "40M500N40M"),    # (0, 3001, 3500)
    (3, 0, 3060, 1, "40M410N40M"), (3, 0, 3060, 1, "40M410N40M"), (3, 0, 3060, 1, "40M410N40M"),    # (0, 3101, 3510): acceptor 10 away
    (3, 0, 4960, 1, "40M60000N40M"),                                                                 # 60 000 bases, one read
    (3, 1, 960, 1, "40M100N40M50N40M"), (3, 1, 960, 1, "40M100N40M50N40M"), (3, 1, 960, 0, "40M100N40M50N40M"),
]


def test_records_in_two_cuts(eng):
    cig, off = [], [0]
    for r in SHORT_READS:
        cig += [(ln << 4) | op for ln, op in sr.parse_cigar(r[4])]
        off.append(len(cig))
    r = dict(flag=np.array([x[0] for x in SHORT_READS], np.uint16), tid=np.array([x[1] for x in SHORT_READS], np.int32), pos=np.array([x[2] for x in SHORT_READS], np.int32),
             uniq=np.array([x[3] for x in SHORT_READS], np.uint8), cig_off=np.array(off, np.int64), cig=np.array(cig, np.uint32))
    six = st.table_numpy(*st.rows_numpy(r["flag"], r["tid"], r["pos"], r["uniq"], r["cig_off"], r["cig"]))
    n = len(six[0])
    nine = [six[0], six[1], six[2], np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), six[3], six[4], six[5]]
    filt = ((0, 30, 12, 12, 12), (0, 1, 1, 1, 1), (0, 1, 1, 1, 1))
    want = nr.filter2_numpy(nine, filt, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    assert n == 7 and want["keep"].tolist() == [False, False, True, True, False, True, True] and want["n_long"] == 1 and want["n_near"] == 2
    tables = []
    for cuts in ([0, len(SHORT_READS)], [0, 4, 5, len(SHORT_READS)]):
        eng.sj_begin_tab()
        for a, b in zip(cuts[:-1], cuts[1:]):
            c0, c1 = r["cig_off"][a], r["cig_off"][b]
            eng.sj_add(r["flag"][a:b], r["tid"][a:b], r["pos"][a:b], r["uniq"][a:b], r["cig_off"][a:b + 1] - c0, r["cig"][c0:c1])
        eng.sj_finish()
        got = eng.sj_filter_rows2(*filt, dist_min=nr.STAR_DIST, intron_max=nr.STAR_INTRON_MAX)
        for name, w in zip(NINE, nine):
            assert np.array_equal(getattr(got, name).astype(np.int64), w[want["keep"]]), name
        tables.append(got)
    assert all(np.array_equal(getattr(tables[0], c), getattr(tables[1], c)) for c in NINE)


# ---------------------------------------------------------------------------------------------------- 9: the command

GTF_LINE = '%s\tsynth\texon\t%d\t%d\t.\t+\t.\tgene_id "%s"; transcript_id "%s"; gene_name "%s"; transcript_name "%s";\n'
EXTRA_LINE = re.compile(r"\[sjtab\] (\d+) junctions dropped for their intron size, (\d+) for the distance to another junction")


def _hand_files(tmp_path):
    """The hand table as the command's inputs: per row uniq_c reads with NH 1 and multi_c with NH 2 (the rows without a read cannot be
    written as reads and are left out), overhang 40; the genome that gives the motifs; the annotated rows as two-exon transcripts."""
    rows = [r for r in nr.HAND_ROWS if r[6] + r[7] > 0]
    t, seqs = _hand_table(rows)
    lines = [sc.HDR]
    for k, r in enumerate(rows):
        for j in range(r[6] + r[7]):
            lines.append(sc.sam_line("r%d_%d" % (k, j), 3, sc.NAMES[r[0]], r[1] - 40, "40M%dN40M" % (r[2] - r[1] + 1), ["NH:i:1" if j < r[6] else "NH:i:2"]))
    text = "".join(lines)
    fa, gtf, sam = str(tmp_path / "g.fa"), str(tmp_path / "a.gtf"), str(tmp_path / "in.sam")
    with open(fa, "w") as fh:
        for name, s in zip(sc.NAMES, seqs):
            fh.write(">%s\n%s\n" % (name, s))
    introns = set()
    with open(gtf, "w") as fh:
        for k, r in enumerate(rows):
            if r[5]:
                introns.add(r[:3])
                for s, e in ((r[1] - 50, r[1] - 1), (r[2] + 1, r[2] + 50)):
                    fh.write(GTF_LINE % (sc.NAMES[r[0]], s, e, "G%d" % k, "T%d" % k, "g%d" % k, "t%d" % k))
    with open(sam, "w") as fh:
        fh.write(text)
    every = st.nine_columns(st.table(st.rows_of(sr.records_from_sam(text)[1])), seqs, introns, st.KEEP_ALL)
    assert every == rows
    return text, seqs, introns, fa, gtf, sam


def test_cli(tmp_path):
    text, seqs, introns, fa, gtf, sam = _hand_files(tmp_path)
    base = ["-g", fa, "-G", gtf]
    rc, plain, plain_err = _cli(base + [sam])
    assert rc == 0 and plain == st.expected_stdout(text, seqs, introns) and "junctions dropped" not in plain_err
    rc, out, err = _cli(base + ["-d", "0,0,0,0,0", sam])
    assert rc == 0 and out == plain and EXTRA_LINE.search(err).groups() == ("0", "0")
    assert err.replace(EXTRA_LINE.search(err).group(0) + "\n", "") == plain_err
    seen = set()
    for args, dist, lens in ((["-s"], nr.STAR_DIST, nr.STAR_INTRON_MAX), (["-d", "0,201,0,0,0", "-m", "60000,59999"], (0, 201, 0, 0, 0), (60000, 59999)),
                             (["-s", "-m", "70000"], nr.STAR_DIST, (70000,)), (["-m", "70000", "-s"], nr.STAR_DIST, nr.STAR_INTRON_MAX),
                             (["--star-filter", "--dist-other", "0,0,0,0,0", "--intron-max", "1,2,3,4,5,6,7,8"], (0,) * 5, (1, 2, 3, 4, 5, 6, 7, 8))):
        want, n_long, n_near = nr.expected_stdout(text, seqs, introns, st.DEFAULT_FILTER, dist, lens)
        rc, out, err = _cli(base + args + [sam])
        assert rc == 0 and out == want, args
        assert EXTRA_LINE.search(err).groups() == (str(n_long), str(n_near)), args
        assert "%d left by the filter" % want.count(b"\n") in err
        seen.add((n_long > 0, n_near > 0, want))
    assert len(seen) == 4 and {s[:2] for s in seen} >= {(True, True), (True, False)}
    want_star = nr.expected_stdout(text, seqs, introns, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)[0]
    assert b"chr1\t1000\t1300\t" in plain and b"chr1\t1000\t1300\t" not in want_star and b"chr1\t1000\t1100\t" in want_star
    for env in ({"L2R_SJ_BATCH": 1}, {"L2R_SJ_BATCH": 7}):
        assert _cli(base + ["-s", sam], env=env)[1] == want_star
    for bad in (["-m", ""], ["-m", "1,"], ["-m", "1,2,3,4,5,6,7,8,9"], ["-m", "-1"], ["-m", "1 2"], ["-d", "1,2,3"], ["-d", "0,10,0,5,x"], ["-d", "0,-1,0,0,0"]):
        rc, out, err = _cli(base + bad + [sam])
        assert rc == 1 and out == b"" and "Usage:" in err and "sjtab" in err, bad


def test_cli_output_feeds_update_gtf(tmp_path):
    """As tests/test_gpu_sjtab.py does for the plain table: the file `sjtab -s` writes is the -j file of update-gtf, and a junction that
    only a dropped row supported is not supported any more."""
    anno = synth.make_annotation(8000, 7)
    af = anno.in_file_order()
    reads = synth.make_reads(anno, 5000, 5, 7)
    sam, gtf, short = str(tmp_path / "reads.sam"), str(tmp_path / "anno.gtf"), str(tmp_path / "short.sam")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    lines = ["@HD\tVN:1.6\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (c, reads.chrom_len) for c in reads.chrom_names]
    for i in range(reads.n):
        lines.append(sc.sam_line("s%d" % i, 3, reads.chrom_names[int(reads.tid[i])], int(reads.pos[i]) + 1, reads.cigar_string(i),
                                 ["NH:i:1"] if i % 3 else ["NH:i:4"]))
    text = "".join(lines)
    with open(short, "w") as fh:
        fh.write(text)
    introns = st.annotation_introns(af.tx_tid, af.tx_ex_off, af.ex_start, af.ex_end)
    plain = st.expected_stdout(text, None, introns)
    want, n_long, n_near = nr.expected_stdout(text, None, introns, st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)
    gone = set(plain.splitlines()) - set(want.splitlines())
    assert n_near > 0 and len(gone) == n_long + n_near and all(l.split(b"\t")[5] == b"0" for l in gone)
    tabs = [str(tmp_path / "cli.tab"), str(tmp_path / "restated.tab"), str(tmp_path / "plain.tab")]
    rc, out, err = _cli(["-G", gtf, "-s", "-o", tabs[0], short])
    assert rc == 0, err
    for path, data in ((tabs[1], want), (tabs[2], plain)):
        with open(path, "wb") as fh:
            fh.write(data)
    assert open(tabs[0], "rb").read() == want
    outs = []
    for k, tab in enumerate(tabs[:2]):
        o = {n: str(tmp_path / ("%d.%s" % (k, n))) for n in ("updated.gtf", "detail.txt", "novel_exon.bed", "summary.txt")}
        p = hostlib.run_cli(["update-gtf", "-l", "3", "-J", "1", "-j", tab, "-A", o["detail.txt"], "-E", o["novel_exon.bed"], "-y", o["summary.txt"],
                             "-o", o["updated.gtf"], sam, gtf])
        assert p.returncode == 0, p.stderr.decode()
        outs.append({n: open(path, "rb").read() for n, path in o.items()})
    for n in outs[0]:
        assert outs[0][n] == outs[1][n] and len(outs[0][n]) > 0, n
    # what the two tables decide, read back from the files
    passed = []
    e = capi.Engine(0)
    try:
        e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        for tab in (tabs[2], tabs[0]):
            cols = [[], [], [], [], []]
            for l in open(tab).read().splitlines():
                f = l.split("\t")
                for c, v in zip(cols, (reads.chrom_names.index(f[0]), f[1], f[2], f[6], f[7])):
                    c.append(int(v))
            e.set_junctions(tuple(np.array(c, np.int32) for c in cols))
            res = e.classify(reads, capi.default_params(full_level=3, min_sj_cnt=1))
            passed.append(((res.info & capi.INFO_SJ_CHECKED) != 0, (res.info & capi.INFO_SJ_PASS) != 0))
    finally:
        e.close()
    print("reads checked %d, passed with the plain table %d, with the filtered one %d" % (passed[0][0].sum(), passed[0][1].sum(), passed[1][1].sum()))
    assert np.array_equal(passed[0][0], passed[1][0])
    assert not (passed[1][1] & ~passed[0][1]).any() and passed[1][1].sum() < passed[0][1].sum()


# ---------------------------------------------------------------------------------------------------- 10: errors

def test_errors_leave_the_table_usable(eng):
    t = Table([[1, 1], [100, 103], [500, 900], [3, 3], [0, 0], [40, 40]])
    t.load(eng)
    with pytest.raises(capi.L2RError, match=r"l2r_sj_filter_rows2.*n_intron_max"):
        eng.sj_filter_rows2(intron_max=(1,) * 9)
    with pytest.raises(capi.L2RError, match=r"l2r_sj_filter_rows2.*dist_min"):
        eng.sj_filter_rows2(dist_min=(0, -1, 0, 0, 0))
    with pytest.raises(capi.L2RError, match=r"l2r_sj_filter_rows2.*intron_max"):
        eng.sj_filter_rows2(intron_max=(5, -5))
    import ctypes as C
    g = capi.CSjFilter2((C.c_int32 * 5)(), -1, (C.c_int32 * 8)())
    f = capi.CSjFilter(*[(C.c_int32 * 5)(*v) for v in st.DEFAULT_FILTER])
    n = C.c_int64(0)
    assert eng.lib.l2r_sj_filter_rows2(eng.ctx, C.byref(f), C.byref(g), C.byref(n)) != 0 and b"l2r_sj_filter_rows2" in eng.lib.l2r_last_error()
    assert eng.sj_download_tab(2).tid.tolist() == [1, 1]                    # the table is what it was
    got = eng.sj_filter_rows2(dist_min=nr.STAR_DIST)
    assert got.tid.size == 0 and eng.sj_stats()["rows_dropped_near"] == 2
    # a plain table; a call in front of l2r_sj_finish
    eng.sj_begin()
    eng.sj_add_rows([1], [2], [3], [1], [0])
    with pytest.raises(capi.L2RError, match=r"l2r_sj_filter_rows2.*l2r_sj_begin_tab"):
        eng.sj_filter_rows2(dist_min=nr.STAR_DIST)
    assert eng.sj_finish().tid.tolist() == [1]
    eng.sj_begin_tab()
    eng.sj_add_rows_over([1], [2], [3], [1], [0], [5])
    with pytest.raises(capi.L2RError, match=r"l2r_sj_filter_rows2.*l2r_sj_finish comes first"):
        eng.sj_filter_rows2(dist_min=nr.STAR_DIST)
    assert eng.sj_finish().max_over.tolist() == [5]
    assert eng.sj_filter_rows2(st.KEEP_ALL[0], st.KEEP_ALL[1], st.KEEP_ALL[2], dist_min=nr.STAR_DIST).tid.tolist() == [1]
