"""The timed path of the table commands (L2R_SORT_TIMING, L2R_SJ_TIMING, L2R_FUSION_TIMING): every command once untimed and once timed
on one fresh engine.  The outputs and every stats word that is no time are the same in both runs; untimed every millisecond word is 0;
timed the word of a kernel group that ran is > 0 and the word of one that did not run is 0."""
import numpy as np
import pytest

from lr2rmats_amd import capi
from tests import gtf_order_restatement as gr
from tests import sj_cases as sc
from tests import test_fusion as tf

pytestmark = pytest.mark.gpu

T = capi.header_define("L2R_SORT_TILE")
G = capi.header_define("L2R_GTF_TILE")

SORT_MS = capi.SORT_STAT_NAMES[3:7]
NAME_MS = capi.NAME_STAT_NAMES[6:11]
GTF_MS = capi.GTF_STAT_NAMES[10:16]
SJ_MS = capi.SJ_STAT_NAMES[5:15] + capi.SJ_STAT_NAMES[17:23] + capi.SJ_STAT_NAMES[25:29]
FUSION_MS = capi.FUSION_STAT_NAMES[1:5]
NINE = ("tid", "don", "acc", "strand", "motif", "anno", "uniq_c", "multi_c", "max_over")
ONE_CLASS = ((0, 5, 5, 5, 5), (0,) * 5, (0,) * 5)              # an overhang of 5 outside the annotation: stage 1 keeps every row below
DIST = (0, 150, 150, 150, 150)


@pytest.fixture
def eng():
    e = capi.Engine(0)                                          # fresh: no call has left a time behind
    yield e
    e.close()


def both(monkeypatch, var, ms, run):
    """run() -> (list of output arrays, stats dict), untimed and then with `var` set: the four assertions the two runs share.
    -> the timed stats."""
    monkeypatch.delenv(var, raising=False)
    out0, st0 = run()
    monkeypatch.setenv(var, "1")
    out1, st1 = run()
    monkeypatch.delenv(var)
    assert len(out0) == len(out1)
    for a, b in zip(out0, out1):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert set(ms) < set(st0) and st0.keys() == st1.keys()
    for k in st0:
        if k in ms:
            assert st0[k] == 0, (k, st0[k])
        else:
            assert st0[k] == st1[k], (k, st0[k], st1[k])
    return st1


def ran(st, ms, zero=()):
    for k in ms:
        assert (st[k] == 0) if k in zero else (st[k] > 0), (k, st[k])


# ---------------------------------------------------------------------------------------------------- sort

def _rows(n, seed):
    rng = np.random.default_rng(seed)
    flag = rng.choice(np.array([0, 16, 4, 20, 256, 272], np.uint16), n)
    return flag, rng.integers(0, 25, n).astype(np.int32), rng.integers(0, 1 << 28, n).astype(np.int32)


@pytest.mark.parametrize("n", [T + 1, T])
def test_sort_order(eng, monkeypatch, n):
    flag, tid, pos = _rows(n, n)
    want = np.argsort(capi.sort_keys(flag, tid, pos), kind="stable").astype(np.uint32)

    def run(rec=(flag, tid, pos)):
        return [eng.sort_order(*rec)], eng.sort_stats()

    st = both(monkeypatch, "L2R_SORT_TIMING", SORT_MS, run)
    np.testing.assert_array_equal(run()[0][0], want)
    assert st["rows"] == n and st["radix_passes"] > 0 and st["in_order"] == 0
    ran(st, SORT_MS)
    # in order: the keys kernel alone
    st = both(monkeypatch, "L2R_SORT_TIMING", SORT_MS, lambda: run((flag[want], tid[want], pos[want])))
    assert st["radix_passes"] == 0 and st["in_order"] == 1
    ran(st, SORT_MS, zero=SORT_MS[1:])


# ---------------------------------------------------------------------------------------------------- sort -n

def _names(n, seed):
    rng = np.random.default_rng(seed)
    return [b"read/%07d" % int(k) for k in rng.integers(0, n // 3 + 1, n)]


@pytest.mark.parametrize("n", [T + 1, T])
def test_name_order(eng, monkeypatch, n):
    def run(names):
        order, groups = eng.name_order(names)
        return [order, np.asarray([groups])], eng.name_stats()

    names = _names(n, n)
    st = both(monkeypatch, "L2R_SORT_TIMING", NAME_MS, lambda: run(names))
    assert st["rows"] == n and st["radix_passes"] > 0 and st["identity"] == 0 and st["route"] == 0 and 1 < st["groups"] < n
    ran(st, NAME_MS)
    # one name: every hash byte has one value, no pass
    st = both(monkeypatch, "L2R_SORT_TIMING", NAME_MS, lambda: run([b"one/name"] * n))
    assert st["radix_passes"] == 0 and st["identity"] == 1 and st["groups"] == 1
    ran(st, NAME_MS, zero=["radix passes (hist + scan + scatter)"])


# ---------------------------------------------------------------------------------------------------- sort-gtf

def _gtf_text():
    """Shuffled transcript blocks, a little more than one tile of text."""
    n_rows = 200
    while True:
        text = gr.text_of(gr.blocks_with_rows(np.random.default_rng(n_rows), n_rows))
        if len(text) > G:
            assert len(text) < G + G // 4
            return text
        n_rows += 10


def test_gtf_order(eng, monkeypatch):
    def run(text):
        return list(eng.gtf_order(text)), eng.gtf_stats()

    text = _gtf_text()
    st = both(monkeypatch, "L2R_SORT_TIMING", GTF_MS, lambda: run(text))
    assert st["bytes"] == len(text) and st["identity"] == 0 and st["route"] == 0 and st["passes_stage2"] > 0
    ran(st, GTF_MS)
    want = gr.gtf_order(text)[0]
    assert run(text)[0][2].tolist() == [r[2] for r in want]
    # in order: no key kernel, no pass, nothing to compose
    st = both(monkeypatch, "L2R_SORT_TIMING", GTF_MS, lambda: run(gr.sort_gtf(text)))
    assert st["identity"] == 1 and st["passes_stage1"] == 0 and st["passes_stage2"] == 0
    ran(st, GTF_MS, zero=["key kernels + radix passes", "k_gtf_compose"])


# ---------------------------------------------------------------------------------------------------- bam2sj

BAM2SJ_MS = capi.SJ_STAT_NAMES[5:15]


def test_bam2sj(eng, monkeypatch):
    r = sc.synth_records(8000, 3)
    off = np.arange(6, dtype=np.int64) * 400100
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, int(off[-1]))]

    def run():
        eng.sj_begin(genome=(off, bases))
        half = 4000
        c = int(r["cig_off"][half])
        eng.sj_add(r["flag"][:half], r["tid"][:half], r["pos"][:half], r["uniq"][:half], r["cig_off"][:half + 1], r["cig"][:c])
        eng.sj_add(r["flag"][half:], r["tid"][half:], r["pos"][half:], r["uniq"][half:], r["cig_off"][half:] - c, r["cig"][c:])
        t = eng.sj_finish()
        return [t.tid, t.don, t.acc, t.uniq_c, t.multi_c, t.strand, t.motif], eng.sj_stats()

    st = both(monkeypatch, "L2R_SJ_TIMING", SJ_MS, run)
    assert st["rows_made"] == st["rows_in"] > T and 0 < st["rows_out"] < st["rows_in"] and st["radix_passes"] > 0 and st["rounds"] == 1
    ran(st, SJ_MS, zero=[k for k in SJ_MS if k not in BAM2SJ_MS])

    # rows of one key, counted already: no record kernel, no pass
    def run_rows():
        n = T + 1
        eng.sj_begin()
        eng.sj_add_rows(np.full(n, 2), np.full(n, 1000), np.full(n, 2000), np.ones(n), np.arange(n) % 2)
        t = eng.sj_finish()
        return [t.tid, t.don, t.acc, t.uniq_c, t.multi_c, t.strand, t.motif], eng.sj_stats()

    st = both(monkeypatch, "L2R_SJ_TIMING", SJ_MS, run_rows)
    assert st["radix_passes"] == 0 and st["rows_in"] == T + 1 and st["rows_out"] == 1
    ran(st, SJ_MS, zero=[k for k in SJ_MS if k not in ("k_sj_hist12", "k_sj_heads + scan", "k_sj_reduce", "k_sj_motif")])


# ---------------------------------------------------------------------------------------------------- sjtab

def _anno_of_rows(tid, don, acc):
    """Two-exon transcripts whose intron is the given row."""
    tid = np.asarray(tid, np.int64); don = np.asarray(don, np.int64); acc = np.asarray(acc, np.int64)
    ex_start = np.stack([don - 50, acc + 1], axis=1).reshape(-1)
    ex_end = np.stack([don - 1, acc + 50], axis=1).reshape(-1)
    return tid.astype(np.int32), (2 * np.arange(len(tid) + 1)).astype(np.int64), ex_start.astype(np.int32), ex_end.astype(np.int32)


def _sjtab(eng, six):
    eng.sj_begin_tab()
    eng.sj_add_rows_over(*six)
    eng.sj_finish()
    eng.sj_annotate(*_anno_of_rows(*[c[::16] for c in six[:3]]))
    t = eng.sj_filter_rows2(*ONE_CLASS, dist_min=DIST)
    return [getattr(t, k) for k in NINE], eng.sj_stats()


SJTAB_ZERO = ["k_sj_count", "k_scan_u32 (counts)", "k_sj_fill"]         # rows, no records


def test_sjtab(eng, monkeypatch):
    rng = np.random.default_rng(5)
    n = T + 1
    tid = rng.integers(0, 3, n)
    don = rng.permutation(np.arange(1000, 1000 + 97 * n, 97))              # distinct keys
    acc = don + rng.integers(30, 300000, n)
    six = [tid, don, acc, np.full(n, 3), np.zeros(n), np.full(n, 40)]
    st = both(monkeypatch, "L2R_SJ_TIMING", SJ_MS, lambda: _sjtab(eng, six))
    assert st["rows_in"] == n and st["anno_introns"] == len(tid[::16]) and st["acc_radix_passes"] > 0
    assert 0 < st["rows_dropped"] == st["rows_dropped_near"] < n and st["rows_dropped_long"] == 0
    ran(st, SJ_MS, zero=SJTAB_ZERO)
    # acceptors in the donors' order: the keys kernel, no pass
    don = 1000 + np.cumsum(rng.integers(1, 300, n))
    six = [np.zeros(n), don, don + 777, np.full(n, 3), np.zeros(n), np.full(n, 40)]
    st = both(monkeypatch, "L2R_SJ_TIMING", SJ_MS, lambda: _sjtab(eng, six))
    assert st["acc_radix_passes"] == 0 and 0 < st["rows_dropped_near"] < n
    ran(st, SJ_MS, zero=SJTAB_ZERO + ["acceptor order passes"])


# ---------------------------------------------------------------------------------------------------- fusion, filter

def _reads(n=100):
    rng = np.random.default_rng(8)
    flag, pos, off, cig = tf._random_records(rng, n, 1, 12)
    tid = rng.integers(0, 3, n).astype(np.int32)
    goff = np.arange(0, n + 1, 2, dtype=np.int64)                           # pairs
    return rng, flag, tid, pos, off, cig, goff


def test_fusion(eng, monkeypatch):
    rng, flag, tid, pos, off, cig, goff = _reads()
    n = len(flag)
    score = rng.integers(0, 200, n).astype(np.int32); ed = rng.integers(0, 3, n).astype(np.int32)
    prm = capi.CFusionParams(0.1, 0.1, 0.99, 100000)

    def run():
        rs, re, fs, fe, qlen = eng.fusion_segments(flag, pos, off, cig)
        first, second = eng.fusion_select(goff, score, ed, tid, rs, re, fs, fe, qlen[::2], prm)
        return [rs, re, fs, fe, qlen, first, second], eng.fusion_stats()

    st = both(monkeypatch, "L2R_FUSION_TIMING", FUSION_MS, run)
    want = tf._segments_numpy(flag, pos, off, cig)
    for g, w in zip(run()[0][:5], want):
        np.testing.assert_array_equal(g, w)
    ran(st, FUSION_MS, zero=["k_filter_score", "k_filter_select"])


def test_filter(eng, monkeypatch):
    rng, flag, tid, pos, off, cig, goff = _reads()
    n = len(flag)
    l_qseq = tf._segments_numpy(flag & 0xffef, pos, off, cig)[4]
    nm = rng.integers(0, 20, n).astype(np.int32)
    prm = capi.CFilterParams(0.67, 0.75, 0.98, 0)
    spans = (np.array([0, 1], np.int32), np.array([1000, 5000], np.int32), np.array([900000, 70000], np.int32))

    def run():
        drop, score, intron = eng.filter_score(flag, tid, pos, l_qseq, nm, off, cig, prm, spans)
        win = eng.filter_select(goff, score, intron, prm)
        return [drop, score, intron, win], eng.fusion_stats()

    st = both(monkeypatch, "L2R_FUSION_TIMING", FUSION_MS, run)
    out = run()[0]
    assert 0 < out[0].sum() < n and (out[3] >= 0).any()
    ran(st, FUSION_MS, zero=["k_fusion_seg", "k_fusion_select"])


# ---------------------------------------------------------------------------------------------------- the sort buffers, lent

@pytest.mark.parametrize("timed", [False, True])
def test_sort_stats_outlive_the_commands_that_borrow_the_passes(eng, monkeypatch, timed):
    if timed:
        monkeypatch.setenv("L2R_SORT_TIMING", "1")
        monkeypatch.setenv("L2R_SJ_TIMING", "1")
    flag, tid, pos = _rows(T + 1, 77)
    eng.sort_order(flag, tid, pos)
    st = eng.sort_stats()
    assert st["radix_passes"] > 0
    ran(st, SORT_MS, zero=() if timed else SORT_MS)
    eng.name_order(_names(T + 1, 78))
    assert eng.name_stats()["radix_passes"] > 0 and eng.sort_stats() == st
    eng.gtf_order(_gtf_text())
    assert eng.gtf_stats()["passes_stage2"] > 0 and eng.sort_stats() == st
    rng = np.random.default_rng(79)
    n = T + 1
    don = rng.permutation(np.arange(1000, 1000 + 97 * n, 97))
    _sjtab(eng, [rng.integers(0, 3, n), don, don + rng.integers(30, 300000, n), np.full(n, 3), np.zeros(n), np.full(n, 40)])
    assert eng.sj_stats()["acc_radix_passes"] > 0 and eng.sort_stats() == st
