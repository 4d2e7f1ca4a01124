"""k_tile runs as two instances (l2r_tile.hip.h): the EXACT instance takes the tiles k_describe_scan<true> marks for it whole
(tile_exact_direct, l2r_slab.hip.h: exact under -e / -i / -t, a window of at most 32 members, every exon fits the staged positions, no
dictionary key in several entries), the general instance runs over the rest list beside it.  L2R_TILE_SPLIT=0 sends every tile to the
general instance.  Split on, split off and the oracle must agree bit for bit, and l2r_debug_counters' words 27 / 28 must say that
each instance took the tiles the upload's op statistics predict.

Who may wait for whom decides how a run splits (l2r_engine.hip, split_mode).  With inexact tiles in the run the FIRST run of an upload
only makes the rest list and the general instance takes every tile in tile order; from the second run on -- the list is known to be
short -- the EXACT instance takes its tiles and the general instance runs over the list in front of it.  Every case therefore runs
the upload twice and checks both runs.  A run without any inexact tile splits from its first run on.

The workload is a seeded `synth` case whose CIGARs are chains of M and N.  -i and -e are tuned against it on the CPU, with the arithmetic
of tile_exact over a model of the upload's tile cut, so that a handful of tiles -- fewer than the engine's rule "more than 2 % of the tiles
(+ 16) inexact -> slab pipeline" allows -- hold an N shorter than -i or an inner exon shorter than -e, some of them in front of exact
tiles: those publish their exon counts late, from the general instance, and the exact tiles behind them find their first result slots
through the second look at the counts in front.  The pipeline is not forced: the engine has to choose the tile path itself."""
import ctypes as C

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import util
from tests.upload_plan_restatement import TILE_POS_CAP, _tile_firsts, _tile_stats      # the model of the upload's tile cut

SEED = 8008
N_READS = 16000
MAX_DELET = 50
MIN_EXACT, MIN_INEXACT, MAX_INEXACT = 20, 4, 12


def _exact(stats, min_exon, min_intron):
    _, min_n, max_d, min_seg, _ = stats
    return (min_n >= min_intron) & (max_d <= MAX_DELET) & (min_seg >= min_exon)        # tile_exact, l2r_slab.hip.h


def _tune(stats):
    """(-e, -i) that leave MIN_INEXACT .. MAX_INEXACT tiles inexact, at least one by each of the two thresholds."""
    _, min_n, _, min_seg, _ = stats
    for i in sorted(set(int(v) + 1 for v in min_n))[:40]:
        for e in sorted(set(int(v) + 1 for v in min_seg))[:40]:
            by_i, by_e = min_n < i, min_seg < e
            if by_i.any() and (by_e & ~by_i).any() and MIN_INEXACT <= int((by_i | by_e).sum()) <= MAX_INEXACT:
                return e, i
    raise AssertionError("no -e / -i leaves %d .. %d inexact tiles" % (MIN_INEXACT, MAX_INEXACT))


@pytest.fixture(scope="module")
def case():
    _, af, reads = util.make_case(SEED, n_reads=N_READS, n_exons=5, anno_exons=4000, nchr=2)
    firsts = _tile_firsts(reads)
    stats = _tile_stats(reads, firsts)
    min_exon, min_intron = _tune(stats)
    exact = _exact(stats, min_exon, min_intron)
    # ---- what the test rests on, from the same arithmetic the engine uses
    n_tiles = len(firsts) - 1
    n_inexact = int((~exact).sum())
    assert exact.sum() >= MIN_EXACT and MIN_INEXACT <= n_inexact <= MAX_INEXACT
    assert n_inexact * 50 <= n_tiles + 800                      # (choose_pipeline's rule keeps the tile path)
    assert min_exon >= 1 and min_intron >= 1
    n_act = np.diff(firsts)
    assert (n_act + stats[0] <= TILE_POS_CAP).all() and (stats[4] + 1 < 255).all()       # no tile too large, no read of 255 exons
    # an inexact tile in FRONT of exact ones on the same launch: the first exact tile behind the first inexact one
    first_inexact = int(np.nonzero(~exact)[0][0])
    behind = np.nonzero(exact & (np.arange(n_tiles) > first_inexact))[0]
    assert len(behind) >= MIN_EXACT // 2
    # ... and both kinds of borderline operation change what a read's exons are (else the thresholds would test nothing)
    s = synth.cigar_summary(reads.cig_off, reads.cig).astype(np.int64)
    assert ((s[:, 1] >> 16) < min_intron).any() and (((s[:, 2] >> 16) < min_exon) & ((s[:, 1] >> 16) >= min_intron)).any()
    return dict(af=af, reads=reads, firsts=firsts, exact=exact, min_exon=min_exon, min_intron=min_intron, behind=behind, oracle={}, sj=None)


def _engine(split):
    import os
    old = {k: os.environ.get(k) for k in ("L2R_TILE_SPLIT", "L2R_PIPELINE", "L2R_ABLATE")}
    for k in old:
        os.environ.pop(k, None)
    if not split:
        os.environ["L2R_TILE_SPLIT"] = "0"
    try:
        e = capi.Engine(0)                                       # (l2r_create reads the switches)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return e


@pytest.fixture(scope="module")
def engines(case):
    af = case["af"]
    on, off = _engine(True), _engine(False)
    for e in (on, off):
        e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    yield on, off
    on.close(); off.close()


def _params(po, case, level, dis):
    return po.default_params(full_level=level, ss_dis=dis, min_exon=case["min_exon"], min_intron=case["min_intron"], max_delet=MAX_DELET,
                             min_sj_cnt=1)


def _junctions(po, case):
    if case["sj"] is None:
        base = util.oracle_run(po, case["af"], case["reads"], _params(po, case, 3, 0))
        case["sj"] = util.junction_table(case["af"], case["reads"], base, SEED, cover=0.7)[1]
    return case["sj"]


def _want(po, case, level, dis, with_sj):
    key = (level, dis, with_sj)
    if key not in case["oracle"]:                                # one oracle run per parameter set, shared by the cases
        case["oracle"][key] = util.oracle_run(po, case["af"], case["reads"], _params(po, case, level, dis), _junctions(po, case) if with_sj else None)
    return case["oracle"][key]


def _counters(eng):
    cnt = (C.c_longlong * 29)()
    eng.lib.l2r_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert eng.lib.l2r_debug_counters(eng.ctx, cnt, 29) == 0
    return list(cnt)


def _run(eng, po, case, level, dis, with_sj, acc):
    """Two runs of one upload: [(result, accepted list, counters)] of the first (the rest list's length is not known yet) and of the
    second run (it is: the steady state), and the kernel behind the tile stage."""
    reads, op = case["reads"], _params(po, case, level, dis)
    eng.set_junctions(_junctions(po, case) if with_sj else None)
    eng.set_outputs(3 if acc else 1)
    out = [(eng.classify(reads, util.to_engine_params(capi, op)), eng.download_accepted() if acc else None, _counters(eng))]
    eng.run(); eng.sync()
    out.append((eng.download(), eng.download_accepted() if acc else None, _counters(eng)))
    return out, (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()


def _acc_rows(a):
    """(the accepted list's order depends on which tile reserves its chunk first: compared as sets of records with their exons)"""
    out = []
    for k in range(len(a.rec)):
        lo, hi = int(a.ex_off[k]), int(a.ex_off[k + 1])
        out.append((a.rec[k].tobytes(), a.ex_start[lo:hi].tobytes(), a.ex_end[lo:hi].tobytes(), a.ex_flag[lo:hi].tobytes()))
    return sorted(out)


def _same_as_oracle(got, want, acc, n_sj):
    if acc:
        util.assert_same_result(got, want, n_sj, 0)
    else:                                                        # (without the accepted list nobody owes the ACCEPTED bit)
        for f in ("ex_off", "ex_start", "ex_end", "ex_flag", "ref_tx"):
            np.testing.assert_array_equal(getattr(got, f), getattr(want, f))
        np.testing.assert_array_equal(got.info & 0x7f, want.info & 0x7f)
        np.testing.assert_array_equal(got.info >> 8, np.diff(want.ex_off).astype(np.uint32))


CASES = [(level, 0, sj, acc) for level in (1, 2, 3, 4, 5) for sj in (False, True) for acc in (False, True)] + [(3, 2, False, False), (3, 2, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("level,dis,with_sj,acc", CASES)
def test_split_on_off_and_oracle_agree(engines, case, oracle, level, dis, with_sj, acc):
    on, off = engines
    want = _want(oracle, case, level, dis, with_sj)
    n_tiles, exact = len(case["firsts"]) - 1, case["exact"]
    n_exact, n_inexact = int(exact.sum()), int((~exact).sum())
    runs_on, kernel_on = _run(on, oracle, case, level, dis, with_sj, acc)
    runs_off, kernel_off = _run(off, oracle, case, level, dis, with_sj, acc)
    print("tiles %d (model %d)  exact %d  [27] / [28] split on: first run %d / %d, second run %d / %d  off: %d / %d  look-back fallbacks %d" %
          (runs_on[0][2][3], n_tiles, n_exact, runs_on[0][2][27], runs_on[0][2][28], runs_on[1][2][27], runs_on[1][2][28],
           runs_off[1][2][27], runs_off[1][2][28], runs_on[1][2][13]))
    # the engine chose the tile path itself, and no run was done again on the slab pipeline
    assert kernel_on.startswith("k_tile") and kernel_off.startswith("k_tile"), (kernel_on, kernel_off)
    # the model's tiles are the engine's; every tile has a 32-bit-mask window and the annotation has no key in several entries: the
    # verdict then is tile_exact alone
    cnt = runs_on[0][2]
    assert cnt[3] == n_tiles and cnt[1] == 0 and cnt[4] == n_tiles and cnt[12] == 0, cnt
    # first run: the list is made, no tile is marked (inexact tiles, list length unknown); second run: each instance takes its tiles
    assert (runs_on[0][2][27], runs_on[0][2][28]) == (0, n_inexact), runs_on[0][2]
    assert (runs_on[1][2][27], runs_on[1][2][28]) == (n_exact, n_inexact), runs_on[1][2]
    n_sj = len(case["sj"][0]) if with_sj else 0
    r_first = case["firsts"][case["behind"]]
    for k in (0, 1):
        got_on, acc_on, cnt_on = runs_on[k]
        got_off, acc_off, cnt_off = runs_off[k]
        assert cnt_on[13] == 0 and cnt_off[13] == 0
        assert cnt_off[27] == 0 and cnt_off[28] == 0, cnt_off
        # bit for bit: the oracle, and the two engines against each other on everything they return
        _same_as_oracle(got_on, want, acc, n_sj)
        _same_as_oracle(got_off, want, acc, n_sj)
        for f in ("ex_off", "ex_start", "ex_end", "ex_flag", "info", "ref_tx"):
            assert np.array_equal(getattr(got_on, f), getattr(got_off, f)), (k, f)
        # the late-publish path: exact tiles behind an inexact one begin at the slots the oracle gives their first reads
        assert np.array_equal(got_on.ex_off[r_first], want.ex_off[r_first])
        if acc:
            assert len(acc_on.rec) == int(((got_on.info & 128) != 0).sum()) == len(acc_off.rec)
            assert _acc_rows(acc_on) == _acc_rows(acc_off)


@pytest.mark.gpu
def test_run_without_inexact_tiles_splits_from_its_first_run(engines, case, oracle):
    """Default thresholds: no tile of the workload is inexact, nobody waits for a count -- every tile is the EXACT instance's from the
    first run on, the rest list is empty, and the second run (which launches no general instance at all) gives the same."""
    on, _ = engines
    reads, af = case["reads"], case["af"]
    stats = _tile_stats(reads, case["firsts"])
    assert _exact(stats, 3, 3).all()
    n_tiles = len(case["firsts"]) - 1
    op = oracle.default_params(full_level=3)
    want = util.oracle_run(oracle, af, reads, op)
    on.set_junctions(None)
    on.set_outputs(1)
    got = on.classify(reads, util.to_engine_params(capi, op))
    cnt = _counters(on)
    assert (cnt[3], cnt[27], cnt[28], cnt[13]) == (n_tiles, n_tiles, 0, 0), cnt
    _same_as_oracle(got, want, False, 0)
    on.run(); on.sync()
    cnt = _counters(on)
    assert (cnt[27], cnt[28], cnt[13]) == (n_tiles, 0, 0), cnt
    _same_as_oracle(on.download(), want, False, 0)
