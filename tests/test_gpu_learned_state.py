"""What a completed run of the tile path teaches the engine (l2r_engine.hip, RunFacts): l2r_sync reads the run's list counters, and the
next run of the same inputs, parameters and outputs sizes its list-driven launches by them, skips those whose list was empty, turns the
split of k_tile on, drops the generic kernel and the junction check once nothing is left for them.  Whatever is skipped, the results
must not move: an engine that launches everything always (L2R_LAUNCH_ALL=1), one without side streams (L2R_SIDE=0), one that waits for
the device at every stage (L2R_CHECK=1) and the default engine run one upload four times -- the learning run, the first run on what it
learned, two more -- and every run of every engine is bit-equal to the oracle and to the other engines.

    case A   inexact tiles (test_gpu_tile_split's seeded workload): the first run only makes the rest list (SPLIT_LIST), the later ones
             run the general instance over it in front of the EXACT one (SPLIT_ON); without and with junction table + accepted list
    case B   isoform-rich annotations: tiles on wide_list (k_tile's WIDE instance) and on chunk_list (k_tile_chunk); l2r_debug_counters
             has to say so, or the case would test nothing.  Two of them: isoforms per gene heavy-tailed (config `cfg3_gencode` scaled
             down: most tiles are the EXACT instance's, a few on each list), and 24 per gene (nearly every tile on a list: at -d 2 most
             tiles keep the slab form, and the run behind the one that showed it takes the slab pipeline)
    forgetting   l2r_set_params between runs (-d 2: k_tile_chunk takes no tile any more, they are k_probe_slab_chunked's) and a
             second upload of the same reads: a "list empty" left over from the runs before would drop reads
"""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import util
from tests.test_gpu_tile_split import _acc_rows, _counters, _junctions, _params, _same_as_oracle, _want, case  # noqa: F401  (case: fixture)

pytestmark = pytest.mark.gpu

SWITCHES = {"default": {}, "launch_all": {"L2R_LAUNCH_ALL": "1"}, "side_off": {"L2R_SIDE": "0"}, "check": {"L2R_CHECK": "1"}}
CLEARED = ("L2R_TILE_SPLIT", "L2R_PIPELINE", "L2R_ABLATE", "L2R_LAUNCH_ALL", "L2R_SIDE", "L2R_CHECK", "L2R_WIDE_DIRECT", "L2R_CHUNK_DIRECT",
           "L2R_TILE_ANYWAY")
FIELDS = ("ex_off", "ex_start", "ex_end", "ex_flag", "info", "ref_tx")
N_RUNS = 4


def _engine(env):
    old = {k: os.environ.get(k) for k in CLEARED}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        e = capi.Engine(0)                                       # (l2r_create reads the switches)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return e


def _engines(af):
    out = {}
    for name, env in SWITCHES.items():
        out[name] = _engine(env)
        out[name].set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    return out


def _close(engines):
    for e in engines.values():
        e.close()


def _kernel(eng):
    return (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()


def _runs(eng, n, acc):
    """n runs of the resident upload with l2r_sync between them: [(result, accepted list, counters, kernel of the tile stage)]"""
    out = []
    for _ in range(n):
        eng.run(); eng.sync()
        out.append((eng.download(), eng.download_accepted() if acc else None, _counters(eng), _kernel(eng)))
    return out


def _same_everywhere(runs, want, acc, n_sj):
    """runs: {engine: [(result, accepted, ...)]} -- every run of every engine against the oracle, and against the default engine's first"""
    first = runs["default"][0]
    for name, rs in runs.items():
        for k, (got, alist, _, _) in enumerate(rs):
            _same_as_oracle(got, want, acc, n_sj)
            for f in FIELDS:
                assert np.array_equal(getattr(got, f), getattr(first[0], f)), (name, k, f)
            if acc:
                assert len(alist.rec) == int(((got.info & 128) != 0).sum()), (name, k)
                assert _acc_rows(alist) == _acc_rows(first[1]), (name, k)


# ---- case A: inexact tiles

@pytest.fixture(scope="module")
def engines_a(case):  # noqa: F811
    e = _engines(case["af"])
    yield e
    _close(e)


@pytest.mark.parametrize("with_sj,acc", [(False, False), (True, True)])
def test_rest_list_is_learned_then_used(engines_a, case, oracle, with_sj, acc):  # noqa: F811
    want = _want(oracle, case, 3, 0, with_sj)
    exact = case["exact"]
    n_exact, n_inexact = int(exact.sum()), int((~exact).sum())
    prm = util.to_engine_params(capi, _params(oracle, case, 3, 0))
    reads, runs = case["reads"], {}
    for name, eng in engines_a.items():
        eng.set_junctions(_junctions(oracle, case) if with_sj else None)
        eng.set_outputs(3 if acc else 1)
        eng.set_params(prm)
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        runs[name] = _runs(eng, N_RUNS, acc)
        for k, (_, _, cnt, kernel) in enumerate(runs[name]):
            print(name, "run", k, "tiles", cnt[3], "[27] / [28]", cnt[27], cnt[28], "redo", cnt[0], "fallbacks", cnt[13])
            assert kernel.startswith("k_tile") and cnt[13] == 0, (name, k, kernel, cnt)
            # the learning run makes the rest list and marks no tile; every later run splits
            assert (cnt[27], cnt[28]) == ((0, n_inexact) if k == 0 else (n_exact, n_inexact)), (name, k, cnt)
    _same_everywhere(runs, want, acc, len(case["sj"][0]) if with_sj else 0)


# ---- case B: wide and chunked lists

B_SEED, B_READS = 5, 20000


@pytest.fixture(scope="module", params=[("lognormal", 20000), (24, 43000)], ids=["gencode_like", "24_per_gene"])
def case_b(request, oracle):
    """(24 isoforms per gene: a tile over one gene has a 32-bit-mask window, one that meets two a 64-bit-mask window -- wide_list --, one
    that meets three a window beyond 63 members -- chunk_list)"""
    tx_per_gene, anno_exons = request.param
    anno = synth.make_annotation(anno_exons, B_SEED, nchr=2, tx_per_gene=tx_per_gene, mean_tx_exons=7)
    af = anno.in_file_order()
    reads = synth.make_reads(anno, B_READS, 6, B_SEED)
    ops = {dis: oracle.default_params(full_level=3, ss_dis=dis) for dis in (0, 2)}
    return dict(af=af, reads=reads, ops=ops, want={dis: util.oracle_run(oracle, af, reads, op) for dis, op in ops.items()})


@pytest.fixture(scope="module")
def engines_b(case_b):
    e = _engines(case_b["af"])
    yield e
    _close(e)


def _upload_b(eng, case_b, dis):
    reads = case_b["reads"]
    eng.set_junctions(None)
    eng.set_outputs(3)
    eng.set_params(util.to_engine_params(capi, case_b["ops"][dis]))
    eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)


def test_wide_and_chunk_lists_are_learned_then_used(engines_b, case_b):
    runs = {}
    for name, eng in engines_b.items():
        _upload_b(eng, case_b, 0)
        runs[name] = _runs(eng, N_RUNS, True)
        for k, (_, _, cnt, kernel) in enumerate(runs[name]):
            print(name, "run", k, "tiles", cnt[3], "64-member", cnt[12], "chunked", cnt[23], "k_tile_chunk took", cnt[26], "declined", cnt[14],
                  "late", cnt[15], "redo", cnt[0])
            # the tile path throughout (a run that has shown the lists heavy would send the next one to the slab pipeline), both lists in use
            assert kernel.startswith("k_tile") and cnt[13] == 0, (name, k, kernel, cnt)
            assert cnt[12] > 0 and cnt[23] > 0 and cnt[26] > 0, (name, k, cnt)
    _same_everywhere(runs, case_b["want"][0], True, 0)


def test_new_parameters_and_a_new_upload_forget_what_was_learned(engines_b, case_b):
    """Two runs at -d 0 (k_tile_chunk takes the chunked tiles: nothing is left to k_probe_slab_chunked, which the second run skips), then
    -d 2 without a new upload: k_tile_chunk takes none of them, every one is k_probe_slab_chunked's -- two runs; then the same reads
    uploaded again, one run."""
    first, second, third = {}, {}, {}
    for name, eng in engines_b.items():
        _upload_b(eng, case_b, 0)
        first[name] = _runs(eng, 2, True)
        assert first[name][1][2][26] > 0, (name, first[name][1][2])
        eng.set_params(util.to_engine_params(capi, case_b["ops"][2]))
        second[name] = _runs(eng, 2, True)
        for k, (_, _, cnt, _) in enumerate(second[name]):
            print(name, "-d 2 run", k, "chunked", cnt[23], "k_tile_chunk took", cnt[26], "declined", cnt[14], "redo", cnt[0])
            assert cnt[23] > 0 and cnt[26] == 0, (name, k, cnt)
        _upload_b(eng, case_b, 2)
        third[name] = _runs(eng, 1, True)
    _same_everywhere(first, case_b["want"][0], True, 0)
    _same_everywhere(second, case_b["want"][2], True, 0)
    _same_everywhere(third, case_b["want"][2], True, 0)
    for f in FIELDS:
        assert np.array_equal(getattr(third["default"][0][0], f), getattr(second["default"][0][0], f)), f
