"""GPU: `update-gtf -j` junction support at its staging, cursor and tolerance edges -- every case of tests/sj_support_cases.py on every
route that decides it, bit exact against the oracle and against the outcome the case states by hand.

The engine has four implementations of src/update_gtf.c:589-627, 698-709: k_tile's staged path (up to SJ_STAGE table rows over the dead
dictionary slices, l2r_tile.hip.h), k_tile with the table in HBM (more rows, -d < 0, -i < 1), k_validate_sj over a block's exon positions
and its per-read loop (l2r_kernels.hip.h).  Each replaces the reference's scan from a sequential cursor by a search.  The routes:

    tile            L2R_PIPELINE=tile                      k_tile, split on (EXACT and general instance)
    tile_general    L2R_PIPELINE=tile L2R_TILE_SPLIT=0     k_tile's general instance for every tile
    tile_validate   L2R_PIPELINE=tile L2R_ABLATE=1024      the tile path with every junction check left to k_validate_sj
    slab            L2R_PIPELINE=slab
    classic         L2R_PIPELINE=classic

each with split_trans 0 and 1 (I_ACCEPT differs), each upload run twice with l2r_sync in between: the second run is the learned steady
state (l2r_engine.hip, RunFacts) and must give the same result.  One engine per route for the whole module.

Nothing outside the engine tells which of k_tile's two -j paths a tile took, and k_tile gets no counter for it: family A brackets the
staging cap on both sides (SJ_STAGE - 1, SJ_STAGE, SJ_STAGE + 1 entries, counted by sj_support_cases.staged_entries the way the kernel
counts them, for spans that do not depend on how the reads are cut into tiles), so both paths run wherever the engine's arithmetic lands,
and the cases at -i 0 and -d -1 take the table-in-HBM path at any size."""
import ctypes as C
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import sj_support_cases as sc
from tests import sj_support_restatement as rs
from tests import util
from tests.test_gpu_edges import _anno, _reads

pytestmark = pytest.mark.gpu

ROUTES = {"tile": {"L2R_PIPELINE": "tile"},
          "tile_general": {"L2R_PIPELINE": "tile", "L2R_TILE_SPLIT": "0"},
          "tile_validate": {"L2R_PIPELINE": "tile", "L2R_ABLATE": "1024"},
          "slab": {"L2R_PIPELINE": "slab"},
          "classic": {"L2R_PIPELINE": "classic"}}
CLEARED = ("L2R_TILE_SPLIT", "L2R_PIPELINE", "L2R_ABLATE", "L2R_LAUNCH_ALL", "L2R_SIDE", "L2R_CHECK", "L2R_WIDE_DIRECT", "L2R_CHUNK_DIRECT",
           "L2R_TILE_ANYWAY")
CASES = sc.CASES


def _engine(env):
    old = {k: os.environ.get(k) for k in CLEARED}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return capi.Engine(0)                                    # (l2r_create reads the switches)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(route):
        if route not in made:
            made[route] = _engine(ROUTES[route])
        return made[route]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def inputs(oracle):
    """per case: annotation, reads, table columns and the oracle's result for split_trans 0 / 1 -- computed once, never changed"""
    made = {}

    def get(case):
        if case.name not in made:
            af, reads = _anno(case.txs), _reads(case.rows)
            sj = tuple(np.array([r[k] for r in case.table], np.int32) for k in range(5))
            want = {s: util.oracle_run(oracle, af, reads, oracle.default_params(split_trans=s, **case.params), sj) for s in (0, 1)}
            made[case.name] = (af, reads, sj, want)
        return made[case.name]
    return get


def _counters(eng):
    cnt = (C.c_longlong * 27)()
    eng.lib.l2r_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert eng.lib.l2r_debug_counters(eng.ctx, cnt, 27) == 0
    return list(cnt)


def _check(eng, case, want, n_sj, split):
    got = eng.download()
    util.assert_same_result(got, want, n_sj, split)
    # the accepted list == the accepted reads of the full result, in read order (as test_gpu_edges._run checks it)
    acc = eng.download_accepted()
    idx = np.nonzero((got.info & 128) != 0)[0]
    lens = (got.info[idx] >> 8).astype(np.int64)
    g = synth._ragged_gather_index(got.ex_off[idx], lens)
    np.testing.assert_array_equal(acc.read_index, idx)
    np.testing.assert_array_equal(np.diff(acc.ex_off), lens)
    np.testing.assert_array_equal(acc.ex_start, got.ex_start[g])
    np.testing.assert_array_equal(acc.ex_end, got.ex_end[g])
    np.testing.assert_array_equal(acc.ex_flag, got.ex_flag[g])
    # the outcome the case states
    for r, what in case.expect.items():
        lo, hi = int(got.ex_off[r]), int(got.ex_off[r + 1])
        unrel = [1 if f & rs.EXF_UNREL_JUNC else 0 for f in got.ex_flag[lo:hi].tolist()]
        have = rs.outcome(int(got.info[r]) & 0x70, unrel)
        assert have == (what if isinstance(what, str) else (what[0], list(what[1]))), (case.name, r, have, what)
        accepted = (int(got.info[r]) & 128) != 0
        assert accepted == (what == "pass" or (bool(split) and what != "not_checked")), (case.name, r, what)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_junction_support(engines, inputs, route, split, case):
    af, reads, sj, want = inputs(case)
    eng = engines(route)
    eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    eng.set_junctions(sj)
    eng.set_outputs(3)
    eng.set_params(capi.default_params(split_trans=split, **case.params))
    eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    for run in (0, 1):
        eng.run(); eng.sync()
        _check(eng, case, want[split], len(case.table), split)


REACH_CASES = [c for c in CASES if c.family == "F" or c.name == "E_behind_exon_64"]


@pytest.mark.parametrize("case", REACH_CASES, ids=[c.name for c in REACH_CASES])
def test_cases_reach_their_kernels(engines, inputs, case):
    """On the tile route l2r_debug_counters and l2r_stage_kernel have to say that the cases meant for one kernel are classified by it, with
    no read left to the generic kernel -- or they would test what the other families test already:
        family E (99-exon reads, junctions behind exon 64)   the tile pipeline (the short reads of the case keep the upload's tile index)
        40-isoform loci                                        tiles of the 64-bit-mask kernel: k_tile's WIDE instance
        70-isoform loci at -d 0                                tiles k_tile_chunk took from their CIGARs (their junction check: k_validate_sj)
        70-isoform loci at -d > 0                              tiles of the chunked kernels; k_tile_chunk takes none beyond -d 0
                                                               (tile_chunk_direct, l2r_slab.hip.h), they are k_probe_slab_chunked's"""
    af, reads, sj, want = inputs(case)
    eng = engines("tile")
    eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    eng.set_junctions(sj)
    eng.set_outputs(3)
    eng.set_params(capi.default_params(**case.params))
    eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    eng.run(); eng.sync()
    cnt = _counters(eng)
    kernel = (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()
    print(case.name, "kernel", kernel, "tiles", cnt[3], "64-member", cnt[12], "chunked", cnt[23], "k_tile_chunk took", cnt[26], "declined", cnt[14],
          "redo", cnt[0], "all", cnt)
    assert kernel.startswith("k_tile"), kernel
    assert cnt[0] == 0, cnt                                      # nothing for the generic kernel
    if case.name.endswith("_iso40"):
        assert cnt[12] > 0, cnt
    elif case.name.endswith("_iso70"):
        assert cnt[23] > 0, cnt
        if case.params["ss_dis"] == 0:
            assert cnt[26] > 0, cnt
