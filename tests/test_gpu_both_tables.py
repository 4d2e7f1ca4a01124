"""The detail table (l2r_detail_*) and the read lists (l2r_gtftext_anno / _reads / _list) on ONE context, given the same reads: each
keeps gene tables and read rows of its own (GeneTables, ReadRows of l2r_engine.hip), so neither may see what the other was given, lose
its state to the other's calls or failures, or miss a run that has gone stale.  Over results {uploaded, of a run} x route {device,
host}, against tests/detail_restatement.py and tests/read_list_restatement.py byte for byte.  About 150 reads: more than four write
tiles of 32 in either command, batches of 48."""
import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import detail_restatement as dr
from tests import read_list_cases as rc
from tests import read_list_restatement as rr
from tests.test_gpu_read_lists import first_difference, run_case

pytestmark = pytest.mark.gpu

BATCH = 48
N_READS = 150
WAYS = [(results, route) for results in ("uploaded", "run") for route in ("device", "host")]


@pytest.fixture(scope="module")
def eng():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("L2R_CHECK", "1")                     # (read when the context is made: the guards behind both texts are filled and looked at)
        e = capi.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def run_set():
    anno = synth.make_annotation(3000, 61, nchr=3)
    return anno.in_file_order(), synth.make_reads(anno, N_READS, 6, 61), synth.make_reads(anno, N_READS - 50, 6, 62)


def run_reads(e, af, reads):
    e.set_params(capi.default_params(full_level=3))
    e.set_outputs(capi.WANT_RESULTS)
    e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    e.set_junctions(None)
    e.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    e.run()
    e.sync()


@pytest.fixture
def given(eng, run_set, monkeypatch, request):
    """(case, res): the reads of one way -- made up with their results, or run on the context (res None: the results where they lie)."""
    results, route = request.param
    if route == "host":
        monkeypatch.setenv("L2R_DETAIL_ROUTE", "host")
        monkeypatch.setenv("L2R_GTX_ROUTE", "host")
    if results == "uploaded":
        case = rc.make_case(70, np.random.default_rng(7).choice([1, 2, 2, 3, 4, 6, 9, 14, 25, 70], N_READS), flags="pieces")
        res = rc.result_of(case)
    else:
        af, reads, _ = run_set
        run_reads(eng, af, reads)
        case = dict(run_case(af, reads, eng.download()), has_sj=False, split=False)     # (the run had no junction table)
        res = None
    assert len(case["tid"]) == N_READS and dr.error(case) is None
    return case, res, 1 if route == "host" else 0


def begin_both(e, case):
    e.detail_begin(case["refs"], case["anno"], case["tx_gid"], case["tx_gname"])
    e.gtftext_begin(case["refs"], case["src"], capi.GTX_READ)
    e.gtftext_anno(case["anno"], case["tx_gid"], case["tx_gname"])


def detail_rows(e, case, res, tid=None):
    return e.detail_rows(case["tid"] if tid is None else tid, case["names"], case["qname"], res)


def list_reads(e, case, res, tid=None):
    e.gtftext_reads(case["tid"] if tid is None else tid, case["names"], case["qname"], case.get("tid_name"), res, case["has_sj"], case["split"])


def same(got, want):
    assert got == want, first_difference(got, want)


def sound(e, route):
    for st in (e.detail_stats(), e.gtftext_stats()):
        assert st["route"] == route and st["guard_intact"] == 1


@pytest.mark.parametrize("given", WAYS, indirect=True)
def test_alternating_batches(eng, given):
    case, res, route = given
    begin_both(eng, case)
    assert detail_rows(eng, case, res) == len(dr.text(case))
    list_reads(eng, case, res)
    for lst in (rr.ALL, rr.NOVEL):
        m = eng.gtftext_list(lst)[0]
        assert m == len(rr.select(case, lst)) and (m > 2 * BATCH or lst != rr.ALL)
        at, text = [0, 0], [[], []]
        while at[0] < N_READS or at[1] < m:                 # one detail batch, one list batch, until both are exhausted
            if at[0] < N_READS:
                k, t = eng.detail_lines(at[0], BATCH, BATCH << 20)
                at[0] += k; text[0].append(t)
            if at[1] < m:
                k, t = eng.gtftext_lines(at[1], BATCH, BATCH << 20)
                at[1] += k; text[1].append(t)
        same(b"".join(text[0]), dr.text(case))
        same(b"".join(text[1]), rr.text(case, lst))
        assert len(text[0]) == (N_READS + BATCH - 1) // BATCH and len(text[1]) == (m + BATCH - 1) // BATCH
        sound(eng, route)


@pytest.mark.parametrize("given", WAYS, indirect=True)
def test_different_gene_tables(eng, given):
    case, res, route = given
    other = dict(case, anno=bytes(case["anno"]).swapcase())             # the same ids, other strings
    assert other["anno"] != bytes(case["anno"]) and dr.text(other) != dr.text(case)
    begin_both(eng, case)
    detail_rows(eng, case, res)
    list_reads(eng, case, res)
    m = eng.gtftext_list(rr.ALL)[0]
    want = rr.texts(case, rr.ALL)
    same(eng.detail_lines(0, BATCH)[1], b"".join(dr.texts(case)[:BATCH]))
    same(eng.gtftext_lines(0, BATCH)[1], b"".join(want[:BATCH]))
    eng.detail_begin(other["refs"], other["anno"], other["tx_gid"], other["tx_gname"])
    same(eng.gtftext_lines(BATCH, BATCH)[1], b"".join(want[BATCH:2 * BATCH]))      # the list's next batch: its own tables
    detail_rows(eng, other, res)
    same(eng.detail_all(N_READS, BATCH), dr.text(other))                 # the detail table: the new names
    same(eng.gtftext_all(m, BATCH), rr.text(case, rr.ALL))
    sound(eng, route)


@pytest.mark.parametrize("given", WAYS, indirect=True)
def test_a_domain_error_on_one_side(eng, given):
    case, res, route = given
    bad_read = 101
    bad_tid = case["tid"].copy()
    bad_tid[bad_read] = len(case["refs"])                   # one reference outside the table
    begin_both(eng, case)
    list_reads(eng, case, res)
    m = eng.gtftext_list(rr.ALL)[0]
    with pytest.raises(capi.L2RError) as err:
        detail_rows(eng, case, res, bad_tid)
    assert str(err.value) == "rc=-1: [l2r_detail_rows] read %d: a reference outside the table" % bad_read
    same(eng.gtftext_all(m, BATCH), rr.text(case, rr.ALL))  # the list composes from the state given earlier
    assert eng.gtftext_stats()["guard_intact"] == 1
    # the mirror image: the rows stand, the list fails
    detail_rows(eng, case, res)
    list_reads(eng, case, res, bad_tid)
    with pytest.raises(capi.L2RError) as err:
        eng.gtftext_list(rr.ALL)
    assert str(err.value) == "rc=-1: [l2r_gtftext_list] block %d: a reference outside the table" % bad_read
    same(eng.detail_all(N_READS, BATCH), dr.text(case))
    assert eng.detail_stats()["guard_intact"] == 1 and eng.detail_stats()["route"] == route


def test_no_rows_with_a_names_table(eng):
    """n == 0 with a names table: l2r_detail_rows has rows (none) and has waited for what it queued -- the table here is a temporary of
    the binding -- and the lists take the same reads; neither has anything to compose."""
    case = rc.make_case(70, [2, 1, 3])
    begin_both(eng, case)
    none = np.zeros(0, np.int32)
    res = capi.Result(np.zeros(1, np.int64), none, none, np.zeros(0, np.uint8), np.zeros(0, np.uint32), none)
    assert eng.detail_rows(none, bytes(case["names"]), np.zeros(0, np.uint32), res) == 0
    assert eng.detail_stats()["rows"] == 0
    eng.gtftext_reads(none, bytes(case["names"]), np.zeros(0, np.uint32), None, res, True, True)
    assert eng.gtftext_list(rr.ALL) == (0, 0, 0)
    for lines in (eng.detail_lines, eng.gtftext_lines):
        with pytest.raises(capi.L2RError) as err:
            lines(0, BATCH)
        assert "rc=-4:" in str(err.value) and " 0 of 0" in str(err.value)
    assert detail_rows(eng, case, rc.result_of(case)) == len(dr.text(case))      # ... and the next rows are composed
    same(eng.detail_all(3, BATCH), dr.text(case))


def test_a_stale_run(eng, run_set):
    af, reads, others = run_set
    run_reads(eng, af, reads)
    case = dict(run_case(af, reads, eng.download()), has_sj=False, split=False)
    begin_both(eng, case)
    detail_rows(eng, case, None)
    list_reads(eng, case, None)
    assert eng.gtftext_list(rr.ALL)[0] == N_READS
    eng.upload_reads(others.tid, others.pos, others.rev, others.cig_off, others.cig)
    with pytest.raises(capi.L2RError) as err:
        eng.detail_lines(0, BATCH)
    assert str(err.value) == "rc=-4: [l2r_detail_lines] the rows stand for a run of %d reads, the context now holds %d" % (N_READS, others.n)
    with pytest.raises(capi.L2RError) as err:
        eng.gtftext_lines(0, BATCH)
    assert str(err.value) == "rc=-4: [l2r_gtftext_lines] the reads stand for a run of %d reads, the context now holds %d" % (N_READS, others.n)
