"""The read classes and unique counts of `update-gtf -y` on the GPU: l2r_summary_begin / _add / _finish on the device route (k_sum_class,
k_sum_place, k_sum_gather in both forms, the merge kernels of l2r_uniq.hip.h over the class-keyed concatenation, k_sum_count) against
the exact host routine behind L2R_SUMMARY_ROUTE=host on all eight counts and against tests/summary_restatement.py, over the cases of
tests/summary_cases.py; the results of a run where they lie; and the command against L2R_SUMMARY_ROUTE=off and the oracle CLI."""
import filecmp
import os
import re

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import summary_cases as sc
from tests import summary_restatement as sr
from tests import util

pytestmark = pytest.mark.gpu

CASES = sc.cases()


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def as_result(reads):
    """The arrays of a download that holds the reads."""
    tid, info, xs, xe = sr.columns(reads)
    off = np.zeros(len(tid) + 1, np.int64)
    off[1:] = np.cumsum(info >> 8)
    return tid, capi.Result(off, xs, xe, np.zeros(len(xs), np.uint8), info, np.full(len(tid), -1, np.int32))


def summary(e, reads, opts, cuts=()):
    """begin, one add per piece of the reads between the cuts, finish: (counts, stats)."""
    e.summary_begin(force_strand=opts.get("s", 0), ss_dis=opts.get("d", 0), end_dis=opts.get("D", 0x7fffffff), frac=np.float32(opts.get("f", 0.8)))
    edges = [0] + list(cuts) + [len(reads)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        tid, res = as_result(reads[lo:hi])
        e.summary_add(tid, res)
    return e.summary_finish(), e.summary_stats()


def both_routes(e, monkeypatch, reads, opts, cuts=(), name=""):
    """The device route against the host route and the restatement; returns the device's stats."""
    monkeypatch.delenv("L2R_SUMMARY_ROUTE", raising=False)
    dev, dst = summary(e, reads, opts, cuts)
    monkeypatch.setenv("L2R_SUMMARY_ROUTE", "host")
    host, hst = summary(e, reads, opts, cuts)
    monkeypatch.delenv("L2R_SUMMARY_ROUTE")
    want = sr.counts(reads, **opts)
    assert hst["route"] == 1 and host == want, (name, host, want)
    assert dev == want, (name, dev, want)
    assert dst["reads"] == len(reads) and dst["exons"] == sum(len(r[2]) for r in reads) and dst["adds"] == len(cuts) + 1, (name, dst)
    return dst


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_on_the_device_route(eng, monkeypatch, name):
    reads, opts = CASES[name]
    assert sr.in_order(reads)
    st = both_routes(eng, monkeypatch, reads, opts, name=name)
    assert st["route"] == 0
    if reads:
        assert st["clusters"] >= len({sr.klass(r[1]) for r in reads}) and 1 <= st["largest_cluster"] <= len(reads)


def test_what_the_cases_are_built_to_show(eng):
    reads, want = sc.bit_combinations()
    assert summary(eng, reads, {})[0] == [8, 2, 2, 4, 8, 2, 2, 4]
    assert summary(eng, sc.twins(0, 1), {})[0] == [1, 1, 0, 0, 1, 1, 0, 0]
    counts, st = summary(eng, sc.twins(2, 2), {})
    assert counts == [0, 0, 2, 0, 0, 0, 1, 0] and (st["clusters"], st["largest_cluster"]) == (1, 2)
    counts, st = summary(eng, sc.descends_overall(), {})
    assert st["route"] == 0 and counts == [5, 5, 0, 0, 5, 5, 0, 0] and st["clusters"] == 2      # the class boundary is a cluster boundary


@pytest.mark.parametrize("k", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("wave", [0, 1])
def test_chain_lengths_in_both_forms_of_the_gather(eng, monkeypatch, k, wave):
    monkeypatch.setenv("L2R_SUMMARY_WAVE", str(wave))
    st = both_routes(eng, monkeypatch, sc.long_chains(k), dict(f=0.5), name=(k, wave))
    assert st["route"] == 0 and st["wave_form"] == wave
    assert summary(eng, sc.long_chains(k), dict(f=0.5))[0] == [3, 2, 0, 1, 2, 1, 0, 1]


def test_the_form_of_the_gather_follows_the_exons_per_read(eng):
    assert summary(eng, sc.long_chains(200), {})[1]["wave_form"] == 1 and summary(eng, sc.long_chains(2), {})[1]["wave_form"] == 0


@pytest.mark.parametrize("n_adds", [2, 3])
def test_one_cluster_over_several_adds(eng, monkeypatch, n_adds):
    """... with an empty add between them: the count is 1, not the number of adds."""
    reads = sc.one_cluster(6 * n_adds)
    cuts = [c for k in range(1, n_adds) for c in (6 * k, 6 * k)]
    st = both_routes(eng, monkeypatch, reads, {}, cuts=cuts)
    assert st["route"] == 0 and st["adds"] == 2 * n_adds - 1 and st["clusters"] == 1
    assert summary(eng, reads, {}, cuts)[0] == [0, len(reads), 0, 0, 0, 1, 0, 0]


def test_adds_of_the_generated_set_at_odd_places(eng, monkeypatch):
    reads, opts = CASES["generated"]
    st = both_routes(eng, monkeypatch, reads, opts, cuts=[1, 257, 258, 1000])
    assert st["route"] == 0 and st["clusters"] > 100


def test_input_that_descends_inside_a_class_takes_the_host_routine(eng):
    reads = sc.descends_in_a_class()
    counts, st = summary(eng, reads, {})
    assert st["route"] == 1 and counts == sr.counts(reads) == [6, 5, 0, 0, 5, 5, 0, 0]
    reads, opts = CASES["generated"]
    swapped = reads[300:] + reads[:300]
    counts, st = summary(eng, swapped, opts)
    assert st["route"] == 1 and counts == sr.counts(swapped, **opts)


@pytest.mark.parametrize("name", sorted(k for k, v in sc.edge_cases().items() if v[1] is not None))
@pytest.mark.parametrize("route", ["device", "host"])
def test_the_checks_at_their_edges(eng, monkeypatch, name, route):
    reads, refusal = sc.edge_cases()[name]
    if route == "host":
        monkeypatch.setenv("L2R_SUMMARY_ROUTE", "host")
    with pytest.raises(capi.L2RError) as err:
        summary(eng, reads, {})
    assert "rc=-1:" in str(err.value) and refusal in str(err.value)
    monkeypatch.delenv("L2R_SUMMARY_ROUTE", raising=False)
    assert summary(eng, sc.twins(0, 0), {})[0] == [2, 0, 0, 0, 1, 0, 0, 0]          # the unit works on behind a refusal


def test_order_of_calls_and_arrays_that_do_not_fit():
    e = capi.Engine(0)
    tid, res = as_result(sc.twins(0, 1))
    with pytest.raises(capi.L2RError) as err:
        e.summary_add(tid, res)
    assert "no l2r_summary_begin in front" in str(err.value)
    e.summary_begin()
    with pytest.raises(capi.L2RError) as err:               # res == NULL without a run
        e.summary_add(tid)
    assert "no completed run" in str(err.value)
    bad = capi.Result(res.ex_off + np.asarray([0, 1, 0]), res.ex_start, res.ex_end, res.ex_flag, res.info, res.ref_tx)
    with pytest.raises(capi.L2RError) as err:
        e.summary_add(tid, bad)
    assert "rc=-1:" in str(err.value) and "not the running sum" in str(err.value)
    e.summary_add(tid, res)                                 # the refused adds have left nothing behind
    assert e.summary_finish() == [1, 1, 0, 0, 1, 1, 0, 0] and e.summary_stats()["adds"] == 1
    e.close()


# ---------------------------------------------------------------------------------------------------- the results of a run where they lie

SEED = 61           # (the set of tests/test_gpu_read_lists.py)


@pytest.fixture(scope="module")
def run_set(oracle):
    anno = synth.make_annotation(3000, SEED, nchr=3)
    af, reads = anno.in_file_order(), synth.make_reads(anno, 700, 6, SEED)
    base = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=3))
    j, sj = util.junction_table(af, reads, base, SEED, cover=0.6)
    op = oracle.default_params(full_level=3, split_trans=1, min_sj_cnt=1)
    return anno, af, reads, j, sj, op


def test_the_results_of_a_run_where_they_lie(eng, monkeypatch, run_set):
    _anno, af, reads, _j, sj, op = run_set
    eng.set_params(util.to_engine_params(capi, op))
    eng.set_outputs(capi.WANT_RESULTS)
    eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    eng.set_junctions(sj)
    eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    eng.run()
    eng.sync()
    res = eng.download()
    as_reads = [(int(reads.tid[i]), int(res.info[i]) & 0xff, [(int(res.ex_start[k]), int(res.ex_end[k])) for k in range(int(res.ex_off[i]), int(res.ex_off[i + 1]))])
                for i in range(reads.n)]
    opts = dict(s=1, d=2, D=50, f=0.8)
    want = sr.counts(as_reads, **opts)
    assert min(want[:4]) > 0 and want[4] < want[0] and want[5] < want[1]            # every class is there, and the two large ones have hits
    got = {}
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("L2R_SUMMARY_ROUTE", "host")
        for how in ("run", "download"):
            eng.summary_begin(force_strand=1, ss_dis=2, end_dis=50, frac=0.8)
            eng.summary_add(reads.tid, None if how == "run" else res)
            got[route, how] = eng.summary_finish()
            st = eng.summary_stats()
            assert st["route"] == (route == "host") and st["reads"] == reads.n and st["exons"] == int(res.ex_off[-1])
    monkeypatch.delenv("L2R_SUMMARY_ROUTE")
    assert all(v == want for v in got.values()), (got, want)
    eng.summary_begin()
    for bad_n in (reads.n - 1, reads.n + 1):                    # n differing from the run's reads
        with pytest.raises(capi.L2RError) as err:
            eng.summary_add(reads.tid[:bad_n] if bad_n < reads.n else np.append(reads.tid, 0))
        assert "%d reads, the last run had %d" % (bad_n, reads.n) in str(err.value) and "rc=-1:" in str(err.value)


# ---------------------------------------------------------------------------------------------------- the command

HAND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand")
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy")
OUTS = ("gtf", "detail", "summary", "bed", "known", "novel", "unrec", "all")
LINE = re.compile(r"\[update_gtf\] summary classes: route (device|host|off), (\d+) reads in (\d+) adds, known (\d+) \((\d+) unique\), reliable (\d+) \((\d+) unique\), "
                  r"unreliable (\d+) \((\d+) unique\), unrecognised (\d+) \((\d+) unique\), (\d+) clusters, largest (\d+)$")


def args(o, extra, aln, gtf):
    return ["update-gtf"] + extra + ["-A", o["detail"], "-y", o["summary"], "-E", o["bed"], "-k", o["known"], "-v", o["novel"], "-u", o["unrec"], "-a", o["all"],
                                     "-o", o["gtf"], aln, gtf]


def every_way(oracle, tmp_path, extra, aln, gtf, n_reads):
    """The command with several shards on one tail thread and on four, with L2R_SUMMARY_ROUTE=host and =off, and the oracle CLI: the same
    bytes in every file; the timing line names the route."""
    shards = max(1, n_reads // 3 - 1)
    configs = {"off": dict(L2R_SUMMARY_ROUTE="off", L2R_THREADS=1), "t1": dict(L2R_THREADS=1, L2R_CHUNK_READS=shards),
               "t4": dict(L2R_THREADS=4, L2R_TAIL_PART_READS=max(1, n_reads // 5), L2R_CHUNK_READS=shards), "host": dict(L2R_SUMMARY_ROUTE="host", L2R_THREADS=4, L2R_TAIL_PART_READS=max(1, n_reads // 5))}
    route = {"off": "off", "t1": "device", "t4": "device", "host": "host"}
    d = tmp_path / "oracle"
    d.mkdir()
    want = {k: str(d / k) for k in OUTS}
    assert oracle.run_cli(args(want, extra, aln, gtf)) == 0
    for tag, env in configs.items():
        d = tmp_path / tag
        d.mkdir()
        o = {k: str(d / k) for k in OUTS}
        r = hostlib.run_cli(args(o, extra, aln, gtf), env=dict(env, L2R_TIMING=1))
        assert r.returncode == 0, (tag, r.stderr.decode()[-1500:])
        lines = [ln for ln in r.stderr.decode().splitlines() if "summary classes: route" in ln]
        assert len(lines) == 1 and LINE.match(lines[0]), (tag, lines)
        m = LINE.match(lines[0])
        assert m.group(1) == route[tag], (tag, lines[0])
        if tag != "off":
            assert int(m.group(2)) == n_reads == sum(int(m.group(g)) for g in (4, 6, 8, 10)), (tag, lines[0])
            if "L2R_CHUNK_READS" in env and n_reads >= 9:
                assert int(m.group(3)) >= 3, (tag, lines[0])
        for k in OUTS:
            assert filecmp.cmp(o[k], want[k], shallow=False), (tag, k)
    return want


@pytest.mark.parametrize("name", ["upd", "upd_c", "split", "dis2"])
def test_cli_hand_cases(oracle, tmp_path, name):
    """... upd_c with -c and dis2 with -d 2: the merge parameters that reach l2r_summary_begin."""
    from tests.test_hand_known_answers import CASES as HAND_CASES
    cmd, inp, anno, _ = HAND_CASES[name]
    n = sum(1 for ln in open(os.path.join(HAND, inp)) if not ln.startswith("@"))
    every_way(oracle, tmp_path, list(cmd)[1:], os.path.join(HAND, inp), os.path.join(HAND, anno if isinstance(anno, str) else "anno.gtf"), n)


def test_cli_toy(oracle, tmp_path):
    n = sum(1 for ln in open(os.path.join(TOY, "toy.sam")) if not ln.startswith("@"))
    every_way(oracle, tmp_path, ["-l", "3"], os.path.join(TOY, "toy.sam"), os.path.join(TOY, "original.gtf"), n)


@pytest.mark.parametrize("merge", [[], ["-c", "-d", "2", "-D", "50", "-f", "0.5"]], ids=["defaults", "c_d_D_f"])
def test_cli_synthetic_set(oracle, tmp_path, run_set, merge):
    """... with the merge parameters -c, -d, -D and -f away from their defaults as well: they reach l2r_summary_begin through the command's
    parameters, and the unique counts of summary.txt depend on them."""
    anno, _af, reads, j, _sj, _op = run_set
    sam, gtf, tab = str(tmp_path / "r.sam"), str(tmp_path / "a.gtf"), str(tmp_path / "sj.tab")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    j.write(tab)
    want = every_way(oracle, tmp_path, ["-s", "-l", "3", "-J", "1", "-j", tab] + merge, sam, gtf, reads.n)
    text = open(want["summary"]).read()
    assert all(int(re.search(r"^%s\t(\d+)$" % k, text, re.M).group(1)) > 0 for k in ("Uniq_Known_Transcripts_from_BAM", "Uniq_Unrecognized_Transcript_from_BAM"))
