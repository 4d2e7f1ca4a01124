"""`unique-gtf`'s merge_trans on the GPU: l2r_uniq_merge on the device route (k_uniq_heads, the prefix maximum and the cluster cut,
k_uniq_merge, k_uniq_take) against the exact host routine behind L2R_UNIQ_ROUTE=host on every output array, over the cases of
tests/uniq_cases.py -- among them reaches carried over the edges of a wave, a tile, a wave and a round of the prefix maximum, and lists
walked in several lane rounds, against their closed-form and literal answers -- and the command against the oracle CLI."""
import filecmp

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import uniq_cases as uc
from tests import uniq_restatement as ur

pytestmark = pytest.mark.gpu

ARRAYS = ("merged", "uniq_of", "u_src", "u_start", "u_end", "u_cov")
COUNTS = ("rows", "unique", "clusters", "largest_cluster", "hits_identical", "hits_contained", "hits_single", "end_extensions")
CASES = dict(uc.cases(), **uc.tile_cases())


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def merge(e, trans, opts):
    """trans: a list of transcripts, or their columns (tid, rev, ex_off, xs, xe) as a tuple."""
    tid, rev, ex_off, xs, xe = trans if isinstance(trans, tuple) else ur.columns(trans)
    out = e.uniq_merge(tid, rev, ex_off, xs, xe, force_strand=opts.get("s", 0), ss_dis=opts.get("d", 0), end_dis=opts.get("D", ur.INT_MAX),
                       frac=np.float32(opts.get("f", 0.8)))
    return out, e.uniq_stats()


def both_routes(e, monkeypatch, trans, opts, name=""):
    """The device route against the host route: every array and every count; returns the device's."""
    monkeypatch.delenv("L2R_UNIQ_ROUTE", raising=False)
    dev, dst = merge(e, trans, opts)
    monkeypatch.setenv("L2R_UNIQ_ROUTE", "host")
    host, hst = merge(e, trans, opts)
    monkeypatch.delenv("L2R_UNIQ_ROUTE")
    assert hst["route"] == 1
    for k in ARRAYS:
        assert dev[k].dtype == host[k].dtype and np.array_equal(dev[k], host[k]), (name, k, dev[k][:20], host[k][:20])
    for k in COUNTS:
        assert dst[k] == hst[k], (name, k, dst[k], hst[k])
    assert dst["rows"] == (len(trans[0]) if isinstance(trans, tuple) else len(trans)) and dst["unique"] == len(dev["u_src"])
    return dev, dst


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_on_the_device_route(eng, monkeypatch, name):
    trans, opts = CASES[name]
    assert ur.in_order(trans)
    dev, st = both_routes(eng, monkeypatch, trans, opts, name)
    assert st["route"] == 0
    assert st["clusters"] == int(ur.heads(trans).sum()) if trans else st["clusters"] == 0


def test_what_the_cases_are_built_to_show(eng):
    c = uc.cases()
    dev, st = merge(eng, *c["mutation_forward"])
    assert st["route"] == 0 and (list(dev["merged"]), list(dev["u_start"]), list(dev["u_end"]), list(dev["u_cov"])) == ([0, 1, 1, 1], [100], [1030], [4])
    assert st["end_extensions"] == 2 and st["hits_single"] == 3
    dev, st = merge(eng, *c["early_stop"])
    assert st["route"] == 0 and list(dev["merged"]) == [0, 0, 0]
    dev, st = merge(eng, *c["strand_between"])
    assert list(dev["uniq_of"]) == [0, 1, 0, 2, 3, 2]
    dev, st = merge(eng, *c["cluster_edge"])
    assert (st["clusters"], st["largest_cluster"]) == (2, 3)
    dev, st = merge(eng, *c["own_clusters"])
    assert st["clusters"] == st["unique"] == 2 * uc.TILE + 1 and st["largest_cluster"] == 1
    for k in (64, 65, 128, 129):
        trans, targets = uc.lane_round_case(k)
        dev, st = merge(eng, trans, {})
        assert st["route"] == 0 and st["clusters"] == 1 and st["unique"] == k and list(dev["uniq_of"][k:]) == targets


def test_fraction_at_the_ulp(eng, monkeypatch):
    trans, r, above, below = uc.fraction_case()
    for f, hit in ((below, 1), (r, 1), (above, 0)):
        dev, st = both_routes(eng, monkeypatch, trans, dict(f=f))
        assert st["route"] == 0 and int(dev["merged"][1]) == hit


def test_generated_set(eng, monkeypatch):
    trans = uc.generated()
    monkeypatch.setenv("L2R_UNIQ_ROUTE", "host")
    host, hst = merge(eng, trans, uc.GENERATED_OPTS)
    # the host alone: every kind of hit, an end raised, and a merged share between 20 % and 80 %
    assert min(hst["hits_identical"], hst["hits_contained"], hst["hits_single"], hst["end_extensions"]) >= 1 and 0.2 <= host["merged"].mean() <= 0.8
    dev, st = both_routes(eng, monkeypatch, trans, uc.GENERATED_OPTS)
    assert st["route"] == 0 and st["clusters"] > 100


# ---------------------------------------------------------------------------------------------------- beyond three tiles

def closed_form(eng, monkeypatch, cols, head, clusters, largest, name):
    """A case of columns in which nothing merges: the host route on every array, and the answer as it is built."""
    n = len(cols[0])
    assert np.array_equal(ur.heads_columns(cols), head), name
    dev, st = both_routes(eng, monkeypatch, cols, {}, name)
    assert st["route"] == 0, name
    assert (st["clusters"], st["largest_cluster"], st["unique"]) == (clusters, largest, n), (name, st["clusters"], st["largest_cluster"], st["unique"])
    assert not dev["merged"].any() and np.array_equal(dev["uniq_of"], np.arange(n)) and np.array_equal(dev["u_src"], np.arange(n)), name
    return st


@pytest.mark.parametrize("p, r", uc.REACH_PAIRS)
def test_reach_over_tile_wave_and_round_edges(eng, monkeypatch, p, r):
    cols = uc.reach_columns(p, r)
    closed_form(eng, monkeypatch, cols, *uc.reach_expected(p, r, len(cols[0])), name=(p, r))


@pytest.mark.parametrize("p, r", uc.REACH_ROUND_PAIRS)
def test_reach_one_cluster_across_the_round_edge(eng, monkeypatch, p, r):
    """More than 262 144 offers through one wave of k_uniq_merge, every one stopped by the newest entry in its first lane round.  The
    device time of k_uniq_merge is printed (pytest -s)."""
    monkeypatch.setenv("L2R_SORT_TIMING", "1")
    cols = uc.reach_columns(p, r)
    st = closed_form(eng, monkeypatch, cols, *uc.reach_expected(p, r, len(cols[0])), name=(p, r))
    print("reach (%d, %d): n = %d, k_uniq_merge %.1f ms, cluster cut %.2f ms" % (p, r, len(cols[0]), st["k_uniq_merge"], st["k_uniq_heads + cluster cut"]))


@pytest.mark.parametrize("long_end", uc.STEP_ENDS)
@pytest.mark.parametrize("chroms", uc.STEP_CHROMS)
@pytest.mark.parametrize("p", uc.STEP_SLOTS)
def test_chromosome_step_behind_a_long_transcript(eng, monkeypatch, p, chroms, long_end):
    """The key carried over the edge has the larger low word (the end) and the smaller high word (the chromosome)."""
    cols = uc.step_columns(p, chroms, long_end)
    n = len(cols[0])
    assert int(cols[4][2 * p + 1]) >= int(cols[3][2 * p + 2::2].max()) and n == p + 1 + uc.N_TAIL
    closed_form(eng, monkeypatch, cols, np.ones(n, np.uint8), n, 1, name=(p, chroms, long_end))


WALK = uc.walk_cases()


@pytest.mark.parametrize("name", sorted(WALK))
def test_walk_cases(eng, monkeypatch, name):
    trans, opts, (merged, uniq_of) = WALK[name]
    assert ur.in_order(trans)
    dev, st = both_routes(eng, monkeypatch, trans, opts, name)
    k = len(merged)
    assert st["route"] == 0 and (list(dev["merged"][-k:]), list(dev["uniq_of"][-k:])) == (merged, uniq_of), (name, dev["merged"][-k:], dev["uniq_of"][-k:])
    assert int(dev["merged"].sum()) == sum(merged) * (st["clusters"] if name.startswith("several") else 1)
    if name.startswith("deep_mutation"):
        j, end = uniq_of[0], trans[0][2][-1][1]
        assert (int(dev["u_end"][j]), int(dev["u_cov"][j]), st["end_extensions"], st["hits_identical"]) == (end + 750, 4, 3, 3)
        assert list(dev["u_end"][:j]) + list(dev["u_end"][j + 1:-1]) == [end] * (len(dev["u_end"]) - 2) and int(dev["u_end"][-1]) == end + 1300
    if name.startswith("several"):
        c = int(name.rsplit("_", 1)[1])
        assert (st["clusters"], st["largest_cluster"], st["unique"]) == (c, 65 + len(merged), 65 * c)
        assert np.array_equal(dev["uniq_of"].reshape(c, -1)[:, 65:] - 65 * np.arange(c)[:, None], np.tile(np.asarray(uniq_of) - 65 * (c - 1), (c, 1)))


def largest_list(cols, u_src):
    """Entries of the longest list of one cluster."""
    cluster = np.cumsum(ur.heads_columns(cols)) - 1
    return int(np.bincount(cluster[u_src]).max())


@pytest.mark.parametrize("which", ["dense", "wide"])
def test_larger_generated_sets(eng, monkeypatch, which):
    trans, cols = getattr(uc, which)()
    monkeypatch.setenv("L2R_UNIQ_ROUTE", "host")
    host, hst = merge(eng, cols, uc.GENERATED_OPTS)
    # the host alone: every kind of hit, an end raised, a merged share between 20 % and 80 %; lists of several lane rounds (dense), more
    # clusters than one round of the scan holds (wide)
    assert min(hst["hits_identical"], hst["hits_contained"], hst["hits_single"], hst["end_extensions"]) >= 1 and 0.2 <= host["merged"].mean() <= 0.8
    if which == "dense":
        assert largest_list(cols, host["u_src"]) >= 130
    else:
        assert hst["clusters"] > 16384
    dev, st = both_routes(eng, monkeypatch, cols, uc.GENERATED_OPTS, which)
    assert st["route"] == 0 and st["clusters"] == int(ur.heads_columns(cols).sum())


def test_one_context_sizes_up_and_down(monkeypatch):
    """The context's buffers grow on demand and stay: a large call, small ones, a larger one, then small ones again."""
    c = uc.cases()
    e = capi.Engine(0)
    try:
        for name, trans, opts in (("reach", uc.reach_columns(5, uc.WAVE + 1), {}), ("n1",) + c["n1"], ("lanes_129",) + c["lanes_129"],
                                  ("wide", uc.wide()[1], uc.GENERATED_OPTS), ("n0",) + c["n0"], ("cluster_edge",) + c["cluster_edge"]):
            dev, st = both_routes(e, monkeypatch, trans, opts, name)
            assert st["route"] == 0, name
            if name == "reach":
                assert (st["clusters"], st["largest_cluster"]) == uc.reach_expected(5, uc.WAVE + 1, len(trans[0]))[1:]
            if name == "cluster_edge":
                assert (st["clusters"], st["largest_cluster"]) == (2, 3)
    finally:
        e.close()


def test_unsorted_input_takes_the_host_routine(eng, monkeypatch):
    trans, opts = uc.unsorted_case()
    dev, st = both_routes(eng, monkeypatch, trans, opts)
    assert st["route"] == 1 and st["clusters"] == 0 and dev["merged"].sum() > 0
    want = ur.merge(trans, **opts)
    for k in ARRAYS:
        assert np.array_equal(dev[k], want[k]), k


def test_argument_checks(eng):
    tid, rev, ex_off, xs, xe = ur.columns([(0, 0, [(1, 5), (9, 12)]), (0, 1, [(3, 4)])])
    for text, cols in (("does not start at 0", (tid, rev, ex_off + 1, xs, xe)), ("transcript 1 has no exon", (tid, rev, np.asarray([0, 3, 3]), xs, xe)),
                       ("transcript 0: a negative coordinate", (tid, rev, ex_off, np.asarray([1, -9, 3]), xe))):
        with pytest.raises(capi.L2RError) as e:
            eng.uniq_merge(*cols)
        assert text in str(e.value)
    with pytest.raises(capi.L2RError):                              # ... and a failed call leaves no results behind
        eng._chk(eng.lib.l2r_uniq_out(eng.ctx, None, None, None, None, None, None))


# ---------------------------------------------------------------------------------------------------- the command

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("uniq")
    anno = synth.make_annotation(3000, 23, nchr=3)
    reads = synth.make_reads(anno, 3000, 5, 23)
    sam, bam = str(d / "r.sam"), str(d / "r.bam")
    reads.write_sam(sam)
    synth.write_bam(reads, bam)
    return d, sam, bam


@pytest.mark.parametrize("extra", [[], ["-I", "-s"]])
def test_cli_bam_input(oracle, tmp_path, files, extra):
    d, sam, bam = files
    want, dev, host = str(tmp_path / "o.gtf"), str(tmp_path / "d.gtf"), str(tmp_path / "h.gtf")
    assert oracle.run_cli(["unique-gtf"] + extra + [sam], stdout_path=want) == 0
    r = hostlib.run_cli(["unique-gtf"] + extra + [bam], stdout_path=dev, env={"L2R_TIMING": 1})
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    assert b"merge_trans: route device" in r.stderr
    r = hostlib.run_cli(["unique-gtf"] + extra + [bam], stdout_path=host, env={"L2R_TIMING": 1, "L2R_UNIQ_ROUTE": "host"})
    assert r.returncode == 0 and b"merge_trans: route host" in r.stderr
    assert filecmp.cmp(want, dev, shallow=False) and filecmp.cmp(want, host, shallow=False)
    import os
    assert os.path.getsize(want) > 10000


def test_cli_gtf_input(oracle, tmp_path, files):
    d, sam, bam = files
    gtf = str(tmp_path / "reads.gtf")
    assert oracle.run_cli(["bam2gtf", sam], stdout_path=gtf) == 0
    want, dev, host = str(tmp_path / "o.gtf"), str(tmp_path / "d.gtf"), str(tmp_path / "h.gtf")
    args = ["unique-gtf", "-m", "g", "-b", bam, gtf]
    assert oracle.run_cli(["unique-gtf", "-m", "g", "-b", sam, gtf], stdout_path=want) == 0
    r = hostlib.run_cli(args, stdout_path=dev, env={"L2R_TIMING": 1})
    assert r.returncode == 0 and b"merge_trans: route device" in r.stderr, r.stderr.decode()[-1000:]
    r = hostlib.run_cli(args, stdout_path=host, env={"L2R_UNIQ_ROUTE": "host"})
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    assert filecmp.cmp(want, dev, shallow=False) and filecmp.cmp(want, host, shallow=False)
