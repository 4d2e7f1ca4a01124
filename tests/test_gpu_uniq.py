"""`unique-gtf`'s merge_trans on the GPU: l2r_uniq_merge on the device route (k_uniq_heads, the prefix maximum and the cluster cut,
k_uniq_merge, k_uniq_take) against the exact host routine behind L2R_UNIQ_ROUTE=host on every output array, over the cases of
tests/uniq_cases.py, and the command against the oracle CLI."""
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
    tid, rev, ex_off, xs, xe = ur.columns(trans)
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
    assert dst["rows"] == len(trans) and dst["unique"] == len(dev["u_src"])
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
