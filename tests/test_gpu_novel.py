"""The novel list of `update-gtf` on the GPU: l2r_novel_begin / _add / _finish / _lines on the device route (the selection kernels in both
forms of the chain copy, the merge kernels of l2r_uniq.hip.h over the accumulated offers, the item, order and keep kernels, the BED
text, and the updated GTF through l2r_novel_names and the GTF-text unit, against tests/gtf_text_restatement.py) against the exact host routine behind L2R_NOVEL_ROUTE=host and against tests/novel_restatement.py, on the entries, the kept
rows of all six lists in order, the counts and the text byte for byte, over the cases of tests/novel_cases.py; the refusals; and the
results of a run where they lie."""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import gtf_text_restatement as gx
from tests import novel_cases as nc
from tests import novel_restatement as nr
from tests import util

pytestmark = pytest.mark.gpu

CASES = nc.cases()
UNORDERED = nc.unordered_cases()
MERGE = {"s": "force_strand", "d": "ss_dis", "D": "end_dis", "f": "frac"}


@pytest.fixture(scope="module")
def eng():
    os.environ["L2R_CHECK"] = "1"                       # (read when the context is made: the guard behind the text is filled and looked at)
    try:
        e = capi.Engine(0)
    finally:
        del os.environ["L2R_CHECK"]
    yield e
    e.close()


def as_result(reads):
    """The arrays of a download that holds the reads."""
    tid, info, ref, xs, xe, f = nr.columns(reads)
    off = np.zeros(len(tid) + 1, np.int64)
    off[1:] = np.cumsum(info >> 8)
    return tid, capi.Result(off, xs, xe, f, info, ref)


SOURCE = b"lr2rmats"


def anno_tables(tx_gene):
    """The gene id and gene name of every annotation transcript (made of the gene's ordinal) as one table and two id columns."""
    table, ids = gx.pack_table([b"gene%d" % g for g in tx_gene] + [b"Name%d" % g for g in tx_gene])
    return table, ids[:len(tx_gene)], ids[len(tx_gene):]


def begin(e, opts, refs=nc.REFS):
    kw = {MERGE[k]: v for k, v in opts.items() if k in MERGE}
    table, gid, gname = anno_tables(list(opts["tx_gene"]))
    e.novel_begin(refs, opts["tx_gene"], opts["na_gene"], has_sj=opts.get("has_sj", 0), split=opts.get("split", 0), source=SOURCE, anno_names=table, tx_gid=gid, tx_gname=gname, **kw)


def entry_names(src, long_name=False):
    """The names table of the entries: read names and transcript ids made of the read's index (one of 254 bytes on demand)."""
    q = [b"read%d" % i for i in src]
    if long_name and q:
        q[0] = b"r" * 254
    return gx.pack_table(q + [b"tx.%d" % i for i in src])


def gtf_want(reads, want, opts, refs):
    """The updated GTF of the restatement's entries by tests/gtf_text_restatement.py: a block of form READ per entry, the source read's
    chain with the overrides start, end and cov."""
    en = want["entries"]
    src = en["src"]
    atab, gid, gname = anno_tables(list(opts["tx_gene"]))
    etab, ids = entry_names(src, opts.get("long_name", False))
    table = atab + b"NA\0" + etab
    na, base = len(atab), len(atab) + 3
    ref = [reads[i][2] for i in src]
    off = np.zeros(len(src) + 1, np.int64)
    off[1:] = np.cumsum([len(reads[i][3]) for i in src])
    case = {"form": gx.READ, "source": SOURCE, "refs": list(refs), "tid": [reads[i][0] for i in src], "rev": [1 if reads[i][1] & nr.REV else 0 for i in src], "ex_off": off.tolist(),
            "xs": [c[0] for i in src for c in reads[i][3]], "xe": [c[1] for i in src for c in reads[i][3]], "table": table,
            "gid": [na if r < 0 else gid[r] for r in ref], "tids": [base + v for v in ids[len(src):]], "gname": [na if r < 0 else gname[r] for r in ref], "tname": [base + v for v in ids[:len(src)]],
            "m": len(src), "sel": None, "start": en["start"], "end": en["end"], "cov": en["cov"]}
    return gx.text(case)


def results(e, long_name=False, **text):
    out = {"counts": e.novel_finish(), "stats": e.novel_stats()}
    en = e.novel_entries()
    out["entries"] = {k: en[k].tolist() for k in ("src", "start", "end", "cov")}
    out["rows"] = []
    for l in range(6):
        r = e.novel_rows(l)
        out["rows"].append([list(v) for v in zip(*(r[k].tolist() for k in ("tid", "a", "b", "score", "meta")))])
    out["bed"] = e.novel_text(**text)
    etab, ids = entry_names(out["entries"]["src"], long_name)
    n = len(out["entries"]["src"])
    out["gtf_sizes"] = e.novel_names(etab, ids[:n], ids[n:])
    out["gtf"] = e.novel_text(capi.NOVEL_GTF, **text)
    gst = e.gtftext_stats()
    out["stats"] = e.novel_stats()
    out["stats"]["gtf_guard"] = gst["guard_intact"]
    return out


def novel(e, reads, opts, cuts=(), refs=nc.REFS, **text):
    """begin, one add per piece of the reads between the cuts, finish, the rows and the text."""
    begin(e, opts, refs)
    edges = [0] + list(cuts) + [len(reads)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        tid, res = as_result(reads[lo:hi])
        e.novel_add(tid, res)
    return results(e, long_name=opts.get("long_name", False), **text)


def same(got, want, name):
    if "gtf" in want:
        assert got["gtf"] == want["gtf"], (name, got["gtf"][:400], want["gtf"][:400])
        assert got["gtf_sizes"] == (want["gtf"].count(b"\n"), len(want["gtf"])) and got["stats"]["gtf_guard"] == 1, (name, got["gtf_sizes"])
    assert got["entries"] == want["entries"], (name, got["entries"], want["entries"])
    for l in range(6):
        assert got["rows"][l] == want["rows"][l], (name, l, got["rows"][l][:5], want["rows"][l][:5])
    assert got["counts"] == want["counts"], (name, got["counts"], want["counts"])
    assert got["bed"] == want["bed"], (name, got["bed"][:300], want["bed"][:300])
    st = got["stats"]
    assert [int(st["items_" + k]) for k in capi.NOVEL_LIST_NAMES] == want["items"], (name, st)
    assert [int(st["kept_" + k]) for k in capi.NOVEL_LIST_NAMES] == [len(r) for r in want["rows"]], (name, st)
    assert (st["offers"], st["known_reads"], st["entries"], st["hits"], st["widened"]) == (want["offers"], want["known"], len(want["entries"]["src"]), want["hits"], want["widened"]), (name, st)
    assert st["guard_intact"] == 1, name


def three_ways(e, monkeypatch, reads, opts, cuts=(), name="", route=0, refs=nc.REFS, **text):
    """The device route, the host route and the restatement; returns the device run."""
    monkeypatch.delenv("L2R_NOVEL_ROUTE", raising=False)
    dev = novel(e, reads, opts, cuts, refs, **text)
    monkeypatch.setenv("L2R_NOVEL_ROUTE", "host")
    host = novel(e, reads, opts, cuts, refs, **text)
    monkeypatch.delenv("L2R_NOVEL_ROUTE")
    want = nr.novel(reads, ref_names=refs, **{k: v for k, v in opts.items() if k != "long_name"})
    want["gtf"] = gtf_want(reads, want, opts, refs)
    assert host["stats"]["route"] == 1
    same(host, want, (name, "host"))
    same(dev, want, (name, "device"))
    assert dev["stats"]["route"] == route, (name, dev["stats"])
    assert dev["stats"]["reads"] == len(reads) and dev["stats"]["adds"] == len(cuts) + 1, (name, dev["stats"])
    return dev


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_on_the_device_route(eng, monkeypatch, name):
    reads, opts = CASES[name]
    three_ways(eng, monkeypatch, reads, opts, name=name)


def test_what_the_cases_are_built_to_show(eng):
    """... from the rule, on the device route."""
    assert novel(eng, *CASES["one"])["bed"] == b"chr2\t99\t150\tT_exon\t1\t-\nchr2\t199\t250\tT_exon\t1\t-\n"
    w = novel(eng, *CASES["widened_end"])
    assert w["bed"] == b"chr1\t299\t450\tT_exon\t2\t+\n" and w["stats"]["hits"] == 1 and w["stats"]["widened"] == 1 and w["stats"]["route"] == 0
    assert novel(eng, *CASES["inner_then_terminal"])["bed"] == b"chr1\t299\t400\tI_exon\t3\t+\n"
    assert novel(eng, *CASES["start_zero"])["bed"].startswith(b"chr1\t-1\t50\tS_exon\t1\t+\n")
    g = novel(eng, *CASES["genes"])
    assert (g["counts"][0], g["counts"][7]) == (6, 5) and [r[:2] for r in g["rows"][nr.GENE]] == [[0, 0], [0, 1], [0, 4], [1, 0], [1, 2], [2, 0]]
    e = novel(eng, *CASES["no_offer"])
    assert e["bed"] == b"" and e["counts"] == [0, 0, 0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 200])
@pytest.mark.parametrize("wave", [0, 1])
def test_chain_lengths_in_both_forms_of_the_copy(eng, monkeypatch, k, wave):
    monkeypatch.setenv("L2R_NOVEL_WAVE", str(wave))
    dev = three_ways(eng, monkeypatch, nc.long_chains(k), dict(nc.BASE), name=(k, wave))
    assert dev["stats"]["wave_form"] == wave and dev["stats"]["hits"] == 1 and dev["stats"]["widened"] == 1
    assert ("\t%d\t" % (1000 + 100 * (k - 1) + 57)).encode() in dev["bed"]                      # the widened end of the novel last exon


def test_the_form_of_the_copy_follows_the_exons_per_offer(eng):
    assert novel(eng, nc.long_chains(200), dict(nc.BASE))["stats"]["wave_form"] == 1 and novel(eng, nc.long_chains(2), dict(nc.BASE))["stats"]["wave_form"] == 0


def test_several_adds_with_an_empty_one_and_a_cluster_over_the_cut(eng, monkeypatch):
    reads, opts = CASES["mixed_twice"]
    k = next(i for i in range(100, len(reads)) if reads[i] is reads[i - 1])                    # between an offer and its repetition
    dev = three_ways(eng, monkeypatch, reads, opts, cuts=[1, k, k, k + 130])
    assert dev["stats"]["adds"] == 5 and dev["stats"]["hits"] > 0


@pytest.mark.parametrize("name", sorted(UNORDERED))
def test_input_that_is_not_in_order_takes_the_host_routine(eng, monkeypatch, name):
    reads, opts = UNORDERED[name]
    dev = three_ways(eng, monkeypatch, reads, opts, name=name, route=1)
    # (the only cases in which an entry's start differs from its source's: on ordered input a hit never lowers a start, so the device's
    #  k_nov_emit takes u_start for exon 0 with equal values only; its use of u_end is what test_chain_lengths... and widened_end pin)
    if name == "widened_start":
        assert dev["bed"] == b"chr1\t89\t200\tT_exon\t2\t+\n" and dev["stats"]["widened"] == 1


@pytest.mark.parametrize("how", [dict(max_rows=1), dict(max_bytes=3), dict(max_rows=7, max_bytes=200)])
def test_batches_are_the_uncut_text(eng, monkeypatch, how):
    reads, opts = CASES["mixed_257"]
    whole = nr.novel(reads, ref_names=nc.REFS, **opts)["bed"]
    assert whole.count(b"\n") > 40
    whole_gtf = gtf_want(reads, nr.novel(reads, **opts), opts, nc.REFS)
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("L2R_NOVEL_ROUTE", "host")
        got = novel(eng, reads, opts, **how)
        assert got["bed"] == whole and got["gtf"] == whole_gtf, (route, how)
    monkeypatch.delenv("L2R_NOVEL_ROUTE")


def test_a_reference_name_and_a_read_name_of_254_bytes(eng, monkeypatch):
    refs = [b"c" * 254, b"chr2", b"chrX"]
    reads, opts = CASES["mixed_65"]
    dev = three_ways(eng, monkeypatch, reads, dict(opts, long_name=True), refs=refs)
    assert dev["bed"].startswith(b"c" * 254 + b"\t") and dev["stats"]["guard_intact"] == 1
    assert b'transcript_name "' + b"r" * 254 + b'";' in dev["gtf"]


def test_a_read_name_of_255_bytes_is_refused(eng):
    reads, opts = CASES["widened_end"]
    begin(eng, opts)
    eng.novel_add(*as_result(reads))
    eng.novel_finish()
    with pytest.raises(capi.L2RError) as err:
        eng.novel_names(b"r" * 255 + b"\0", [0])
    assert "rc=-1:" in str(err.value) and "a name of 255 or more bytes" in str(err.value)
    with pytest.raises(capi.L2RError) as err:
        eng.novel_lines(capi.NOVEL_GTF)
    assert "rc=-4:" in str(err.value)


def test_what_the_updated_gtf_shows(eng):
    """... from the rule: the widened end in the transcript line and in the last exon line, the coverage, NA where ref < 0."""
    got = novel(eng, *CASES["widened_end"])["gtf"]
    attr = b'gene_id "gene0"; transcript_id "tx.0"; gene_name "Name0"; transcript_name "read0";'
    assert got == (b"chr1\tlr2rmats\ttranscript\t100\t450\t.\t+\t.\t" + attr + b' transcript_cov "2";\n' +
                   b"chr1\tlr2rmats\texon\t100\t200\t.\t+\t.\t" + attr + b"\nchr1\tlr2rmats\texon\t300\t450\t.\t+\t.\t" + attr + b"\n")
    assert novel(eng, *CASES["single_exon_hit"])["gtf"].startswith(b'chr1\tlr2rmats\ttranscript\t100\t210\t.\t+\t.\tgene_id "NA"; transcript_id "tx.0"; gene_name "NA";')


def test_split_route_reads_are_refused_and_the_unit_works_on(eng, monkeypatch):
    reads = nc.bit_combinations()
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("L2R_NOVEL_ROUTE", "host")
        begin(eng, dict(nc.BASE, has_sj=1, split=1))
        eng.novel_add(*as_result(reads))
        with pytest.raises(capi.L2RError) as err:
            eng.novel_finish()
        assert "rc=-3:" in str(err.value) and "1 split-route reads" in str(err.value), route
        assert eng.novel_stats()["split_reads"] == 1
        assert novel(eng, *CASES["widened_end"])["bed"] == b"chr1\t299\t450\tT_exon\t2\t+\n"
        assert novel(eng, reads, dict(nc.BASE, has_sj=0, split=1))["stats"]["split_reads"] == 0           # -s without a table splits nothing
    monkeypatch.delenv("L2R_NOVEL_ROUTE")


@pytest.mark.parametrize("name", sorted(nc.edge_cases()))
@pytest.mark.parametrize("route", ["device", "host"])
def test_the_checks_at_their_edges(eng, monkeypatch, name, route):
    reads, opts, refusal = nc.edge_cases()[name]
    if route == "host":
        monkeypatch.setenv("L2R_NOVEL_ROUTE", "host")
    if refusal is None:
        same(novel(eng, reads, opts), nr.novel(reads, ref_names=nc.REFS, **opts), name)
    else:
        with pytest.raises(capi.L2RError) as err:
            novel(eng, [CASES["one"][0][0]] * 3 + reads, opts, cuts=[3])                # (three reads in an add in front: the index is global)
        bad = refusal.replace("read %d:" % int(refusal.split()[1][:-1]), "read %d:" % (int(refusal.split()[1][:-1]) + 3))
        assert "rc=-1:" in str(err.value) and bad in str(err.value), (name, str(err.value))
    monkeypatch.delenv("L2R_NOVEL_ROUTE", raising=False)
    assert novel(eng, *CASES["widened_end"])["counts"] == [1, 1, 0, 1, 0, 0, 0, 0]          # the unit works on behind a refusal


def test_order_of_calls_and_arrays_that_do_not_fit():
    e = capi.Engine(0)
    tid, res = as_result(nc.widened_end())
    with pytest.raises(capi.L2RError) as err:
        e.novel_add(tid, res)
    assert "no l2r_novel_begin in front" in str(err.value)
    with pytest.raises(capi.L2RError) as err:
        e.novel_finish()
    assert "no l2r_novel_begin in front" in str(err.value)
    begin(e, nc.BASE)
    with pytest.raises(capi.L2RError) as err:               # res == NULL without a run
        e.novel_add(tid)
    assert "no completed run" in str(err.value)
    bad = capi.Result(res.ex_off + np.asarray([0, 1, 0]), res.ex_start, res.ex_end, res.ex_flag, res.info, res.ref_tx)
    with pytest.raises(capi.L2RError) as err:
        e.novel_add(tid, bad)
    assert "rc=-1:" in str(err.value) and "not the running sum" in str(err.value)
    with pytest.raises(capi.L2RError) as err:               # no finish yet
        e.novel_lines()
    assert "rc=-4:" in str(err.value)
    e.novel_add(tid, res)                                   # the refused adds have left nothing behind
    assert e.novel_finish() == [1, 1, 0, 1, 0, 0, 0, 0] and e.novel_stats()["adds"] == 1
    with pytest.raises(capi.L2RError) as err:
        e.novel_lines(capi.NOVEL_GTF)
    assert "rc=-4:" in str(err.value) and "no l2r_novel_names in front" in str(err.value)
    with pytest.raises(capi.L2RError) as err:
        e.novel_lines(first=1)
    assert "rc=-4:" in str(err.value)
    with pytest.raises(capi.L2RError) as err:               # nothing that begin checks
        e.novel_begin([], nc.TX_GENE, 4)
    assert "rc=-1:" in str(err.value) and "0 references" in str(err.value)
    e.close()


# ---------------------------------------------------------------------------------------------------- the results of a run where they lie

SEED = 61           # (the set of tests/test_gpu_summary.py, without a junction table)
FAR = 500_000_000   # beyond every read of the set


def hand_reads(tid):
    """In order behind the set on its last chromosome: an offer twice (a hit), one exon key in two entries, an item of every list, a known
    read."""
    f = nr.NE | nr.ND | nr.NA | nr.NJ
    a = [(FAR, FAR + 50, f), (FAR + 100, FAR + 150, f), (FAR + 200, FAR + 250, 0)]
    b = [(FAR + 100, FAR + 150, nr.NE), (FAR + 900, FAR + 950, 0)]
    return [(tid, nc.OFFER, 0, a), (tid, nc.OFFER, 0, a), (tid, nc.OFFER | nr.REV, -1, b), (tid, nr.KNOWN | nr.FULL, 1, [(FAR + 2000, FAR + 2050, 0)])]


def test_the_results_of_a_run_where_they_lie(oracle, monkeypatch):
    anno = synth.make_annotation(3000, SEED, nchr=3)
    af, reads = anno.in_file_order(), synth.make_reads(anno, 700, 6, SEED)
    e = capi.Engine(0)
    e.set_params(util.to_engine_params(capi, oracle.default_params(full_level=3)))
    e.set_outputs(capi.WANT_RESULTS)
    e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    e.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    e.run()
    e.sync()
    res = e.download()
    extra = hand_reads(2)
    as_reads = [(int(reads.tid[i]), int(res.info[i]) & 0xff, int(res.ref_tx[i]),
                 [(int(res.ex_start[k]), int(res.ex_end[k]), int(res.ex_flag[k])) for k in range(int(res.ex_off[i]), int(res.ex_off[i + 1]))]) for i in range(reads.n)] + extra
    opts = dict(tx_gene=np.asarray(af.tx_gene, np.uint32), na_gene=int(af.n_genes), s=1, d=2, D=50, f=0.8)
    refs = [("chr%d" % (k + 1)).encode() for k in range(3)]
    want = nr.novel(as_reads, ref_names=refs, **opts)
    want["gtf"] = gtf_want(as_reads, want, opts, refs)
    # the restatement alone: offers, hits, a duplicate exon key, a kept row of every list
    assert want["offers"] >= 3 and want["hits"] >= 1 and want["items"][nr.EXON] > len(want["rows"][nr.EXON]) and all(len(r) > 0 for r in want["rows"])
    assert nr.in_order(as_reads)                                # (the generator sorts, the hand reads lie behind: the device route below is the device's)
    got = {}
    for route in ("device", "host"):
        if route == "host":
            monkeypatch.setenv("L2R_NOVEL_ROUTE", "host")
        for how in ("run", "download"):
            begin(e, opts, refs)
            e.novel_add(reads.tid, None if how == "run" else res)
            e.novel_add(*as_result(extra))
            got[route, how] = results(e)
            st = got[route, how]["stats"]
            assert st["route"] == (1 if route == "host" else 0) and st["reads"] == reads.n + len(extra) and st["adds"] == 2, (route, how, st)
    monkeypatch.delenv("L2R_NOVEL_ROUTE")
    for key, g in got.items():
        same(g, want, key)
    begin(e, opts, refs)
    for bad_n in (reads.n - 1, reads.n + 1):                    # n differing from the run's reads
        with pytest.raises(capi.L2RError) as err:
            e.novel_add(reads.tid[:bad_n] if bad_n < reads.n else np.append(reads.tid, 0))
        assert "%d reads, the last run had %d" % (bad_n, reads.n) in str(err.value) and "rc=-1:" in str(err.value)
    e.close()
