"""GPU: k_filter_score, k_filter_select, k_fusion_seg<false|true> and k_fusion_select at their arithmetic and shape edges, through
capi.Engine: every case of tests/filter_fusion_cases.py against the literal restatements of the reference's lines, every output array
compared exactly.  One engine for the module; a failure names the rule of its case."""
import ctypes as C

import numpy as np
import pytest

from tests import filter_fusion_cases as fc

pytestmark = pytest.mark.gpu


def _id(c):
    return "%s-%s" % (c.family, c.name)


def _kind(kind, *families):
    return [c for c in fc.by_family(*families) if c.kind == kind]


@pytest.fixture(scope="module")
def eng():
    from lr2rmats_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


def _fprm(prm):
    from lr2rmats_amd import capi
    return capi.CFilterParams(prm[0], prm[1], prm[2], prm[3])


def _uprm(prm):
    from lr2rmats_amd import capi
    return capi.CFusionParams(prm[0], prm[1], prm[2], prm[3])


def _equal(got, want, names, case):
    assert len(got) == len(want) == len(names)
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype)
        miss = np.flatnonzero(g != w)
        assert miss.size == 0, "%s: %s\n%s differs at %s: got %s, want %s" % (case.name, case.rule, name, miss[:8], g[miss[:8]], w[miss[:8]])


@pytest.mark.parametrize("case", _kind("score", "a", "b"), ids=_id)
def test_filter_score(eng, case):
    i = case.inputs
    spans = i.get("spans")
    got = eng.filter_score(*fc.columns(i["records"]), _fprm(i["prm"]), None if spans is None else tuple(np.asarray([s[k] for s in spans], np.int32) for k in range(3)))
    _equal(got, fc.want_score(i["records"], i["prm"], spans), ("drop", "score", "intron_n"), case)


@pytest.mark.parametrize("case", _kind("spans", "c"), ids=_id)
def test_filter_score_span_lookup(eng, case):
    """Family c through l2r_filter_score: one record per probe -- chromosome tid, pos = lo, hi - lo + 1 reference bases -- with -v 0 -q 0."""
    spans, probes = case.inputs["spans"], case.inputs["probes"]
    records = [fc.rec([(hi - lo + 1, fc.M)], tid=t, pos=lo) for (t, lo, hi) in probes]
    prm = (0.0, 0.0, 0.98, 0)
    cols = tuple(np.asarray([s[k] for s in spans], np.int32) for k in range(3))
    got = eng.filter_score(*fc.columns(records), _fprm(prm), cols)
    want = fc.want_score(records, prm, spans)
    assert np.array_equal(want[0], fc.want_spans(spans, probes))
    _equal(got, want, ("drop", "score", "intron_n"), case)
    if not spans:                                                                  # no -r at all: the same
        _equal(eng.filter_score(*fc.columns(records), _fprm(prm), None), want, ("drop", "score", "intron_n"), case)


@pytest.mark.parametrize("case", _kind("select", "a", "d"), ids=_id)
def test_filter_select(eng, case):
    i = case.inputs
    got = eng.filter_select(i["group_off"], i["score"], i["intron_n"], _fprm(i["prm"]))
    _equal((got,), (fc.want_select(i["group_off"], i["score"], i["intron_n"], i["prm"]),), ("winner",), case)


SEG_NAMES = ("read_start", "read_end", "ref_start", "ref_end", "qlen")
SEG_WANT = {}


def _seg_want(case):
    if case.name not in SEG_WANT:
        SEG_WANT[case.name] = fc.want_seg(case.inputs["records"])
    return SEG_WANT[case.name]


@pytest.mark.parametrize("wave", ["0", "1"], ids=["thread_form", "wave_form"])
@pytest.mark.parametrize("case", _kind("seg", "e"), ids=_id)
def test_fusion_segments(eng, monkeypatch, case, wave):
    monkeypatch.setenv("L2R_FUSION_WAVE", wave)
    flag, _, pos, _, _, off, cig = fc.columns(case.inputs["records"])
    got = eng.fusion_segments(flag, pos, off, cig)
    assert eng.fusion_stats()["wave_form"] == float(wave)
    _equal(got, _seg_want(case), SEG_NAMES, case)


@pytest.mark.parametrize("case", [c for c in _kind("seg", "e") if "auto_wave" in c.inputs], ids=_id)
def test_fusion_segments_chooses_its_form(eng, monkeypatch, case):
    monkeypatch.delenv("L2R_FUSION_WAVE", raising=False)
    flag, _, pos, _, _, off, cig = fc.columns(case.inputs["records"])
    got = eng.fusion_segments(flag, pos, off, cig)
    assert eng.fusion_stats()["wave_form"] == case.inputs["auto_wave"], case.rule
    _equal(got, _seg_want(case), SEG_NAMES, case)


@pytest.mark.parametrize("case", _kind("fsel", "a", "f"), ids=_id)
def test_fusion_select(eng, case):
    i = case.inputs
    got = eng.fusion_select(*fc.fsel_columns(i["groups"]), _uprm(i["prm"]))
    _equal(got, fc.want_fsel(i["groups"], i["prm"]), ("first", "second"), case)


# ------------------------------------------------------------------------------------------------ family g: the C-ABI's answers

SENTINEL = 0x55


def _call(eng, case):
    """The call of family g with real arrays (16 words at least, whatever the offsets say) and NULL where the case asks for it; returns
    (rc, message, the output arrays)."""
    from lr2rmats_amd import capi
    i = case.inputs
    entry, n, null = i["entry"], i["n"], set(i["null"])
    rows = max([n, i["n_cigar"], 16] + [int(x) for x in i["off"]])
    off = np.asarray(i["off"] if i["off"] else [0], np.int64)
    col = {p: np.zeros(rows, np.int32) for p in fc.POINTERS[entry]}
    col["flag"] = np.zeros(rows, np.uint16); col["cig"] = np.zeros(rows, np.uint32)
    outs = {p: np.full(rows * 8, SENTINEL, np.uint8).view(np.uint8 if p == "drop" else np.int64 if p in ("winner", "first", "second") else np.int32)      # (every byte)
            for p in ("drop", "score", "intron_n", "winner", "read_start", "read_end", "ref_start", "ref_end", "qlen", "first", "second")}
    ptr = lambda p, a: None if p in null else a.ctypes.data
    ctx = None if "ctx" in null else eng.ctx
    lib = eng.lib
    if entry in ("l2r_filter_score", "l2r_fusion_segments"):
        recs = capi.CFilterRecords(n, i["n_cigar"], ptr("flag", col["flag"]), ptr("tid", col["tid"]) if entry == "l2r_filter_score" else None, ptr("pos", col["pos"]),
                                   ptr("l_qseq", col["l_qseq"]) if entry == "l2r_filter_score" else None, ptr("nm", col["nm"]) if entry == "l2r_filter_score" else None,
                                   ptr("cig_off", off), ptr("cig", col["cig"]))
        precs = None if "recs" in null else C.byref(recs)
        if entry == "l2r_filter_score":
            prm = _fprm(fc.FILTER_PRM)
            one = np.asarray([0], np.int32)
            sp = capi.CFilterSpans(1, *([None] * 3 if i["null_spans"] else [one.ctypes.data] * 3))
            used = ("drop", "score", "intron_n")
            rc = lib.l2r_filter_score(ctx, precs, None if "prm" in null else C.byref(prm), C.byref(sp), *[ptr(p, outs[p]) for p in used])
        else:
            used = SEG_NAMES
            rc = lib.l2r_fusion_segments(ctx, precs, *[ptr(p, outs[p]) for p in used])
    elif entry == "l2r_filter_select":
        prm = _fprm(fc.FILTER_PRM)
        used = ("winner",)
        outs["score"] = np.zeros(rows, np.int32); outs["intron_n"] = np.zeros(rows, np.int32)      # (inputs here)
        rc = lib.l2r_filter_select(ctx, n, ptr("group_off", off), ptr("score", outs["score"]), ptr("intron_n", outs["intron_n"]), None if "prm" in null else C.byref(prm),
                                   ptr("winner", outs["winner"]))
    else:
        prm = _uprm(fc.FUSION_PRM)
        used = ("first", "second")
        names = ("score", "ed", "tid", "read_start", "read_end", "ref_start", "ref_end", "rlen_of_group")
        rc = lib.l2r_fusion_select(ctx, n, ptr("group_off", off), *[ptr(p, col[p]) for p in names], None if "prm" in null else C.byref(prm),
                                   ptr("first", outs["first"]), ptr("second", outs["second"]))
    return rc, lib.l2r_last_error().decode(), [outs[p] for p in used]


@pytest.mark.parametrize("case", fc.by_family("g"), ids=_id)
def test_rejected_arguments(eng, case):
    rc, msg, outs = _call(eng, case)
    n = case.inputs["n"]
    if case.hand is None:
        assert rc == 0, (case.rule, rc, msg)
        for o in outs:                                                             # n rows written, nothing behind them
            assert np.all(o.view(np.uint8)[n * o.itemsize:] == SENTINEL), case.rule
            assert n == 0 or not np.all(o.view(np.uint8)[:n * o.itemsize] == SENTINEL), case.rule
    else:
        assert rc == -1 and msg == case.hand, (case.rule, rc, msg)
        for o in outs:
            assert np.all(o.view(np.uint8) == SENTINEL), case.rule
