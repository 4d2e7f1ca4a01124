"""The case table of tests/filter_fusion_cases.py, kept honest without a GPU: the restatements give the answers worked by hand, every
threshold triple holds both verdicts, every input at which the widths decide gives another verdict when the comparison is redone in the
wrong width, and no family is all one verdict."""
import numpy as np
import pytest

from oracle import filter_oracle as fo
from tests import filter_fusion_cases as fc

CASES = fc.all_cases()
RUN = [c for c in CASES if c.kind != "args"]
WANT = {}


def want(case):
    if (case.family, case.name) not in WANT:
        WANT[(case.family, case.name)] = fc.want(case)
    return WANT[(case.family, case.name)]


def _id(c):
    return "%s-%s" % (c.family, c.name)


def test_names_are_unique_and_every_case_states_its_rule():
    ids = [_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert all(len(c.rule) > 10 for c in CASES)
    assert {c.family for c in CASES} == set("abcdefg")


@pytest.mark.parametrize("case", [c for c in RUN if c.hand is not None], ids=_id)
def test_restatement_gives_the_hand_answers(case):
    w = want(case)
    if case.kind == "select":
        assert list(w) == list(case.hand), case.rule
    elif case.kind == "spans":
        assert list(w[:len(case.hand)]) == list(case.hand), case.rule
    else:
        assert len(w) == len(case.hand)
        for k, (a, b) in enumerate(zip(w, case.hand)):
            assert [int(x) for x in a] == list(b), (case.rule, k)


def test_wrapped_sums_by_hand():
    """17 * (2^28 - 1) = 2^32 + 268435439 and 9 * (2^28 - 1) = 2^32 - 1879048201."""
    assert 17 * 0xFFFFFFF - (1 << 32) == 268435439 and fc.i32(17 * 0xFFFFFFF) == 268435439
    assert 9 * 0xFFFFFFF - (1 << 32) == -1879048201 and fc.i32(9 * 0xFFFFFFF) == -1879048201
    assert fc.i32(-1) == -1 and fc.i32((1 << 31)) == -(1 << 31) and fc.i32((1 << 32) + 5) == 5


TRIPLES = [c for c in CASES if c.triple is not None]


@pytest.mark.parametrize("case", TRIPLES, ids=_id)
def test_threshold_triples_hold_both_verdicts(case):
    """(just failing, exactly at, just passing): failing and passing by the restatement alone."""
    v = fc.kept(case, want(case))
    failing, at, passing = case.triple
    assert v[failing] is not None and not v[failing] and v[passing], (case.rule, v)
    assert at is None or at not in (failing, passing)


def test_every_comparison_has_a_triple_and_a_deciding_input():
    names = " ".join(c.name for c in TRIPLES)
    for word in ("cov_", "identity_", "second_", "each_cov_", "all_cov_", "ovlp_"):
        assert word in names
        assert any(c.mix for c in CASES if c.name.startswith(word)), word
        for v in ("0.25", "0.5"):                                                 # the plain > against >= cases
            assert any(c.name == "%s%s_equal" % (word, v) for c in TRIPLES), (word, v)


MIXED = [c for c in CASES if c.mix is not None]


@pytest.mark.parametrize("case", MIXED, ids=_id)
def test_deciding_inputs_decide(case):
    """The comparison redone with numpy scalars: the reference's widths give the restatement's verdict, the wrong width another one."""
    v = fc.mix_verdicts(case.mix)
    at = case.triple[1] if case.triple is not None and case.triple[1] is not None else 0
    assert v["ref"] == bool(fc.kept(case, want(case))[at]), (case.rule, v)
    assert v[case.mix["wrong"]] != v["ref"], (case.rule, v)


def test_the_table_of_the_issue():
    """Verdict by verdict: the reference's arithmetic and the alternative named in the issue."""
    t = {c.name: fc.mix_verdicts(c.mix) for c in MIXED}
    assert t["cov_0.67_of_100"]["ref"] is False and t["cov_0.67_of_100"]["float"] is True
    assert t["identity_0.8_of_10"]["ref"] is True and t["identity_0.8_of_10"]["double"] is False
    assert t["identity_0.8_of_5"]["ref"] is True and t["identity_0.8_of_5"]["double"] is False
    assert t["identity_beyond_2^24"]["ref"] is True and t["identity_beyond_2^24"]["int"] is False and t["identity_beyond_2^24"]["double"] is False
    assert t["second_0.98_of_100"]["ref"] is False and t["second_0.98_of_100"]["double"] is True
    assert t["second_0.98_of_50"]["ref"] is False and t["second_0.98_of_50"]["double"] is True
    assert t["each_cov_0.1_of_100"]["ref"] is False and t["each_cov_0.1_of_100"]["float"] is True
    assert t["all_cov_0.99_of_100"]["ref"] is True and t["all_cov_0.99_of_100"]["double"] is False
    assert t["ovlp_0.7_of_10"]["ref"] is True and t["ovlp_0.7_of_10"]["double"] is False
    # the float neighbours used by the triple of the coverage test
    assert np.float32(0.67) == np.float32(11240735 / 2 ** 24) and np.float64(11240735) / np.float64(2 ** 24) == np.float64(np.float32(0.67))


@pytest.mark.parametrize("family", "abcdf")
def test_no_family_is_all_one_verdict(family):
    v = [x for c in fc.by_family(family) for x in fc.kept(c, want(c))]
    assert 0.1 * len(v) < sum(v) < 0.9 * len(v), (family, sum(v), len(v))


def test_family_a_both_verdicts_per_kernel():
    for kind in ("score", "select", "fsel"):
        v = [x for c in fc.by_family("a") if c.kind == kind for x in fc.kept(c, want(c))]
        assert any(v) and not all(v), kind


def test_family_e_shapes():
    """Every operation count and record count of the issue is there, in both strands, and no two operation lengths of a record are equal."""
    cases = {c.name: c for c in fc.by_family("e")}
    counts = sorted({len(r["cigar"]) for r in cases["operation_counts"].inputs["records"]})
    assert counts == [0, 1, 2, 63, 64, 65, 127, 128, 129, 4097]
    for r in cases["operation_counts"].inputs["records"]:
        lens = [l for (l, _) in r["cigar"]]
        assert len(set(lens)) == len(lens)
        assert all(op in (fc.M, fc.I, fc.D, fc.N, fc.EQ, fc.X, fc.S) for (_, op) in r["cigar"])      # every word counts in some sum
    assert {r["flag"] for r in cases["operation_counts"].inputs["records"]} == {0, 16}
    assert all("%d_records" % n in cases and len(cases["%d_records" % n].inputs["records"]) == n for n in (1, 3, 4, 5, 257))
    for name, total, form in (("auto_128", 128, 0.0), ("auto_129", 129, 1.0)):
        recs = cases[name].inputs["records"]
        assert len(recs) == 4 and sum(len(r["cigar"]) for r in recs) == total and cases[name].inputs["auto_wave"] == form
        assert (total / 4 > 32.0) == bool(form)
    w = want(cases["sums_wrap"])
    assert [int(x[0]) for x in w] == [6, 268435444, 101, 268435539, 268435444]


def test_family_b_reaches_rlen_through_a_span_table():
    """k_filter_score's third sum shows only through the -r lookup: one case turns on every operation code, counted and not, one on a
    record of no reference base, and each holds a hit and a miss."""
    cases = {c.name: c for c in fc.by_family("b")}
    with_spans = [c for c in cases.values() if c.inputs.get("spans")]
    assert {c.name for c in with_spans} >= {"only_I_and_S", "rlen_per_operation", "rlen_of_every_operation"}
    for c in with_spans:
        v = fc.kept(c, want(c))
        assert any(v) and not all(v), c.name
        assert all(x for x in fc.kept(c, fc.want_score(c.inputs["records"], c.inputs["prm"], None))), c.name      # without -r every record stays
    per_op = cases["rlen_per_operation"].inputs["records"]
    assert sorted(r["cigar"][1][1] for r in per_op) == list(range(16)) and all(r["cigar"][1][0] == 7 for r in per_op)
    assert [bool(d) for d in want(cases["rlen_per_operation"])[0]] == [r["cigar"][1][1] in fo.REF_CONSUMING for r in per_op]
    only = cases["only_I_and_S"].inputs["records"]
    assert all(op in (fc.I, fc.S) for r in only for (_, op) in r["cigar"])


def test_family_d_and_f_group_counts():
    for fam, key in (("d", "group_off"), ("f", "groups")):
        cases = {c.name: c for c in fc.by_family(fam)}
        for n in (255, 256, 257):
            c = cases["%d_groups" % n]
            assert len(c.inputs[key]) - (1 if fam == "d" else 0) == n
            v = fc.kept(c, want(c))
            assert v[-1] and any(v[:-1]) and not all(v[:-1])
