"""The host half of `filter` and `fusion` without a GPU: lr2rmats_amd/csrc/l2r_filterplan.hip.h -- the table of the -r transcripts, the
lookup k_filter_score calls, the argument checks of the four entry points -- as a stand-alone program under ASan + UBSan
(tests/filter_dump.hip, `make -C lr2rmats_amd/csrc filter-dump`) over the families c and g of tests/filter_fusion_cases.py.  The table
equals its definition, every probe answer the reference's walk (remove_overlap of oracle/filter_oracle.py); a report of either sanitizer
fails the case."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import filter_fusion_cases as fc
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FILTER_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "filter_dump")
SPAN_CASES = fc.by_family("c")
ARG_CASES = fc.by_family("g")


@pytest.fixture(scope="module")
def filter_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "filter-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return FILTER_DUMP


def case_bytes(spans=(), probes=(), check=0, n=0, n_cigar=0, off=(), null_mask=0, null_spans=False):
    head = struct.pack("<8q", len(spans), len(probes), check, n, n_cigar, len(off), null_mask, int(null_spans))
    cols = [np.asarray([s[k] for s in spans], "<i4").tobytes() for k in range(3)]
    return head + b"".join(cols) + np.asarray(probes, "<i4").reshape(-1).tobytes() + np.asarray(off, "<i8").tobytes()


def dump(exe, tmp_path, cases):
    """The dumps of several cases from one run of the program."""
    args = []
    for k, c in enumerate(cases):
        src, dst = str(tmp_path / ("case%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        with open(src, "wb") as fh:
            fh.write(c)
        args += [src, dst]
    env = dict(os.environ)
    env.update(SAN_ENV)
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    for m in MARKS:
        assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
    return [_read_dump(a) for a in args[1::2]]


@pytest.fixture(scope="module")
def span_dumps(filter_dump, tmp_path_factory):
    got = dump(filter_dump, tmp_path_factory.mktemp("spans"), [case_bytes(c.inputs["spans"], c.inputs["probes"]) for c in SPAN_CASES])
    return {c.name: g for c, g in zip(SPAN_CASES, got)}


@pytest.mark.parametrize("case", SPAN_CASES, ids=[c.name for c in SPAN_CASES])
def test_span_table_and_lookup(span_dumps, case):
    got, spans, probes = span_dumps[case.name], case.inputs["spans"], case.inputs["probes"]
    n_tid, off, start, pmax_end = fc.want_table(spans)
    assert int(got["n_tid"][0]) == n_tid, case.rule
    assert np.array_equal(got["off"], off) and np.array_equal(got["start"], start) and np.array_equal(got["pmax_end"], pmax_end), (case.rule, got, off, start, pmax_end)
    want = fc.want_spans(spans, probes)
    miss = np.flatnonzero(got["hit"] != want)
    assert miss.size == 0, (case.rule, [(probes[k], int(want[k])) for k in miss[:10]])
    assert list(want[:len(case.hand)]) == case.hand, case.rule                     # the restatement gives the answers worked by hand
    assert len(probes) > len(case.hand) or not spans                               # the grid is there


def test_span_cases_hold_both_answers():
    for c in SPAN_CASES:
        if c.inputs["spans"]:
            want = fc.want_spans(c.inputs["spans"], c.inputs["probes"])
            assert 0 < int(want.sum()) < len(want), c.name


def test_span_table_on_random_file_orders(filter_dump, tmp_path):
    """Small random tables (tids -1..3 in any file order, short coordinates): the table and a grid of probes."""
    rng = np.random.default_rng(3)
    cases = []
    for k in range(40):
        n = int(rng.integers(1, 9))
        spans = [(int(t), int(s), int(s + w)) for t, s, w in zip(rng.integers(-1, 4, n), rng.integers(1, 30, n), rng.integers(0, 12, n))]
        probes = [(t, lo, hi) for t in range(-1, 5) for lo in range(0, 44, 3) for hi in range(lo - 1, 44, 4)]
        cases.append((spans, probes))
    for (spans, probes), got in zip(cases, dump(filter_dump, tmp_path, [case_bytes(s, p) for s, p in cases])):
        n_tid, off, start, pmax_end = fc.want_table(spans)
        assert int(got["n_tid"][0]) == n_tid and np.array_equal(got["off"], off) and np.array_equal(got["start"], start) and np.array_equal(got["pmax_end"], pmax_end), spans
        assert np.array_equal(got["hit"], fc.want_spans(spans, probes)), spans


def arg_case_bytes(c):
    i = c.inputs
    names = fc.POINTERS[i["entry"]]
    mask = sum(1 << names.index(p) for p in i["null"])
    return case_bytes([(0, 1, 2)], (), fc.ENTRY_ID[i["entry"]], i["n"], i["n_cigar"], i["off"], mask, i["null_spans"])


@pytest.fixture(scope="module")
def arg_dumps(filter_dump, tmp_path_factory):
    got = dump(filter_dump, tmp_path_factory.mktemp("args"), [arg_case_bytes(c) for c in ARG_CASES])
    return {c.name: g for c, g in zip(ARG_CASES, got)}


@pytest.mark.parametrize("case", ARG_CASES, ids=[c.name for c in ARG_CASES])
def test_argument_checks(arg_dumps, case):
    got = arg_dumps[case.name]
    rc, msg = int(got["rc"][0]), got["error"].tobytes().decode()
    if case.hand is None:
        assert rc == 0 and msg == "", (case.rule, rc, msg)
    else:
        assert rc == -1 and msg == case.hand, (case.rule, rc, msg)


def test_every_entry_point_accepts_and_rejects():
    for entry in fc.POINTERS:
        mine = [c for c in ARG_CASES if c.inputs["entry"] == entry]
        assert any(c.hand is None for c in mine) and any(c.hand is not None for c in mine), entry
        assert any(c.inputs["n"] == 0 and c.hand is None for c in mine), entry
    assert any(c.hand == "[l2r_filter_score] cig_off descends at record 1" for c in ARG_CASES)
