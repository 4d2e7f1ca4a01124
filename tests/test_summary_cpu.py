"""The read classes and unique counts of `update-gtf -y`, the parts that need no GPU: the host side of l2r_summary_* -- the class of a
read, the argument checks, the route test and the exact host routine summary_host -- as a stand-alone program under ASan + UBSan
(tests/summary_dump.hip, `make -C lr2rmats_amd/csrc summary-dump`) against tests/summary_restatement.py: four
tests/uniq_restatement.merge lists and the class function."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import summary_cases as sc
from tests import summary_restatement as sr
from tests import uniq_restatement as ur
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SUMMARY_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "summary_dump")


@pytest.fixture(scope="module")
def summary_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "summary-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return SUMMARY_DUMP


def case_bytes(reads, s=0, d=0, D=ur.INT_MAX, f=0.8, have=(0, 0), sizes=None):
    tid, info, xs, xe = sr.columns(reads)
    bits = int(np.asarray(f, np.float32).view(np.uint32))
    n, nx = sizes if sizes is not None else (len(tid), len(xs))
    head = struct.pack("<8q", n, nx, s, d, D, bits, have[0], have[1])
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in (tid, info, xs, xe))


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


# ---------------------------------------------------------------------------------------------------- the restatement by hand

def test_the_info_bits_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    for name, value in (("KNOWN", sr.KNOWN), ("KNOWN_SITE", sr.KNOWN_SITE), ("FULL", sr.FULL), ("REV", sr.REV), ("UNREL", sr.UNREL)):
        assert int(re.search(r"^#define\s+L2R_INFO_%s\s+(0x[0-9a-f]+)u" % name, text, re.M).group(1), 16) == value


def test_restatement_on_the_cases_derived_by_hand():
    """What the cases are built to show, written down from the rule (not from a program's output)."""
    reads, want = sc.bit_combinations()
    assert len(reads) == 16 and [sr.klass(r[1]) for r in reads] == want and sorted(set(want)) == [0, 1, 2, 3]
    assert sr.counts(reads) == [8, 2, 2, 4, 8, 2, 2, 4]
    assert sr.counts(sc.twins(0, 1)) == [1, 1, 0, 0, 1, 1, 0, 0]            # two identical chains in two classes: 2 unique
    assert sr.counts(sc.twins(2, 2)) == [0, 0, 2, 0, 0, 0, 1, 0]            # in one class: 1
    for k in (1, 63, 64, 65, 200):
        assert sr.counts(sc.long_chains(k), f=0.5) == [3, 2, 0, 1, 2, 1, 0, 1], k
    assert sr.counts(sc.one_cluster(7)) == [0, 7, 0, 0, 0, 1, 0, 0]
    a, b = sc.descends_overall(), sc.descends_in_a_class()
    assert not ur.in_order([(t, 0, ch) for t, _b, ch in a]) and sr.in_order(a) and not sr.in_order(b)
    assert sr.counts(a) == [5, 5, 0, 0, 5, 5, 0, 0] and sr.counts(b) == [6, 5, 0, 0, 5, 5, 0, 0]


def test_one_list_over_the_class_keyed_concatenation_is_the_four_lists():
    """The argument of the device route on the restatement alone: the reads in class-major order with tid' = class << 29 | tid, offered
    to one list, are pushed class by class as often as the four lists are long -- and one list over the reads as they come is not."""
    reads = sc.generated()
    want = sr.counts(reads, **sc.GENERATED_OPTS)
    major = [(sr.klass(b) << 29 | tid, 1 if b & sr.REV else 0, chain) for c in range(4) for tid, b, chain in reads if sr.klass(b) == c]
    one = ur.merge(major, **sc.GENERATED_OPTS)
    pushed = [int(sum(1 for t, m in zip(major, one["merged"]) if t[0] >> 29 == c and not m)) for c in range(4)]
    assert pushed == want[4:]
    plain = ur.merge([(tid, 1 if b & sr.REV else 0, chain) for tid, b, chain in reads], **sc.GENERATED_OPTS)
    assert len(plain["u_src"]) < sum(want[4:])


def test_the_generated_set_holds_every_kind():
    """... by the restatement alone: every class is there, and every class has a push and a hit of each kind."""
    reads = sc.generated()
    merges = sr.per_class(reads, **sc.GENERATED_OPTS)
    assert 1900 <= len(reads) <= 2000 and sr.in_order(reads)
    for c, m in enumerate(merges):
        assert len(m["merged"]) >= 100 and len(m["u_src"]) >= 1 and min(m["hits"]) >= 1, (c, len(m["merged"]), m["hits"])


# ---------------------------------------------------------------------------------------------------- summary_host (summary_dump)

def test_every_case(summary_dump, tmp_path):
    cases = sc.cases()
    names = sorted(cases)
    got = dump(summary_dump, tmp_path, [case_bytes(cases[k][0], **cases[k][1]) for k in names])
    for k, g in zip(names, got):
        reads, opts = cases[k]
        assert int(g["rc"][0]) == 0, (k, g.get("error", np.zeros(0, np.uint8)).tobytes())
        assert list(g["class"]) == [sr.klass(r[1]) for r in reads], k
        assert list(g["counts"]) == sr.counts(reads, **opts), (k, list(g["counts"]))
        assert int(g["in_order"][0]) == int(sr.in_order(reads)), k


def test_input_that_descends_inside_a_class(summary_dump, tmp_path):
    reads = sc.descends_in_a_class()
    (g,) = dump(summary_dump, tmp_path, [case_bytes(reads)])
    assert int(g["rc"][0]) == 0 and int(g["in_order"][0]) == 0 and list(g["counts"]) == sr.counts(reads)


def test_the_checks_at_their_edges(summary_dump, tmp_path):
    edges = sc.edge_cases()
    names = sorted(edges)
    got = dump(summary_dump, tmp_path, [case_bytes(edges[k][0]) for k in names])
    for k, g in zip(names, got):
        refusal = edges[k][1]
        if refusal is None:
            assert int(g["rc"][0]) == 0 and list(g["counts"]) == sr.counts(edges[k][0]), k
        else:
            assert int(g["rc"][0]) == -1 and refusal in g["error"].tobytes().decode(), (k, g["error"].tobytes())


def test_the_totals(summary_dump, tmp_path):
    one = sc.twins(0, 0)
    bad = {
        "2147483648 reads in all": case_bytes(one, have=((1 << 31) - 2, 0)),
        "4294967232 exons in all": case_bytes(one, have=(0, (1 << 32) - 64 - 4)),
        "negative size": case_bytes([], sizes=(-1, 0)),
    }
    names = sorted(bad)
    got = dump(summary_dump, tmp_path, [bad[k] for k in names] + [case_bytes(one, have=((1 << 31) - 3, (1 << 32) - 64 - 5))])
    for k, g in zip(names, got):
        assert int(g["rc"][0]) == -1 and k in g["error"].tobytes().decode(), (k, g["error"].tobytes())
    assert int(got[-1]["rc"][0]) == 0                                # one below both bounds
