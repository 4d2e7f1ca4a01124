"""The name order (`sort -n`, `filter -N`, `fusion -N`), the parts that need no GPU: the argument checks and the exact host routine of
l2r_name_order as a stand-alone program under ASan + UBSan (tests/name_dump.hip, `make -C lr2rmats_amd/csrc name-dump`) against
tests/name_order_restatement.py, the header rewrite (h_header_grouped), and `sort-check -n` on small SAM files."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import hostlib
from tests import name_order_restatement as nr
from tests.test_sort_cpu import REFS, SQ, _block, _line, _split
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "name_dump")


@pytest.fixture(scope="module")
def name_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "name-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return NAME_DUMP


def _run(exe, tmp_path, off, blob):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "order.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<q", len(off) - 1) + np.asarray(off, "<i8").tobytes() + bytes(blob))
    env = dict(os.environ)
    env.update(SAN_ENV)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    for m in MARKS:
        assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
    return _read_dump(dst)


def _order(exe, tmp_path, names):
    off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
    got = _run(exe, tmp_path, off, b"".join(names))
    assert int(got["rc"][0]) == 0, bytes(got.get("error", b"")).decode()
    want, groups = nr.name_order(names)
    assert got["order"].tolist() == want
    assert int(got["n_groups"][0]) == groups
    return got["order"].tolist()


A254, B254 = b"a" * 254, b"a" * 253 + b"b"
ORDER_CASES = {
    "n0": [],
    "n1": [b"r"],
    "n2_same": [b"r", b"r"],
    "n2_differ": [b"s", b"r"],
    "all_equal": [b"read7"] * 9,
    "all_distinct": [b"read%d" % k for k in (5, 3, 9, 1, 0, 8)],
    "empty_name_mixed": [b"x", b"", b"y", b"", b"x", b""],
    "one_and_254_bytes": [A254, b"a", B254, b"a", A254, b"b", B254],
    "prefix_pairs": [b"read1", b"read10", b"read", b"read1", b"read10", b"read100", b"read"],
    "last_byte_pairs": [b"read0000001", b"read0000002", b"read0000001", b"read0000003", b"read0000002"],
    "bytes_from_0x80": [b"\x80\xff", b"\x7f\xff", b"\xff", b"\x80\xff", b"\xff", b"\x7f\xff", b"\xfe\x80"],
    "ababa": [b"A", b"B", b"A", b"B", b"A"],
    "grouped_already": [b"q", b"q", b"p", b"z", b"z", b"z", b"a"],
}


@pytest.mark.parametrize("case", sorted(ORDER_CASES))
def test_host_routine_equals_the_restatement(name_dump, tmp_path, case):
    names = ORDER_CASES[case]
    got = _order(name_dump, tmp_path, names)
    if case == "grouped_already" or len(set(names)) == len(names) or len(set(names)) <= 1:
        assert got == list(range(len(names)))                       # grouped input: the identity
    if case == "ababa":
        assert got == [0, 2, 4, 1, 3]


def test_host_routine_on_random_names(name_dump, tmp_path):
    rng = np.random.default_rng(17)
    pool = [bytes(rng.integers(1, 256, int(rng.integers(0, 255))).astype(np.uint8)) for _ in range(120)]
    names = [pool[int(k)] for k in rng.integers(0, len(pool), 700)]
    _order(name_dump, tmp_path, names)


def test_rejections(name_dump, tmp_path):
    got = _run(name_dump, tmp_path, [0, 3, 258, 260], b"x" * 260)                 # a name of 255 bytes
    assert int(got["rc"][0]) != 0
    msg = bytes(got["error"]).decode()
    assert "l2r_name_order" in msg and "record 1" in msg and "255" in msg and "254" in msg
    assert "order" not in got
    got = _run(name_dump, tmp_path, [0, 4, 2, 6], b"x" * 6)                       # descending offsets
    msg = bytes(got["error"]).decode()
    assert int(got["rc"][0]) != 0 and "l2r_name_order" in msg and "descends" in msg and "record 1" in msg
    got = _run(name_dump, tmp_path, [0, 254, 508], A254 + B254)                   # 254 bytes is a name
    assert int(got["rc"][0]) == 0 and got["order"].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------------- h_header_grouped

HD = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n"
HEADER_CASES = [
    ("no_hd", SQ + "@PG\tID:x\n", HD + SQ + "@PG\tID:x\n"),
    ("empty", "", HD),
    ("hd_without_so_go", "@HD\tVN:1.5\n" + SQ, "@HD\tVN:1.5\tSO:unsorted\tGO:query\n" + SQ),
    ("so_coordinate", "@HD\tVN:1.6\tSO:coordinate\n" + SQ, HD + SQ),
    ("go_alone", "@HD\tVN:1.6\tGO:none\n" + SQ, "@HD\tVN:1.6\tGO:query\tSO:unsorted\n" + SQ),
    ("so_then_go", "@HD\tVN:1.6\tSO:coordinate\tGO:none\tSS:x\n" + SQ, "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:x\n" + SQ),
    ("go_then_so", "@HD\tGO:reference\tVN:1.6\tSO:queryname\n" + SQ, "@HD\tGO:query\tVN:1.6\tSO:unsorted\n" + SQ),
    ("as_wanted", HD + SQ, HD + SQ),
    ("crlf", "@HD\tVN:1.6\tSO:coordinate\r\n" + SQ, "@HD\tVN:1.6\tSO:unsorted\tGO:query\r\n" + SQ),
    ("hd_without_newline", "@HD\tVN:1.6", "@HD\tVN:1.6\tSO:unsorted\tGO:query"),
    ("not_hd", "@HDX\tVN:1.6\n" + SQ, HD + "@HDX\tVN:1.6\n" + SQ),
]


@pytest.mark.parametrize("name,text,want", HEADER_CASES, ids=[c[0] for c in HEADER_CASES])
def test_header_grouped(name, text, want):
    refs = [] if name == "empty" else REFS
    block = _block(text.encode(), refs)
    got = hostlib.header_grouped(block)
    l_text, got_text, rest = _split(got)
    assert l_text == len(want) and got_text == want.encode()
    assert rest == _split(block)[2]                              # n_ref and the references: untouched
    assert len(got) <= len(block) + hostlib.HEADER_GO_ROOM
    assert hostlib.header_grouped(got) == got                    # a second rewrite changes nothing


def test_header_grouped_rejects_a_corrupt_header():
    assert hostlib.header_grouped(b"") is None
    assert hostlib.header_grouped(b"BAM\2" + b"\0" * 8) is None
    assert hostlib.header_grouped(b"BAM\1" + struct.pack("<I", 100) + b"@HD\n" + b"\0" * 4) is None      # l_text beyond the block


def test_header_coordinate_is_what_it_was():
    block = _block(("@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + SQ).encode())
    assert _split(hostlib.header_coordinate(block))[1] == ("@HD\tVN:1.6\tSO:coordinate\tGO:query\n" + SQ).encode()


# ---------------------------------------------------------------------------------------------------- sort-check -n

GROUPED = [("r0", 0, "chr1", 5000), ("r0", 256, "chr2", 7), ("r1", 16, "chr1", 100), ("r2", 0, "chr1", 101), ("r2", 2048, "chr1", 100), ("r2", 256, "chr2", 8), ("r3", 0, "chr2", 9)]


def _write(path, rows):
    with open(path, "w") as fh:
        fh.write("@HD\tVN:1.6\tSO:unsorted\n" + SQ)
        for r in rows:
            fh.write(_line(*r))
    return str(path)


def _by_coordinate(rows):
    tid = {"chr1": 0, "chr2": 1}
    return sorted(rows, key=lambda r: (tid[r[2]], r[3], (r[1] >> 4) & 1))


def _check(args):
    r = hostlib.run_cli(["sort-check"] + args)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_sort_check_n_accepts_a_grouped_file(tmp_path):
    path = _write(tmp_path / "g.sam", GROUPED)
    rc, out, err = _check(["-n", path])
    assert rc == 0 and "name grouped: 7 records in 4 reads" in out, (out, err)
    assert hostlib.name_grouped(path) == (-1, 4)
    rc, out, _ = _check(["-n", _write(tmp_path / "e.sam", [])])
    assert rc == 0 and "0 records" in out


def test_sort_check_n_names_the_first_record_of_a_reopened_group(tmp_path):
    rows = _by_coordinate(GROUPED)
    names = [r[0] for r in rows]
    bad = nr.is_grouped(names)
    assert names == ["r2", "r1", "r2", "r0", "r0", "r2", "r3"] and bad == 2
    path = _write(tmp_path / "c.sam", rows)
    rc, out, _ = _check(["-n", path])
    assert rc == 1 and 'record 2 ("r2")' in out and "not name grouped" in out, out
    assert hostlib.name_grouped(path)[0] == 2
    # BAM input: the same verdict
    bam = str(tmp_path / "c.bam")
    assert hostlib.records_to_bam(path, bam) == 0
    assert _check(["-n", bam])[0] == 1
    # two names reopened: the earlier record is named
    rows = [("a", 0, "chr1", 1), ("b", 0, "chr1", 2), ("c", 0, "chr1", 3), ("b", 0, "chr1", 4), ("a", 0, "chr1", 5)]
    rc, out, _ = _check(["-n", _write(tmp_path / "d.sam", rows)])
    assert rc == 1 and 'record 3 ("b")' in out, out


def test_plain_sort_check_is_unchanged(tmp_path):
    rc, out, _ = _check([_write(tmp_path / "c.sam", _by_coordinate(GROUPED))])
    assert rc == 0 and "coordinate sorted: 7 records" in out
    rc, out, _ = _check([_write(tmp_path / "g.sam", GROUPED)])
    assert rc == 1 and 'record 2 ("r1")' in out and "not coordinate sorted" in out
    for args in ([], ["-n"], ["-x", "a.sam"], ["-n", "a.sam", "b.sam"]):
        rc, out, err = _check(args)
        assert rc == 2 and out == "" and "Usage:" in err, args


def test_usage_texts_name_the_new_options():
    assert b"-n --name" in hostlib.run_cli(["sort"]).stderr
    assert b"-N --group-names" in hostlib.run_cli(["filter"]).stderr
    assert b"-N --group-names" in hostlib.run_cli(["fusion"]).stderr
    assert b"sort-check [-n]" in hostlib.run_cli(["sort-check"]).stderr
