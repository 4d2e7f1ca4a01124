"""The detail table of `update-gtf -A`, the parts that need no GPU: tests/detail_restatement.py against the hand-written golden
(tests/golden/detail) and, fed the oracle's result arrays, against the committed detail files of tests/golden/hand and tests/golden/toy;
and the host side of l2r_detail_* -- the argument checks, detail_line_bytes, detail_cut and the exact host routine detail_text_host -- as
a stand-alone program under ASan + UBSan (tests/detail_dump.hip, `make -C lr2rmats_amd/csrc detail-dump`) against the restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from oracle import pyoracle as po
from tests import detail_cases as dc
from tests import detail_restatement as dr
from tests.test_hand_known_answers import CASES as HAND_CASES
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DETAIL_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "detail_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "detail")
HAND = os.path.join(ROOT, "tests", "golden", "hand")
TOY = os.path.join(ROOT, "tests", "golden", "toy")
SYMBOLS = ["l2r_detail_begin", "l2r_detail_rows", "l2r_detail_lines", "l2r_detail_out", "l2r_detail_stats"]


def golden():
    with open(os.path.join(GOLDEN, "hand.detail.txt"), "rb") as fh:
        return dr.from_json(os.path.join(GOLDEN, "hand.json")), fh.read()


# ---------------------------------------------------------------------------------------------------- the restatement

def test_restatement_equals_the_golden():
    case, want = golden()
    assert dr.text(case) == want
    assert [len(t) for t in dr.texts(case)] == [len(l) + 1 for l in want.split(b"\n")[:-1]]
    for i in range(len(case["tid"])):
        assert dr.split(case, i)[-1] < len(dr.line(case, i))


def test_the_golden_holds_what_it_should():
    case, want = golden()
    lines = want.split(b"\n")[:-1]
    assert [int(v) >> 8 for v in case["info"]] == [1, 3, 2, 3]                              # a one-exon read among them
    assert lines[0].endswith(b"\t1\t100\t200\t0\tNA\t0\tNA\t0\tNA\t0\tNA\t") and lines[2].endswith(b"\t0\tNA\t0\tNA\t0\tNA\t0\tNA\t")      # every list empty
    assert lines[1].endswith(b"\t3\t0,1,2\t4\t0,1,2,3\t2\t0,1\t2\t0,1")                    # every flag on every exon: the junction lists stop at n - 1
    assert b"\tNA\tNA\t" in lines[2] and int(case["ref_tx"][2]) < 0                         # ref < 0
    assert {l.split(b"\t")[2] for l in lines} == {b"+", b"-"} and {l.split(b"\t")[3] for l in lines} == {b"0", b"1", b"2"}
    # the two line endings: a tab behind an empty last list, none behind a list with members
    assert want.count(b"\tNA\t\n") == 2 and lines[3].endswith(b"\t0\tNA\t1\t1") and not lines[1].endswith(b"\t") and not lines[3].endswith(b"\t")


def job_case(argv):
    """The case of an update-gtf command line: its inputs through the host readers, the result arrays from the oracle."""
    job = hostlib.Job(argv, open_outputs=False)
    try:
        a, r, v = job.annotation_arrays(), job.read_arrays(), job.detail_views()
        prm = po.Params.from_buffer_copy(bytes(job.prm))
        res = po.classify_soa(r["tid"], r["pos"], r["rev"], r["cig_off"], r["cig"], a["tx_tid"], a["tx_start"], a["tx_end"], a["tx_rev"], a["tx_ex_off"],
                              a["ex_start"], a["ex_end"], sj=job.junction_arrays(), params=prm)
        return {"refs": v["refs"], "tid": r["tid"].copy(), "names": v["names"], "qname": v["qname"], "anno": v["anno"], "tx_gid": v["tx_gid"], "tx_gname": v["tx_gname"],
                "ex_off": res.ex_off, "xs": res.ex_start, "xe": res.ex_end, "f": res.ex_flag, "ref_tx": res.ref_tx,
                "info": (res.info & 0xff) | (np.diff(res.ex_off).astype(np.uint32) << 8)}            # (the oracle leaves the exon count to ex_off)
    finally:
        job.close()


HAND_DETAIL = sorted(k for k, v in HAND_CASES.items() if "detail" in v[3])


@pytest.mark.parametrize("name", HAND_DETAIL + ["toy_l3"])
def test_restatement_reproduces_the_committed_detail_files(name):
    """The oracle is the checker of the result arrays; the text over them is the restatement's."""
    if name == "toy_l3":
        argv, want = ["update-gtf", "-l", "3", os.path.join(TOY, "toy.sam"), os.path.join(TOY, "original.gtf")], os.path.join(TOY, "expect_l3.detail.txt")
    else:
        cmd, inp, anno, expect = HAND_CASES[name]
        argv = list(cmd) + [os.path.join(HAND, inp), os.path.join(HAND, anno if isinstance(anno, str) else "anno.gtf")]
        want = os.path.join(HAND, expect["detail"])
    case = job_case(argv)
    assert dr.error(case) is None
    with open(want, "rb") as fh:
        assert dr.HEADER + dr.text(case) == fh.read()


def test_symbols_in_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    for m in ("detail_begin", "detail_rows", "detail_lines", "detail_all", "detail_stats"):
        assert hasattr(capi.Engine, m), m
    assert capi.header_define("L2R_DETAIL_TILE") == capi.DETAIL_TILE and capi.header_define("L2R_DETAIL_LDS_BYTES") == capi.DETAIL_LDS_BYTES
    assert capi.header_define("L2R_ABI_VERSION") == 3


# ---------------------------------------------------------------------------------------------------- the host side (detail_dump)

@pytest.fixture(scope="module")
def detail_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "detail-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return DETAIL_DUMP


def dump(exe, tmp_path, cases):
    """The dumps of several case files from one run of the program."""
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


def check_sound(got, case):
    """Text, bytes and split of every read of a dump against the restatement."""
    want = dr.texts(case)
    assert int(got["rc"][0]) == 0 and int(got["text_rc"][0]) == 0
    assert not got["kind"].any()
    assert got["text"].tobytes() == b"".join(want)
    assert got["bytes"].tolist() == [len(t) for t in want]                                   # detail_line_bytes == len(line), read by read
    assert got["split"].reshape(-1, 6).tolist() == [dr.split(case, i) for i in range(len(want))]
    assert got["text_cut"].tobytes() == b"".join(want)


def test_golden_through_the_host_routine(detail_dump, tmp_path):
    case, want = golden()
    got, = dump(detail_dump, tmp_path, [dc.case_file(case)])
    check_sound(got, case)
    assert got["text"].tobytes() == want


def test_random_reads_against_the_restatement(detail_dump, tmp_path):
    rng = np.random.default_rng(3)
    cases = [dc.make_case(1, []), dc.make_case(2, [4]), dc.make_case(3, rng.choice([1, 1, 2, 3, 5, 8, 13, 40, 65, 130], 300)),
             dc.make_case(4, rng.choice([1, 2, 7], 40), n_tx=0), dc.make_case(5, [1, 2, 3, 70], flags=dc.ALL_FLAGS)]
    for got, case in zip(dump(detail_dump, tmp_path, [dc.case_file(c) for c in cases]), cases):
        check_sound(got, case)


def edge_cases():
    """Coordinates at the digit edges; index values at the same edges (reads of 5, 6, 50, 51, 500, 501 exons reach 9 / 10, 99 / 100 and
    999 / 1000 with 2j + 1, reads of 10, 11, 100, 101 with j); names of 0, 1 and 254 bytes."""
    E = dc.EDGES
    a = dc.make_case(7, [1] * len(E) + [2] * len(E), flags=dc.ALL_FLAGS, name_len=(254, 254), gene_len=(254, 254), no_ref=0.0)
    a["xs"][:len(E)] = E
    a["xe"][:len(E)] = E
    a["xs"][len(E)::2], a["xe"][len(E)::2], a["xs"][len(E) + 1::2], a["xe"][len(E) + 1::2] = 0, E, E, 2147483647
    b = dc.make_case(8, [5, 6, 10, 11, 50, 51, 100, 101, 500, 501, 1001], flags=dc.ALL_FLAGS, name_len=(0, 1), gene_len=(0, 1), refs=(b"1", b"c" * 300))
    c = dc.make_case(9, [5, 6, 50, 51, 500, 501], flags=2, name_len=(1, 1))               # donors alone: 2j
    d = dc.make_case(10, [5, 6, 50, 51, 500, 501], flags=4)                                # acceptors alone: 2j + 1
    return [a, b, c, d]


def test_digit_edges_and_names(detail_dump, tmp_path):
    cases = edge_cases()
    for got, case in zip(dump(detail_dump, tmp_path, [dc.case_file(c) for c in cases]), cases):
        check_sound(got, case)
    assert b",9\t" in dr.text(cases[3]) and b",99\t" in dr.text(cases[3]) and b",999\t" in dr.text(cases[3])           # 2j + 1 reaches the edges
    assert b",1000\t" in dr.text(cases[1]) and b",1999\t" in dr.text(cases[1])            # j and 2j + 1 of 1 001 exons


def error_cases():
    """(case, smallest bad read, kind): every domain error, the bad read behind good ones and in front of a second bad one."""
    out = []
    base = dc.make_case(11, [2, 1, 3, 1, 2, 4], no_ref=0.0)

    def variant(kind, read, **change):
        c = dict(base)
        c.update(change)
        out.append((c, read, kind))

    def col(name, at, v, t=None):
        a = np.array(base[name] if t is None else t).copy()
        a[at] = v
        return a
    n_tx = len(base["tx_gid"])
    variant("tid", 3, tid=col("tid", 3, len(base["refs"])))
    variant("tid", 1, tid=col("tid", 4, -1, col("tid", 1, -1)))
    variant("qname_id", 4, qname=col("qname", 4, len(base["names"])))
    variant("qname_id", 0, qname=col("qname", 0, 0xffffffff))
    variant("qname_long", 1, names=base["names"] + b"L" * 255 + b"\0", qname=col("qname", 1, len(base["names"])))
    variant("qname_nul", 5, names=base["names"] + b"tail-without-nul", qname=col("qname", 5, len(base["names"]) + 3))
    variant("ref", 2, ref_tx=col("ref_tx", 2, n_tx))
    variant("ref", 0, ref_tx=col("ref_tx", 0, 2147483647))
    r3, r5 = int(base["ref_tx"][3]), int(base["ref_tx"][5])
    first3, first5 = int(np.flatnonzero(base["ref_tx"] == r3)[0]), int(np.flatnonzero(base["ref_tx"] == r5)[0])   # (reads share transcripts: the first of them)
    variant("gene_id", first3, tx_gid=col("tx_gid", r3, len(base["anno"])))
    variant("gene_id", first5, tx_gname=col("tx_gname", r5, 0xfffffff0))
    variant("gene_long", first3, anno=base["anno"] + b"G" * 255 + b"\0", tx_gname=col("tx_gname", r3, len(base["anno"])))
    variant("gene_nul", first3, anno=base["anno"] + b"no-nul", tx_gid=col("tx_gid", r3, len(base["anno"]) + 1))
    info = np.array(base["info"]).copy(); info[2] &= 0xff                                    # read 2 loses its exons
    off = np.array(base["ex_off"]).copy(); off[3:] -= 3
    variant("noexon", 2, info=info, ex_off=off, xs=np.delete(base["xs"], [3, 4, 5]), xe=np.delete(base["xe"], [3, 4, 5]), f=np.delete(base["f"], [3, 4, 5]))
    variant("neg", 2, xs=col("xs", int(base["ex_off"][2]) + 1, -5))
    variant("neg", 3, xe=col("xe", int(base["ex_off"][3]), -2147483648))
    # the kinds are looked for in one order: a bad reference in front of a bad read name, that in front of a bad transcript index and so on
    variant("tid", 2, tid=col("tid", 2, 99), qname=col("qname", 2, 0xffffffff))
    variant("qname_id", 2, qname=col("qname", 2, 0xffffffff), ref_tx=col("ref_tx", 2, n_tx))
    variant("ref", 2, ref_tx=col("ref_tx", 2, n_tx), xs=col("xs", int(base["ex_off"][2]), -1))
    variant("gene_id", first3, tx_gid=col("tx_gid", r3, len(base["anno"])), xs=col("xs", int(base["ex_off"][first3]), -1))
    # the smallest read wins whatever its kind
    variant("neg", 0, xs=col("xs", 0, -1), tid=col("tid", 1, -1))
    return out


def test_every_domain_error(detail_dump, tmp_path):
    cases = error_cases()
    for c, read, kind in cases:
        assert dr.error(c) == (read, kind)
    for got, (c, read, kind) in zip(dump(detail_dump, tmp_path, [dc.case_file(c) for c, _, _ in cases]), cases):
        assert int(got["rc"][0]) == 0
        bad = np.flatnonzero(got["kind"])
        assert int(bad[0]) == read and int(got["kind"][read]) == dr.KIND_CODE[kind]
        assert int(got["bytes"][read]) == 0
        assert int(got["text_rc"][0]) == -1 and "text" not in got
        msg = got["error"].tobytes().decode()
        assert "read %d:" % read in msg and dr.KIND_TEXT[kind] in msg


def test_the_cut_at_its_edges(detail_dump, tmp_path):
    case = dc.make_case(17, [1, 2, 3, 1, 40, 1, 1, 2, 5, 1, 1, 1])
    texts = dr.texts(case)
    lens = [len(t) for t in texts]
    s3, big = sum(lens[:3]), lens[4]
    plans = [(0, 1, 1 << 30), (0, 3, 1 << 30), (0, len(lens), 1 << 30), (0, len(lens) + 1, 1 << 30), (0, len(lens) - 1, 1 << 30),
             (0, 1 << 20, s3 - 1), (0, 1 << 20, s3), (0, 1 << 20, s3 + 1),                 # max_bytes at a row boundary -1, 0, +1
             (0, 1 << 20, big - 1), (0, 1 << 20, big), (0, 1 << 20, big + 1),               # a single row over / at the batch limit: taken alone
             (0, 1 << 20, 1), (5, 2, lens[5] + lens[6]), (5, 2, lens[5] + lens[6] - 1)]
    got = dump(detail_dump, tmp_path, [dc.case_file(case, f, mr, mb) for f, mr, mb in plans])
    for g, (f, mr, mb) in zip(got, plans):
        want, at = [], f
        while at < len(lens):
            k = dr.cut(lens, at, mr, mb)
            assert k >= 1
            want.append(k)
            at += k
        assert g["cut"].tolist() == want, (f, mr, mb)
        assert g["cut_bytes"].tolist() == [sum(lens[a:a + k]) for a, k in zip(np.cumsum([f] + want[:-1]).tolist(), want)]
        assert g["text_cut"].tobytes() == b"".join(texts[f:])                               # batches concatenated: the text however it was cut
    assert got[5]["cut"][0] == 2 and got[6]["cut"][0] == 3 and got[7]["cut"][0] == 3
    assert got[11]["cut"].tolist() == [1] * len(lens)                                       # every row is over the limit: one each


def test_the_cut_at_the_32_bit_bound(detail_dump, tmp_path):
    """Made-up lengths: the summed bytes of a batch stay below 2^32 - 64 whatever max_bytes says, and a row is always taken."""
    B = dr.BATCH_BYTES
    case = dc.make_case(19, [1])
    fakes = [[B - 1, 1, 5], [B - 2, 1, 5], [B // 2, B // 2 - 1, 1, 1], [B // 2, B // 2, 7], [0xffffffff, 0xffffffff, 3]]
    got = dump(detail_dump, tmp_path, [dc.case_file(case, 0, 1 << 40, 1 << 62, fake=f) for f in fakes])
    for g, f in zip(got, fakes):
        want, at = [], 0
        while at < len(f):
            k = dr.cut(f, at, 1 << 40, 1 << 62)
            want.append(k)
            at += k
        assert g["fake_cut"].tolist() == want, f
        bounds = np.cumsum([0] + want)
        assert g["fake_cut_bytes"].tolist() == [sum(f[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    assert got[0]["fake_cut"].tolist() == [1, 2] and got[1]["fake_cut"].tolist() == [2, 1]
    assert got[2]["fake_cut"].tolist() == [2, 2] and got[3]["fake_cut"].tolist() == [1, 2] and got[4]["fake_cut"].tolist() == [1, 1, 1]
    bad = dump(detail_dump, tmp_path, [dc.case_file(case, 3, 1, 1, fake=[1, 2, 3]), dc.case_file(case, 0, 0, 1, fake=[1]), dc.case_file(case, 0, 1, 0, fake=[1])])
    for g in bad:
        assert "fake_cut_error" in g and g["fake_cut"].size == 0


def test_argument_errors(detail_dump, tmp_path):
    base = dc.make_case(21, [1, 2])
    bad = [dc.case_file(base, res_n=3), dc.case_file(base, res_x=2), dc.case_file(base, res_x=1 << 33)]
    c = dict(base); c["ex_off"] = np.asarray([0, 2, 3], np.int64); bad.append(dc.case_file(c))           # ex_off against the exon counts of info
    c = dict(base); c["ex_off"] = np.asarray([1, 2, 4], np.int64); bad.append(dc.case_file(c))
    c = dict(base); c["refs"] = [b"r" * 65536]; c["tid"] = np.zeros(2, np.int32); bad.append(dc.case_file(c))
    for got in dump(detail_dump, tmp_path, bad):
        assert int(got["rc"][0]) == -2 and got["error"].size and "text" not in got and "kind" not in got
