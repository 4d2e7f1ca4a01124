"""The GTF block of `bam2gtf` / `unique-gtf`, the parts that need no GPU: tests/gtf_text_restatement.py against the hand-written goldens
(tests/golden/gtf_text), and the host side of l2r_gtftext_* -- the argument checks, gtx_block_bytes, gtx_cut and the exact host routine
gtx_text_host -- as a stand-alone program under ASan + UBSan (tests/gtx_dump.hip, `make -C lr2rmats_amd/csrc gtx-dump`) against the
restatement."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi
from tests import gtf_text_cases as gc
from tests import gtf_text_restatement as gr
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GTX_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "gtx_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gtf_text")
NAMES = ("plain", "read", "read_default")
KIND_CODE = {"sel": 1, "tid": 2, "noexon": 3, "name_id": 4, "name_long": 5, "name_nul": 6, "neg": 7, "big": 8}     # GTX_E_* of l2r_gtftextplan.hip.h
SYMBOLS = ["l2r_gtftext_begin", "l2r_gtftext_rows", "l2r_gtftext_blocks", "l2r_gtftext_lines", "l2r_gtftext_out", "l2r_gtftext_stats"]


def golden(name):
    with open(os.path.join(GOLDEN, name + ".gtf"), "rb") as fh:
        return gr.from_json(os.path.join(GOLDEN, name + ".json")), fh.read()


# ---------------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_goldens(name):
    case, want = golden(name)
    assert gr.text(case) == want
    assert sum(gr.block_bytes(case, q) for q in range(case["m"])) == len(want)


def test_the_goldens_hold_what_they_should():
    plain, read = golden("plain")[1], golden("read")[1]
    assert b'\t-\t.\tgene_id "readB"' in plain and b'gene_id ""; transcript_id "x";' in plain
    assert plain.index(b"exon\t5\t9") < plain.index(b"exon\t100000\t999999")               # PLAIN with rev: ascending
    assert read.index(b"exon\t500\t650") < read.index(b"exon\t90\t200")                    # READ with rev: descending, overrides in the exon lines
    assert b'transcript_cov "10";' in read and b"\t.\t transcript_cov \"3\";\n" in read and b"\texon\t7\t8\t.\t-\t.\t\n" in read
    assert b"gene_name" not in read.split(b"\n")[0]


def test_symbols_in_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    for m in ("gtftext_begin", "gtftext_rows", "gtftext_blocks", "gtftext_lines", "gtftext_stats"):
        assert hasattr(capi.Engine, m), m
    assert capi.header_define("L2R_GTX_TILE") == capi.GTX_TILE and capi.header_define("L2R_GTX_LDS_BYTES") == capi.GTX_LDS_BYTES


# ---------------------------------------------------------------------------------------------------- the host side (gtx_dump)

@pytest.fixture(scope="module")
def gtx_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "gtx-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return GTX_DUMP


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
    """Text, lines and the bytes of every block of a dump against the restatement."""
    want = gr.texts(case)
    assert int(got["rc"][0]) == 0 and int(got["text_rc"][0]) == 0
    assert not got["kind"].any()
    assert got["text"].tobytes() == b"".join(want)
    assert got["bytes"].tolist() == [len(t) for t in want]                                   # gtx_block_bytes == len(text), block by block
    assert got["lines"].tolist() == [t.count(b"\n") for t in want]
    assert int(got["n_lines"][0]) == sum(t.count(b"\n") for t in want)
    assert got["text_cut"].tobytes() == b"".join(want)


def test_goldens_through_the_host_routine(gtx_dump, tmp_path):
    cases = [golden(n) for n in NAMES]
    for got, (case, want) in zip(dump(gtx_dump, tmp_path, [gc.case_file(c) for c, _ in cases]), cases):
        check_sound(got, case)
        assert got["text"].tobytes() == want


def random_cases():
    out = []
    for seed, form in ((1, gr.PLAIN), (2, gr.READ)):
        rng = np.random.default_rng(seed)
        exons = rng.choice([1, 1, 1, 2, 3, 5, 8, 13, 40, 120], 150)
        base = gc.make_case(seed, exons, form, empty_names=0.3 if form == gr.READ else 0.1)
        out.append(base)
        out.append(gc.with_selection(base, rng.integers(0, 150, 200), seed, overrides=True))
        out.append(gc.with_selection(base, None, seed, overrides=True))
        out.append(gc.with_selection(base, [], seed))
    return out


def test_random_blocks_against_the_restatement(gtx_dump, tmp_path):
    cases = random_cases()
    for got, case in zip(dump(gtx_dump, tmp_path, [gc.case_file(c) for c in cases]), cases):
        check_sound(got, case)


def test_digit_edges_names_and_source(gtx_dump, tmp_path):
    E = gc.EDGES
    cases = []
    for form in (gr.PLAIN, gr.READ):
        c = gc.make_case(5, [1] * len(E) + [2] * len(E), form, name_len=(254, 254), source=b"s" * 1023)
        c["xs"][:len(E)] = E
        c["xe"][:len(E)] = E
        c["xs"][len(E)::2], c["xe"][len(E)::2], c["xs"][len(E) + 1::2], c["xe"][len(E) + 1::2] = 0, E, E, 2147483647
        cases.append(c)
        d = gc.with_selection(gc.make_case(6, [3] * len(E), form, name_len=(0, 1), source=b"", empty_names=0.5), None)
        d["start"], d["end"], d["cov"] = np.asarray(E, np.int32), np.asarray(E[::-1], np.int32), np.asarray(E, np.int32)
        cases.append(d)
    for got, case in zip(dump(gtx_dump, tmp_path, [gc.case_file(c) for c in cases]), cases):
        check_sound(got, case)


def error_cases(form):
    """(case, smallest bad block, kind): every domain error, the bad block behind good ones and in front of a second bad one."""
    out = []
    base = gc.make_case(11, [2, 1, 3, 1, 2, 4], form)

    def variant(kind, block, **change):
        c = dict(base)
        for k, v in change.items():
            c[k] = v
        out.append((c, block, kind))
    n = len(base["tid"])

    def col(name, at, v, t=None):
        a = np.array(base[name] if t is None else t).copy()
        a[at] = v
        return a
    variant("sel", 2, sel=np.asarray([0, 1, n, 2, -1], np.int32), m=5)
    variant("sel", 0, sel=np.asarray([-1, 0], np.int32), m=2)
    variant("tid", 3, tid=col("tid", 3, len(base["refs"])))
    variant("tid", 1, tid=col("tid", 4, -1, col("tid", 1, -1)))
    off = np.array(base["ex_off"]).copy(); off[2] = off[3]                                   # transcript 2 loses its exons to transcript 1
    variant("noexon", 2, ex_off=off)
    variant("name_id", 4, tids=col("tids", 4, len(base["table"])))
    variant("name_id", 0, gid=col("gid", 0, 0xffffffff))
    long_table = base["table"] + b"L" * 255 + b"\0"
    variant("name_long", 1, table=long_table, gid=col("gid", 1, len(base["table"])))
    variant("name_nul", 5, table=base["table"] + b"tail-without-nul", tids=col("tids", 5, len(base["table"]) + 3))
    variant("neg", 2, xs=col("xs", int(base["ex_off"][2]) + 1, -5))
    variant("neg", 3, xe=col("xe", int(base["ex_off"][3]), -1))
    variant("neg", 1, start=np.asarray([1, -1, 1, 1, 1, 1], np.int32))
    variant("neg", 4, end=np.asarray([2000000000, 2000000000, 2000000000, 2000000000, -9, 2000000000], np.int32))
    variant("neg", 5, cov=np.asarray([1, 1, 1, 1, 1, -2147483648], np.int32))
    # the kinds are looked for in one order: a bad reference in front of a bad name
    variant("tid", 2, tid=col("tid", 2, 99), gid=col("gid", 2, 0xffffffff))
    if form == gr.READ:
        variant("name_id", 3, tname=col("tname", 3, len(base["table"]) + 7))
        variant("name_long", 0, table=long_table, gname=col("gname", 0, len(base["table"])), tname=col("tname", 0, 0xfffffff0))
    return out


def big_case(form):
    """One block whose text reaches 2^32 - 64 bytes behind a small one: long source and names, two million exons of ten digits."""
    c = gc.make_case(13, [1, 1], form, name_len=(254, 254), source=b"S" * 1023, refs=(b"chr1",))
    per_line = 4 + 1 + 1023 + 1 + 5 + 10 + 1 + 10 + 7 + (29 + 508 if form == gr.PLAIN else 3 + 7 + 13 + 9 + 15 + 16 + 4 * 254) + 1
    k = gr.BATCH_BYTES // per_line + 1
    c["ex_off"] = np.asarray([0, 1, 1 + k], np.int64)
    c["xs"] = np.concatenate([c["xs"][:1], np.full(k, 1000000000, np.int32)])
    c["xe"] = np.concatenate([c["xe"][:1], np.full(k, 2000000000, np.int32)])
    return c


@pytest.mark.parametrize("form", [gr.PLAIN, gr.READ])
def test_every_domain_error(gtx_dump, tmp_path, form):
    cases = error_cases(form) + [(big_case(form), 1, "big")]
    for c, block, kind in cases:
        assert gr.error(c, sizes_only=True) == (block, kind)
    for got, (c, block, kind) in zip(dump(gtx_dump, tmp_path, [gc.case_file(c) for c, _, _ in cases]), cases):
        assert int(got["rc"][0]) == 0
        bad = np.flatnonzero(got["kind"])
        assert int(bad[0]) == block and int(got["kind"][block]) == KIND_CODE[kind]
        assert int(got["text_rc"][0]) == -1 and "text" not in got
        msg = got["error"].tobytes().decode()
        assert "block %d:" % block in msg and gr.KIND_TEXT[kind] in msg


def test_the_cut_at_its_edges(gtx_dump, tmp_path):
    case = gc.make_case(17, [1, 2, 3, 1, 40, 1, 1, 2, 5, 1, 1, 1], gr.READ)
    lens = [len(t) for t in gr.texts(case)]
    want_text = gr.text(case)
    s3, big = sum(lens[:3]), lens[4]
    plans = [(0, 1, 1 << 30), (0, 3, 1 << 30), (0, len(lens), 1 << 30), (0, len(lens) + 1, 1 << 30), (0, len(lens) - 1, 1 << 30),
             (0, 1 << 20, s3 - 1), (0, 1 << 20, s3), (0, 1 << 20, s3 + 1),                 # max_bytes at a block boundary -1, 0, +1
             (0, 1 << 20, big - 1), (0, 1 << 20, big), (0, 1 << 20, big + 1),               # a single block over / at the batch limit: taken alone
             (0, 1 << 20, 1), (5, 2, lens[5] + lens[6]), (5, 2, lens[5] + lens[6] - 1)]
    got = dump(gtx_dump, tmp_path, [gc.case_file(case, f, mb, mx) for f, mb, mx in plans])
    for g, (f, mb, mx) in zip(got, plans):
        want, at = [], f
        while at < len(lens):
            k = gr.cut(lens, at, mb, mx)
            assert k >= 1
            want.append(k)
            at += k
        assert g["cut"].tolist() == want, (f, mb, mx)
        assert g["cut_bytes"].tolist() == [sum(lens[a:a + k]) for a, k in zip(np.cumsum([f] + want[:-1]).tolist(), want)]
        assert g["text_cut"].tobytes() == b"".join(gr.texts(case)[f:])                      # batches concatenated: the text however it was cut
        assert g["text"].tobytes() == want_text
    assert got[5]["cut"][0] == 2 and got[6]["cut"][0] == 3 and got[7]["cut"][0] == 3
    assert got[11]["cut"].tolist() == [1] * len(lens)                                       # every block is over the limit: one each


def test_argument_errors(gtx_dump, tmp_path):
    base = gc.make_case(19, [1, 2], gr.READ)
    bad = []
    for change in ({"form": 2}, {"source": b"a\tb"}, {"source": b"a\nb"}, {"source": b"x" * 1024}):
        c = dict(base)
        c.update(change)
        bad.append(c)
    c = dict(base); c["ex_off"] = np.asarray([0, 2, 1], np.int64); bad.append(c)
    c = dict(base); c["ex_off"] = np.asarray([1, 2, 3], np.int64); bad.append(c)
    for got in dump(gtx_dump, tmp_path, [gc.case_file(c) for c in bad]):
        assert int(got["rc"][0]) != 0 and got["error"].size and "text" not in got
