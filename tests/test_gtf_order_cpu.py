"""`sort-gtf`, the parts that need no GPU: tests/gtf_order_restatement.py against the golden pairs the reference's own script wrote
(tests/golden/sort_gtf), the argument checks and the exact host routine of l2r_gtf_order as a stand-alone program under ASan + UBSan
(tests/gtf_dump.hip, `make -C lr2rmats_amd/csrc gtf-dump`) against the restatement, the row writer (h_gtf_write_rows),
`sort-gtf-check`, and -- where the reference's script, awk and sort are at hand -- random texts through that script itself."""
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import gtf_order_restatement as gr
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GTF_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "gtf_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sort_gtf")
PAIRS = sorted(os.path.basename(p)[:-len(".in.gtf")] for p in glob.glob(os.path.join(GOLDEN, "*.in.gtf")))
REF_SCRIPT = "/root/reference/src/sort_gtf.sh"
KIND_TEXT = {"NUL": "a NUL byte", "fields": "fewer than five fields", "start": "the start of", "end": "the end of"}


def golden(name, side):
    with open(os.path.join(GOLDEN, "%s.%s.gtf" % (name, side)), "rb") as fh:
        return fh.read()


def test_the_golden_pairs_are_there():
    assert {"toy", "quirk", "two_files", "synth300"} <= set(PAIRS)
    assert golden("two_files", "a") + golden("two_files", "b") == golden("two_files", "in") and not golden("two_files", "a").endswith(b"\n")
    with open(os.path.join(ROOT, "tests", "golden", "toy", "original.gtf"), "rb") as fh:
        assert fh.read() == golden("toy", "in")


@pytest.mark.parametrize("name", PAIRS)
def test_restatement_equals_the_reference_output(name):
    assert gr.sort_gtf(golden(name, "in")) == golden(name, "out")


def test_toy_output_is_its_own_lines_in_file_order():
    text = golden("toy", "in")
    rows, stats = gr.gtf_order(text)
    assert stats["identity"] == 1 and [r[2] for r in rows] == sorted(r[2] for r in rows)
    want = [ln for ln in text.split(b"\n") if ln.split(b"\t")[2:3] in ([b"transcript"], [b"exon"])]
    assert golden("toy", "out") == b"".join(ln + b"\n" for ln in want)


# ---------------------------------------------------------------------------------------------------- the host routine (gtf_dump)

@pytest.fixture(scope="module")
def gtf_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "gtf-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return GTF_DUMP


def _dump(exe, tmp_path, texts):
    """The dumps of several texts from one run of the program."""
    args = []
    for k, t in enumerate(texts):
        src, dst = str(tmp_path / ("text%d.gtf" % k)), str(tmp_path / ("rows%d.bin" % k))
        with open(src, "wb") as fh:
            fh.write(t)
        args += [src, dst]
    env = dict(os.environ)
    env.update(SAN_ENV)
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    for m in MARKS:
        assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
    return [_read_dump(a) for a in args[1::2]]


def _check(got, text):
    try:
        rows, stats = gr.gtf_order(text)
    except gr.GtfDomainError as e:
        assert int(got["rc"][0]) != 0
        msg = bytes(got["error"]).decode()
        assert "line %d:" % e.line in msg and KIND_TEXT[e.kind] in msg, (msg, e.line, e.kind)
        return
    assert int(got["rc"][0]) == 0, bytes(got.get("error", b"")).decode()
    assert list(zip(got["start"].tolist(), got["len"].tolist(), got["line"].tolist())) == rows
    c = got["counts"].tolist()
    assert c[:5] == [stats["lines"], stats["transcripts"], stats["heads"], stats["names_beyond_table"], stats["names"]]
    assert c[5] == (gr.first_descent(text) or 0) and (c[5] == 0) == (stats["identity"] == 1)
    assert len(got["head_rank"]) == stats["heads"]


def test_host_routine_on_the_goldens(gtf_dump, tmp_path):
    texts = [golden(n, "in") for n in PAIRS]
    for got, text, name in zip(_dump(gtf_dump, tmp_path, texts), texts, PAIRS):
        _check(got, text)
        rows = list(zip(got["start"].tolist(), got["len"].tolist(), got["line"].tolist()))
        assert gr.write_rows(text, rows) == golden(name, "out")


EDGE_TEXTS = [b"", b"\n", b"\n\n\n", b"#only\n#comments", b"x", b"chr1\ts\ttranscript\t1\t2", b"chr1\ts\texon\t1\t2\nchr1\ts\ttranscript\t1\t2\n",
              b"chr2\ts\ttranscript\t5\t6\nchr1\ts\ttranscript\t5\t6", b"a b exon\n\n\na b exon"]


def test_host_routine_on_edges_and_random_texts(gtf_dump, tmp_path):
    rng = np.random.default_rng(2024)
    texts = EDGE_TEXTS + [gr.random_text(rng, int(rng.integers(1, 40))) for _ in range(300)]
    dumps = _dump(gtf_dump, tmp_path, texts)
    assert len(dumps) == len(texts)
    for got, text in zip(dumps, texts):
        _check(got, text)


BAD = {
    "minus": (b"chr1\ts\ttranscript\t-5\t9\n", 1, "start"),
    "exponent": (b"chr1\ts\ttranscript\t1\t1e3\n", 1, "end"),
    "fraction": (b"chr1\ts\ttranscript\t12.5\t20\n", 1, "start"),
    "too_large": (b"chr1\ts\ttranscript\t1\t4294967296\n", 1, "end"),
    "many_digits": (b"chr1\ts\ttranscript\t1\t" + b"9" * 40 + b"\n", 1, "end"),
    "no_end": (b"chr1\ts\ttranscript\t7\n", 1, "fields"),
    "no_start": (b"chr1\ts\ttranscript", 1, "fields"),
    "two_bad_lines": (b"chr1\ts\texon\tx\ty\n#c\nchr1\ts\ttranscript\t1\tx\nchr1\ts\ttranscript\tx\t1\n", 3, "end"),
    "nul_first": (b"chr1\ts\tgene\t\0\n\nchr1\ts\ttranscript\tx\t1\n", 1, "NUL"),
    "nul_behind_a_bad_line": (b"chr1\ts\ttranscript\tx\t1\nab\0\n", 1, "start"),
    "nul_on_the_bad_line": (b"\nchr1\ts\ttranscript\tx\t1\t\0\n", 2, "NUL"),
    "nul_last_byte": (b"chr1\ts\ttranscript\t1\t2\n\0", 2, "NUL"),
}


def test_domain_errors_name_the_smallest_bad_line(gtf_dump, tmp_path):
    names = sorted(BAD)
    for got, name in zip(_dump(gtf_dump, tmp_path, [BAD[n][0] for n in names]), names):
        text, line, kind = BAD[name]
        with pytest.raises(gr.GtfDomainError) as e:
            gr.gtf_order(text)
        assert (e.value.line, e.value.kind) == (line, kind), name
        _check(got, text)
    ok = b"chr1\ts\ttranscript\t0\t4294967295\nchr1\ts\texon\t-5\t1e3\nchr1\ts\ttranscript\t000123\t0\n"
    assert len(gr.gtf_order(ok)[0]) == 3


def test_argument_checks_through_the_library():
    lib = capi.load_library()
    import ctypes as C
    line = C.c_int64(0)
    assert lib.l2r_gtf_check(C.byref(capi.CGtfText(-1, None)), C.byref(line), None) < 0 and b"-1 bytes" in lib.l2r_last_error()
    assert lib.l2r_gtf_check(C.byref(capi.CGtfText(5, None)), C.byref(line), None) < 0 and b"null text" in lib.l2r_last_error()
    assert lib.l2r_gtf_check(C.byref(capi.CGtfText(0, None)), C.byref(line), None) == 0


# ---------------------------------------------------------------------------------------------------- h_gtf_write_rows

@pytest.mark.parametrize("name", PAIRS)
def test_writer_gives_the_golden_bytes(tmp_path, name):
    text = golden(name, "in")
    rows, _ = gr.gtf_order(text)
    out = str(tmp_path / "out.gtf")
    hostlib.gtf_write_rows(text, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], out)
    with open(out, "rb") as fh:
        assert fh.read() == golden(name, "out")


def test_writer_columns(tmp_path):
    text = b"a\tb\tc\td\te\tf\tg\nno tab at all\n1\t2\t3\t4\t5\t6\t7\t8\t9\t10\t11\t12\n\n\t\t\t\t\t\t\t\t\t\t\nx\t\t\t\t\t\t\t\ty"
    rows = [(p, n, k + 1) for k, (p, n) in enumerate(gr.split_lines(text))]
    out = str(tmp_path / "out.gtf")
    hostlib.gtf_write_rows(text, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], out)
    with open(out, "rb") as fh:
        got = fh.read()
    assert got == gr.write_rows(text, rows)
    assert got == b"a\tb\tc\td\te\tf\tg\t\t\nno tab at all" + b"\t" * 8 + b"\n1\t2\t3\t4\t5\t6\t7\t8\t9\n" + b"\t" * 8 + b"\n" + b"\t" * 8 + b"\nx" + b"\t" * 8 + b"y\n"
    hostlib.gtf_write_rows(text, [], [], [], out)
    assert os.path.getsize(out) == 0
    with pytest.raises(OSError):
        hostlib.gtf_write_rows(text, [len(text) - 1], [2], [1], out)


# ---------------------------------------------------------------------------------------------------- sort-gtf-check

@pytest.mark.parametrize("name", PAIRS)
def test_check_command_on_the_goldens(name):
    r = hostlib.run_cli(["sort-gtf-check", os.path.join(GOLDEN, name + ".out.gtf")])
    assert r.returncode == 0 and r.stdout.startswith(b"GTF sorted:"), (r.stdout, r.stderr)
    text = golden(name, "in")
    bad = gr.first_descent(text)
    r = hostlib.run_cli(["sort-gtf-check", os.path.join(GOLDEN, name + ".in.gtf")])
    if bad is None:
        assert name == "toy" and r.returncode == 0
    else:
        assert r.returncode == 1 and (b"line %d " % bad) in r.stdout, (r.stdout, bad)
    assert capi.gtf_check(text)[:2] == (bad is None, bad or 0)
    _, stats = gr.gtf_order(text)
    assert capi.gtf_check(text)[2] == [stats["lines"], stats["rows"], stats["transcripts"], stats["names"]]


def test_check_command_usage_and_domain(tmp_path):
    assert hostlib.run_cli(["sort-gtf-check"]).returncode == 2
    assert hostlib.run_cli(["sort-gtf-check", "a", "b"]).returncode == 2
    assert b"sort-gtf-check <in.gtf>" in hostlib.run_cli(["sort-gtf-check", "-x"]).stderr
    assert hostlib.run_cli(["sort-gtf"]).returncode == 2 and b"sort-gtf [option]" in hostlib.run_cli(["sort-gtf"]).stderr
    r = hostlib.run_cli([])
    assert b" sort-gtf " in r.stderr and b" sort-gtf-check " in r.stderr
    p = str(tmp_path / "bad.gtf")
    with open(p, "wb") as fh:
        fh.write(BAD["two_bad_lines"][0])
    r = hostlib.run_cli(["sort-gtf-check", p])
    assert r.returncode == 1 and b"line 3:" in r.stderr


# ---------------------------------------------------------------------------------------------------- the reference's script itself

@pytest.mark.skipif(not (os.path.exists(REF_SCRIPT) and shutil.which("awk") and shutil.which("sort") and shutil.which("bash")),
                    reason="the reference's script, awk or sort is not at hand")
def test_restatement_equals_the_script_on_random_texts(tmp_path):
    rng = np.random.default_rng(77)
    env = dict(os.environ)
    env["LC_ALL"] = "C"
    src, dst = str(tmp_path / "in.gtf"), str(tmp_path / "out.gtf")
    for k in range(50):
        text = gr.random_text(rng, int(rng.integers(1, 60)))
        if not text.endswith(b"\n"):
            text += b"\n" if k % 2 else b""
        with open(src, "wb") as fh:
            fh.write(text)
        r = subprocess.run(["bash", REF_SCRIPT, src, dst], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr
        with open(dst, "rb") as fh:
            assert fh.read() == gr.sort_gtf(text), text
