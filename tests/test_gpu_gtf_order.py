"""`lr2rmats sort-gtf` and l2r_gtf_order on the GPU.  The expected rows, counts and errors everywhere are those of
tests/gtf_order_restatement.py (a dict and a ``sorted``), which tests/test_gtf_order_cpu.py holds against the output of the reference's
own script; the golden pairs of tests/golden/sort_gtf are that script's output."""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import gtf_order_restatement as gr
from tests.test_gtf_order_cpu import BAD, GOLDEN, KIND_TEXT, PAIRS, golden

pytestmark = pytest.mark.gpu

T = capi.header_define("L2R_SORT_TILE")
G = capi.header_define("L2R_GTF_TILE")
ROW_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
SAME = ["bytes", "lines", "rows", "transcripts", "heads", "names_beyond_table", "identity", "names"]


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    yield e
    e.close()


def check(eng, text, route=0):
    """Rows, counts and errors of one call against the restatement; returns the stats."""
    try:
        want, stats = gr.gtf_order(text)
    except gr.GtfDomainError as e:
        with pytest.raises(RuntimeError) as got:
            eng.gtf_order(text)
        msg = str(got.value)
        assert "line %d:" % e.line in msg and KIND_TEXT[e.kind] in msg, (msg, e.line, e.kind)
        return None
    start, length, line = eng.gtf_order(text)
    st = eng.gtf_stats()
    assert start.dtype == np.uint64 and length.dtype == np.uint32 and line.dtype == np.uint32
    np.testing.assert_array_equal(line, np.asarray([r[2] for r in want], np.uint32))
    np.testing.assert_array_equal(start, np.asarray([r[0] for r in want], np.uint64))
    np.testing.assert_array_equal(length, np.asarray([r[1] for r in want], np.uint32))
    for k in SAME:
        assert st[k] == stats[k], (k, st[k], stats[k])
    assert st["route"] == route
    return st


def padded(lines, total, final_newline=False):
    """The lines and one more exon line whose ninth column is filled so that the text has exactly ``total`` bytes."""
    head = b"".join(ln + b"\n" for ln in lines) + b"chr1\tsrc\texon\t1\t2\t.\t+\t.\t"
    fill = total - len(head) - (1 if final_newline else 0)
    assert fill >= 0, (total, len(head))
    return head + b"p" * fill + (b"\n" if final_newline else b"")


def lines_below(rng, n_bytes):
    """Shuffled transcript blocks of a little less than n_bytes in all."""
    lines, size, k = [], 0, 0
    names = [b"chr3", b"chr1", b"un_2", b"chrX"]
    while True:
        b = gr.transcript_block(rng, names[int(rng.integers(0, 4))], k)
        add = sum(len(x) + 1 for x in b)
        if size + add > n_bytes - 64:
            return lines
        lines += b
        size += add
        k += 1


# ---------------------------------------------------------------------------------------------------- row counts at the radix tile

@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_radix_tile(eng, n):
    rng = np.random.default_rng(100 + n)
    text = gr.text_of(gr.blocks_with_rows(rng, n))
    st = check(eng, text)
    assert st["rows"] == n
    if n > 64:
        assert st["identity"] == 0 and st["passes_stage2"] > 0


# ---------------------------------------------------------------------------------------------------- text-tile edges

@pytest.mark.parametrize("total", [G - 1, G, G + 1, 3 * G + 5])
def test_text_lengths_at_the_tile_without_final_newline(eng, total):
    rng = np.random.default_rng(total)
    text = padded(lines_below(rng, total - 40), total)
    assert len(text) == total and not text.endswith(b"\n")
    check(eng, text)


@pytest.mark.parametrize("at", [G - 1, G, 2 * G - 1, 2 * G])
def test_newline_at_a_tile_edge(eng, at):
    rng = np.random.default_rng(at)
    text = padded(lines_below(rng, at - 40), at + 1, final_newline=True) + gr.text_of([gr.transcript_block(rng, b"chr1", 9000 + k) for k in range(5)])
    assert text[at:at + 1] == b"\n"
    check(eng, text)


@pytest.mark.parametrize("back", [1, 3, 5, 12, 20, 28])
def test_line_head_straddles_a_tile_edge(eng, back):
    rng = np.random.default_rng(back)
    tx = gr.tx_line(b"chr2", 123456, 234567, 1) + b"\n" + gr.tx_line(b"chr2", 123460, 123470, 1, b"exon") + b"\n" + gr.tx_line(b"chr1", 5, 6, 2) + b"\n"
    text = padded(lines_below(rng, G - back - 40), G - back, final_newline=True) + tx
    assert text[G - back:].startswith(b"chr2\tsrc\ttranscript\t123456\t234567") and text[G - back - 1:G - back] == b"\n"
    check(eng, text)


def test_one_line_longer_than_two_tiles(eng):
    rng = np.random.default_rng(3)
    a = lines_below(rng, 3000)
    long_tx = gr.tx_line(b"chr1", 7, 8, 77) + b" note \"" + b"x" * (2 * G + 100) + b"\";"
    text = b"".join(ln + b"\n" for ln in a + [long_tx, gr.tx_line(b"chr1", 7, 8, 77, b"exon")] + lines_below(rng, 3000))
    st = check(eng, text)
    assert st["rows"] == st["lines"]


def test_empty_lines_comments_and_empty_text(eng):
    st = check(eng, b"\n" * (G + 1))
    assert st["lines"] == G + 1 and st["rows"] == 0
    st = check(eng, b"\n" * (G + 1) + gr.tx_line(b"chr1", 1, 2) + b"\n" * 3 + gr.tx_line(b"chr1", 1, 2, 0, b"exon"))
    assert st["lines"] == G + 5 and st["rows"] == 2
    st = check(eng, b"#a\n#b transcript\n##\ttranscript\ttranscript\t1\t2\n#")
    assert st["lines"] == 4 and st["rows"] == 0 and st["identity"] == 1
    st = check(eng, b"")
    assert st["lines"] == 0 and st["rows"] == 0 and st["identity"] == 1
    assert check(eng, b"\n")["lines"] == 1
    assert check(eng, b"x")["lines"] == 1


# ---------------------------------------------------------------------------------------------------- fields

def test_fields(eng):
    lines = [
        b"  \t chr2 \t\t src   transcript \t\t 30   40 . + . blanks everywhere",
        b"chr2 src exon 30 40 . + . a space-separated line",
        b"", b"one", b"one two", b"one two exons", b"one two exon", b"one two three four",
        b"chr1\ts\texon\t1\t2", b"chr1\ts\texons\t1\t2", b"chr1\ts\ttranscript\t10\t20", b"chr1\ts\ttranscripts\t1\t2", b"chr1\ts\tTranscript\t1\t2",
        b"chr1\ts\tprimary_transcript\t1\t2", b"chr1\ts\ttranstranscript\tx\ty", b"chr1\ts\ttranscrip\t1\t2", b"chr1\ts\ttranscriptranscript\t1\t2", b"chr1\ts\texo\t1\t2",
        b"chr1\ts\tEXON\t1\t2", b"chr1\ts\ttttranscript\t1\t2",
        b"#chr1\ts\ttranscript\t1\t2", b" #chr1\ts\ttranscript\t1\t2", b"\t#\ts\texon",
    ]
    text = b"\n".join(lines)
    st = check(eng, text)
    want_kept = {1, 2, 7, 9, 11, 12, 14, 15, 17, 20, 22, 23}
    assert set(eng.gtf_order(text)[2].tolist()) == want_kept
    assert st["transcripts"] == 3                                  # lines 1, 11 and 22 (" #chr1" is a name like any other)


# ---------------------------------------------------------------------------------------------------- numbers

def test_numbers_accepted(eng):
    text = (b"chr1\ts\ttranscript\t0\t0\nchr1\ts\ttranscript\t0000000000000000000017\t4294967295\nchr1\ts\ttranscript\t4294967295\t4294967295\n"
            b"chr1\ts\texon\t-5\t1e3\nchr1\ts\texon\t12.5\t\nchr1\ts\texon\t4294967296\t99999999999999999999999\nchr1\ts\ttranscript\t4294967295\t4294967294\n")
    st = check(eng, text)
    assert st["rows"] == 7 and st["identity"] == 0


@pytest.mark.parametrize("name", sorted(BAD))
def test_numbers_rejected(eng, name):
    text, line, kind = BAD[name]
    assert check(eng, text) is None
    # ... and behind many good lines, in another wave and another workgroup of the fields kernel
    rng = np.random.default_rng(1)
    pre = gr.text_of(gr.blocks_with_rows(rng, 700))
    mid = text if text.endswith(b"\n") else text + b"\n"
    assert check(eng, pre + mid + pre) is None
    with pytest.raises(RuntimeError) as e:
        eng.gtf_order(pre + mid + pre)
    assert "line %d:" % (700 + line) in str(e.value)


def test_two_bad_lines_in_one_wave_and_in_two(eng):
    good = gr.tx_line(b"chr1", 1, 2)
    for gap in (1, 70, 300):
        lines = [good] * 5 + [b"chr1\ts\ttranscript\t1\t1e3"] + [good] * gap + [b"chr1\ts\ttranscript\t-5\t2"]
        with pytest.raises(RuntimeError) as e:
            eng.gtf_order(b"\n".join(lines))
        assert "line 6:" in str(e.value) and "the end of" in str(e.value)
    # after an error the context orders the next text as if nothing had happened
    check(eng, golden("quirk", "in"))


# ---------------------------------------------------------------------------------------------------- names

def test_names_that_are_prefixes_of_each_other(eng):
    rng = np.random.default_rng(8)
    names = [b"chr1_random", b"chr10", b"chr", b"chr1", b"chr1_random", b"chr", b"chr10", b"chr1", b"c", b"n" * 300, b"c", b"n" * 299 + b"m", b"n" * 300]
    blocks = [gr.transcript_block(rng, nm, k, hi=50) for k, nm in enumerate(names * 3)]
    st = check(eng, gr.text_of(blocks))
    assert st["names"] == 7 and st["names_beyond_table"] == 5


def test_every_table_name_behind_unknown_ones(eng):
    rng = np.random.default_rng(9)
    table = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY", b"chrM"]
    names = [b"zz", b"aa", b"chr23", b"chr0", b"chr01", b"chrx", b"Chr1", b"chrMT", b"chr1 "[:4] + b"0"] + [table[int(i)] for i in rng.permutation(25)] + [b"aa", b"zz"]
    blocks = [gr.transcript_block(rng, nm, k, hi=30) for k, nm in enumerate(names)]
    st = check(eng, gr.text_of(blocks))
    assert st["names"] == 8 + 25 and st["names_beyond_table"] == 8      # "chr10" is a table name


def test_names_alternate_on_every_transcript(eng):
    rng = np.random.default_rng(10)
    n = T + 5
    blocks = [gr.transcript_block(rng, (b"u_first", b"u_second", b"chr1")[k % 3], k, max_exons=1) for k in range(n)]
    st = check(eng, gr.text_of(blocks))
    assert st["heads"] == n and st["transcripts"] == n and st["names"] == 3


def test_unknown_name_first_seen_on_an_exon_line(eng):
    text = (b"late\ts\texon\t1\t2\nchr9\ts\ttranscript\t50\t60\nlate\ts\texon\t50\t60\nother\ts\ttranscript\t5\t6\nlate\ts\ttranscript\t1\t2\nchr9\ts\ttranscript\t40\t60\n")
    st = check(eng, text)
    assert st["names_beyond_table"] == 2
    assert eng.gtf_order(text)[2].tolist() == [1, 6, 2, 3, 4, 5]


# ---------------------------------------------------------------------------------------------------- order

def test_equal_chromosome_and_start_with_descending_end(eng):
    lines = [gr.tx_line(b"chr4", 1000, 5000 - k, k) for k in range(300)] + [gr.tx_line(b"chr4", 1000, 4800, 999, b"exon")]
    st = check(eng, b"\n".join(lines) + b"\n")
    assert st["passes_stage1"] > 0 and st["passes_stage2"] == 0    # c << 32 | s is one value: every byte of stage 2 is constant


def test_more_than_a_tile_of_identical_lines(eng):
    same = gr.tx_line(b"chr1", 77, 88, 5)
    st = check(eng, b"\n".join([same] * (T + 3)) + b"\n")
    assert st["identity"] == 1
    st = check(eng, b"\n".join([gr.tx_line(b"chr2", 1, 2)] + [same] * (T + 3) + [gr.tx_line(b"chr1", 77, 87)]) + b"\n")
    assert st["identity"] == 0
    assert eng.gtf_order(b"\n".join([gr.tx_line(b"chr2", 1, 2)] + [same] * 5) + b"\n")[2].tolist() == [2, 3, 4, 5, 6, 1]


def test_exons_before_the_first_transcript(eng):
    rng = np.random.default_rng(12)
    pre = [gr.tx_line(b"chr9", 100 - k, 200, k, b"exon") for k in range(70)]
    text = b"\n".join(pre) + b"\n" + gr.text_of(gr.blocks_with_rows(rng, 500))
    check(eng, text)
    assert eng.gtf_order(text)[2][:70].tolist() == list(range(1, 71))


def test_input_in_order_runs_no_sort(eng, monkeypatch):
    rng = np.random.default_rng(13)
    text = gr.sort_gtf(gr.text_of(gr.blocks_with_rows(rng, 2 * T + 9)))
    monkeypatch.setenv("L2R_SORT_TIMING", "1")
    st = check(eng, text)
    assert st["identity"] == 1 and st["passes_stage1"] == 0 and st["passes_stage2"] == 0
    assert st["key kernels + radix passes"] == 0 and st["k_gtf_compose"] == 0
    assert st["k_gtf_count + k_gtf_starts"] > 0 and st["k_gtf_fields"] > 0
    assert eng.gtf_order(text)[2].tolist() == list(range(1, 2 * T + 10))


@pytest.mark.parametrize("in_order", [False, True])
def test_every_pass_forced(eng, monkeypatch, in_order):
    rng = np.random.default_rng(14)
    text = gr.text_of(gr.blocks_with_rows(rng, T + 100))
    if in_order:
        text = gr.sort_gtf(text)
    plain = [x.copy() for x in eng.gtf_order(text)]
    monkeypatch.setenv("L2R_SORT_FORCE", "1")
    st = check(eng, text)
    assert st["passes_stage1"] == 8 and st["passes_stage2"] == 8 and st["identity"] == int(in_order)
    for a, b in zip(plain, eng.gtf_order(text)):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------------- routes

@pytest.mark.parametrize("name", PAIRS)
def test_host_route_gives_the_same_rows(eng, monkeypatch, name):
    text = golden(name, "in")
    dev = [x.copy() for x in eng.gtf_order(text)]
    assert eng.gtf_stats()["route"] == 0
    monkeypatch.setenv("L2R_GTF_ROUTE", "host")
    check(eng, text, route=1)
    for a, b in zip(dev, eng.gtf_order(text)):
        np.testing.assert_array_equal(a, b)
    assert check(eng, BAD["two_bad_lines"][0], route=1) is None


def test_argument_checks(eng):
    import ctypes as C
    n = C.c_int64(0)
    lib = eng.lib
    assert lib.l2r_gtf_order(eng.ctx, C.byref(capi.CGtfText(-1, None)), C.byref(n)) != 0
    assert lib.l2r_gtf_order(eng.ctx, C.byref(capi.CGtfText(9, None)), C.byref(n)) != 0
    assert lib.l2r_gtf_order(eng.ctx, C.byref(capi.CGtfText(0, None)), C.byref(n)) == 0 and n.value == 0
    text = golden("quirk", "in")
    start, length, line = eng.gtf_order(text)
    rows = capi.CGtfRows(len(line) - 1, 7, start.ctypes.data, length.ctypes.data, line.ctypes.data)
    keep = line.copy()
    assert lib.l2r_gtf_rows_out(eng.ctx, C.byref(rows)) != 0 and rows.n == 7      # cap < n fails and writes nothing
    np.testing.assert_array_equal(line, keep)


# ---------------------------------------------------------------------------------------------------- CLI

@pytest.mark.parametrize("name", PAIRS)
def test_cli_reproduces_the_golden(tmp_path, name):
    src = os.path.join(GOLDEN, name + ".in.gtf")
    r = hostlib.run_cli(["sort-gtf", src])
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden(name, "out")
    _, stats = gr.gtf_order(golden(name, "in"))
    assert (b"Sorted GTF: %d of %d lines in %d transcripts, %d chromosomes" % (stats["rows"], stats["lines"], stats["transcripts"], stats["names"])) in r.stderr
    out = str(tmp_path / "o.gtf")
    r = hostlib.run_cli(["sort-gtf", "-o", out, src])
    assert r.returncode == 0 and r.stdout == b""
    with open(out, "rb") as fh:
        assert fh.read() == golden(name, "out")
    assert hostlib.run_cli(["sort-gtf-check", out]).returncode == 0


def test_cli_several_inputs_and_domain_error(tmp_path):
    r = hostlib.run_cli(["sort-gtf", os.path.join(GOLDEN, "two_files.a.gtf"), os.path.join(GOLDEN, "two_files.b.gtf")])
    assert r.returncode == 0 and r.stdout == golden("two_files", "out")
    bad = str(tmp_path / "bad.gtf")
    with open(bad, "wb") as fh:
        fh.write(BAD["two_bad_lines"][0])
    r = hostlib.run_cli(["sort-gtf", bad])
    assert r.returncode == 1 and b"line 3:" in r.stderr and r.stdout == b""
