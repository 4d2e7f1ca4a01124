"""The GTF block of `bam2gtf` / `unique-gtf` on the GPU: l2r_gtftext_* (k_gtx_measure in both forms, k_scan_u32, k_gtx_write on the LDS and
on the direct path) and the two commands against tests/gtf_text_restatement.py, at the edges of the block count, the exon count, the tile
text, the digits, the names and the batch cut."""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import gtf_text_cases as gc
from tests import gtf_text_restatement as gr
from tests.test_gtf_text_cpu import big_case, error_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "toy")
HAND = os.path.join(ROOT, "tests", "golden", "hand")
TILE = capi.header_define("L2R_GTX_TILE")
LDS = capi.header_define("L2R_GTX_LDS_BYTES")
FORMS = [gr.PLAIN, gr.READ]


@pytest.fixture(scope="module")
def eng():
    os.environ["L2R_CHECK"] = "1"                       # (read when the context is made: the guard behind the text is filled and looked at)
    try:
        e = capi.Engine(0)
    finally:
        del os.environ["L2R_CHECK"]
    yield e
    e.close()


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at %d: %r / %r" % (len(got), len(want), k, got[max(0, k - 60):k + 60], want[max(0, k - 60):k + 60])


def check(e, case, max_blocks=1 << 20, max_bytes=1 << 30, route=0):
    """The engine's text of a case against the restatement; route and guard; the stats of the last batch."""
    want = gr.texts(case)
    text, n_lines, n_bytes, st = gc.engine_text(e, case, max_blocks, max_bytes)
    whole = b"".join(want)
    assert text == whole, first_difference(text, whole)
    assert (n_lines, n_bytes) == (whole.count(b"\n"), len(whole))
    assert st["blocks"] == case["m"] and st["route"] == route and st["guard_intact"] == 1
    return st


@pytest.fixture(scope="module")
def mixed():
    """3 x TILE + 17 transcripts of both forms, made once."""
    rng = np.random.default_rng(7)
    exons = rng.choice([1, 1, 2, 3, 4, 6, 9, 14, 25], 3 * TILE + 17)
    return {f: gc.make_case(70 + f, exons, f, empty_names=0.2) for f in FORMS}


def head(case, n):
    return gc.with_selection(case, np.arange(n))


# ---------------------------------------------------------------------------------------------------- the table of the issue

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_block_counts(eng, mixed, n):
    for f in FORMS:
        st = check(eng, head(mixed[f], n))
        if n:
            assert st["tiles_lds"] + st["tiles_direct"] == (n + TILE - 1) // TILE and st["batches"] == 1


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 63, 64, 65, 129, 300])
def test_exons_per_block_in_both_forms(eng, monkeypatch, k):
    for f in FORMS:
        case = gc.with_selection(gc.make_case(100 + k, [k] * 7, f), None, 3, overrides=(f == gr.READ))
        for form in (0, 1):
            monkeypatch.setenv("L2R_GTX_WAVE", str(form))
            assert check(eng, case)["wave_form"] == form
        monkeypatch.delenv("L2R_GTX_WAVE")
        assert check(eng, case)["wave_form"] == (1 if k > 32 else 0)    # more than 32 exons per block on average: one wave per block


def test_the_form_follows_the_selection_average(eng):
    case = gc.make_case(5, [1, 300, 1, 1], gr.READ)
    assert check(eng, gc.with_selection(case, [0, 2, 3]))["wave_form"] == 0
    assert check(eng, gc.with_selection(case, [1, 1, 0]))["wave_form"] == 1
    assert check(eng, gc.with_selection(gc.make_case(6, [32, 33, 31], gr.PLAIN), None))["wave_form"] == 0      # exactly 32 on average
    assert check(eng, gc.with_selection(gc.make_case(6, [32, 33, 32], gr.PLAIN), None))["wave_form"] == 1


@pytest.mark.parametrize("at", [0, TILE // 2, TILE - 1])
def test_one_long_block_among_short_ones(eng, monkeypatch, at):
    exons = [1] * TILE
    exons[at] = 300
    for f in FORMS:
        case = gc.make_case(200 + at, exons + [2, 300, 1], f)
        for form in (0, 1):
            monkeypatch.setenv("L2R_GTX_WAVE", str(form))
            check(eng, case)


def test_digit_edges(eng, monkeypatch):
    E = gc.EDGES
    for f in FORMS:
        c = gc.make_case(5, [1] * len(E) + [2] * len(E), f)
        c["xs"][:len(E)] = E
        c["xe"][:len(E)] = E
        c["xs"][len(E)::2], c["xe"][len(E)::2], c["xs"][len(E) + 1::2], c["xe"][len(E) + 1::2] = 0, E, E, 2147483647
        d = gc.with_selection(gc.make_case(6, [3] * len(E), f), None)
        d["start"], d["end"], d["cov"] = np.asarray(E, np.int32), np.asarray(E[::-1], np.int32), np.asarray(E, np.int32)
        for form in (0, 1):
            monkeypatch.setenv("L2R_GTX_WAVE", str(form))
            check(eng, c)
            check(eng, d)


@pytest.mark.parametrize("name_len", [0, 1, 254])
@pytest.mark.parametrize("source", [b"", b"s" * 1023])
def test_names_and_source(eng, name_len, source):
    for f in FORMS:
        check(eng, gc.make_case(31, [1, 3, 2, 40, 1], f, name_len=(name_len, name_len), source=source))


def test_aliasing_id_columns(eng):
    for f in FORMS:
        c = gc.make_case(33, [2, 1, 5, 3], f)
        c["tids"] = c["gid"]
        if f == gr.READ:
            c["gname"] = c["tname"] = c["gid"]
        check(eng, c)


def test_strand_and_exon_order(eng):
    for f in FORMS:
        c = gc.make_case(35, [3, 3], f)
        c["rev"][:] = [1, 0]
        text = gc.engine_text(eng, c)[0]
        assert text == gr.text(c)
        firsts = [int(ln.split(b"\t")[3]) for ln in text.splitlines() if b"\texon\t" in ln][:3]
        assert firsts == sorted(firsts, reverse=(f == gr.READ)) and len(set(firsts)) == 3


def test_selections(eng, mixed):
    rng = np.random.default_rng(9)
    for f in FORMS:
        base, n = mixed[f], len(mixed[f]["tid"])
        for sel in (None, rng.permutation(n), rng.integers(0, n, 2 * TILE + 5), np.zeros(TILE + 1, np.int64) + 3, []):
            for over in (False, True):
                check(eng, gc.with_selection(base, sel, 9, overrides=over))


def tile_text_case(form, target):
    """TILE blocks of two exons whose text has exactly ``target`` bytes, and a short tile behind (it starts off a 16-byte boundary)."""
    base = gc.make_case(41, [2] * (TILE + 3), form, name_len=(1, 1), source=b"x", refs=(b"chr1",))
    base["table"] += b"\0"                              # two names only, also in form READ
    base["gname"] = base["tname"] = np.full(TILE + 3, len(base["table"]) - 1, np.uint32)
    base["xs"][0::2], base["xe"][0::2], base["xs"][1::2], base["xe"][1::2] = 1000, 2000, 300000000, 400000000
    per = len(gr.block_text(base, 0))
    assert all(len(gr.block_text(base, q)) == per for q in range(TILE)) and per * TILE < target
    lines = 3 * TILE
    pad = (target - per * TILE) // lines                # the source string pads every line alike ...
    base["source"] = b"x" * (1 + pad)
    rest = target - (per + 3 * pad) * TILE
    assert 0 <= rest < lines
    for q in range(TILE):                               # ... and the digits of an inner exon end, which one line prints, give the last bytes
        k = min(5, rest)
        base["xe"][2 * q] = 2000 * 10 ** k
        rest -= k
    assert rest == 0 and sum(len(gr.block_text(base, q)) for q in range(TILE)) == target
    return base


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_text_at_the_lds_edge(eng, delta):
    for f in FORMS:
        case = tile_text_case(f, LDS + delta)
        assert (LDS + delta) % 16 != 0 or delta == 0
        st = check(eng, case)
        assert (st["tiles_lds"], st["tiles_direct"]) == ((2, 0) if delta <= 0 else (1, 1))


def tile_offset_case(r):
    """2 x TILE + 1 PLAIN blocks of two exons; the gene name of block 0 is lengthened until the first tile's bytes are r modulo 16."""
    case = gc.make_case(47, [2] * (2 * TILE + 1), gr.PLAIN, name_len=(4, 4))
    first = sum(len(gr.block_text(case, q)) for q in range(TILE))
    k = (r - first) * 11 % 16                           # the name stands once in each of the block's three lines: 3 k bytes more, and 3 * 11 = 33
    case["table"] = bytes(case["table"]) + b"G" * (4 + k) + b"\0"
    case["gid"][0] = len(case["table"]) - (4 + k) - 1
    return case


def test_tile_offsets_take_every_residue(eng):
    """The stream-out of k_gtx_write (text_stream_out) with the second tile's span beginning at every offset modulo 16."""
    seen = set()
    for r in range(16):
        case = tile_offset_case(r)
        second = sum(len(t) for t in gr.texts(case)[:TILE])          # where the second tile's span begins
        assert second % 16 == r
        seen.add(second % 16)
        st = check(eng, case)
        assert (st["tiles_lds"], st["tiles_direct"], st["batches"]) == (3, 0, 1)
    assert seen == set(range(16))


def test_oversized_tiles_take_the_direct_path(eng, monkeypatch):
    for f in FORMS:
        case = gc.make_case(43, [300] * 3 + [1] * (TILE - 3) + [2] * 5, f, name_len=(100, 254))
        for form in (0, 1):
            monkeypatch.setenv("L2R_GTX_WAVE", str(form))
            st = check(eng, case)
            assert (st["tiles_lds"], st["tiles_direct"]) == (1, 1)


def test_batch_invariance(eng, mixed):
    for f in FORMS:
        case = gc.with_selection(mixed[f], None, 11, overrides=(f == gr.READ))
        lens = [len(t) for t in gr.texts(case)]
        small = head(case, 40)
        assert check(eng, small, max_blocks=1)["batches"] == 40
        assert check(eng, case, max_blocks=3)["batches"] == (case["m"] + 2) // 3
        assert check(eng, case, max_blocks=TILE)["batches"] == (case["m"] + TILE - 1) // TILE
        for max_bytes in (sum(lens) // 2, 5 * max(lens), max(lens), min(lens), 1):
            st = check(eng, small if max_bytes <= max(lens) else case, max_bytes=max_bytes)
            assert st["batches"] >= 2
        assert check(eng, small, max_bytes=1)["batches"] == 40           # down to one block each


def test_lines_takes_what_the_cut_says(eng, mixed):
    case = head(mixed[gr.READ], 50)
    want = gr.texts(case)
    lens = [len(t) for t in want]
    gc.engine_rows(eng, case)
    gc.engine_blocks(eng, case)
    for first, mb, mx in ((0, 7, 1 << 30), (10, 1 << 20, sum(lens[10:13])), (10, 1 << 20, sum(lens[10:13]) - 1), (10, 1 << 20, sum(lens[10:13]) + 1), (49, 5, 1)):
        k, text = eng.gtftext_lines(first, mb, mx)
        assert k == gr.cut(lens, first, mb, mx) and text == b"".join(want[first:first + k])
        st = eng.gtftext_stats()
        assert st["lines"] == text.count(b"\n") and st["bytes"] == len(text)
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(50)
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(0, 0)


def test_out_needs_room(eng, mixed):
    case = head(mixed[gr.PLAIN], 9)
    want = gr.text(case)
    gc.engine_rows(eng, case)
    gc.engine_blocks(eng, case)
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(0, cap=len(want) - 1)
    buf = np.zeros(len(want), np.uint8)
    eng._chk(eng.lib.l2r_gtftext_out(eng.ctx, buf.ctypes.data, len(want)))
    assert buf.tobytes() == want


@pytest.mark.parametrize("form", FORMS)
def test_every_domain_error(eng, monkeypatch, form):
    good = gc.make_case(51, [2, 1], form)
    for wave in (0, 1):
        monkeypatch.setenv("L2R_GTX_WAVE", str(wave))
        for case, block, kind in error_cases(form) + [(big_case(form), 1, "big")]:
            gc.engine_rows(eng, case)
            with pytest.raises(capi.L2RError) as e:
                gc.engine_blocks(eng, case)
            assert "rc=-1:" in str(e.value) and "block %d:" % block in str(e.value) and gr.KIND_TEXT[kind] in str(e.value), (kind, block, str(e.value))
            with pytest.raises(capi.L2RError) as e:          # nothing was written and nothing can be fetched
                eng.gtftext_lines(0)
            assert "rc=-1:" not in str(e.value)
            check(eng, good)                                 # ... and the next good call works


def test_order_of_calls(mixed):
    case = head(mixed[gr.PLAIN], 3)
    e = capi.Engine(0)
    calls = [lambda: e.gtftext_rows(case["tid"], case["rev"], case["ex_off"], case["xs"], case["xe"], case["table"], case["gid"], case["tids"]),
             lambda: gc.engine_blocks(e, case), lambda: e.gtftext_lines(0)]
    for call in calls:
        with pytest.raises(capi.L2RError) as err:
            call()
        assert "rc=-1:" not in str(err.value)
    e.gtftext_begin(case["refs"], case["source"], case["form"])
    for call in calls[1:]:
        with pytest.raises(capi.L2RError):
            call()
    calls[0]()
    with pytest.raises(capi.L2RError):
        calls[2]()
    with pytest.raises(capi.L2RError):                       # a bad source string
        e.gtftext_begin(case["refs"], b"a\tb", 0)
    with pytest.raises(capi.L2RError):                       # ... leaves no begin behind
        calls[0]()
    e.close()


def test_route_host_gives_the_same_bytes(eng, monkeypatch, mixed):
    monkeypatch.setenv("L2R_GTX_ROUTE", "host")
    for f in FORMS:
        check(eng, gc.with_selection(mixed[f], None, 13, overrides=(f == gr.READ)), route=1)
        check(eng, head(mixed[f], 40), max_blocks=3, route=1)
    for case, block, kind in error_cases(gr.READ)[:6]:
        gc.engine_rows(eng, case)
        with pytest.raises(capi.L2RError) as e:
            gc.engine_blocks(eng, case)
        assert "rc=-1:" in str(e.value) and "block %d:" % block in str(e.value) and gr.KIND_TEXT[kind] in str(e.value)


# ---------------------------------------------------------------------------------------------------- the chains of a run

@pytest.fixture(scope="module")
def run_set():
    anno = synth.make_annotation(3000, 61, nchr=3)
    reads = synth.make_reads(anno, 700, 6, 61)
    return reads


def run_reads(e, reads):
    e.set_params(capi.default_params())
    e.set_outputs(capi.WANT_RESULTS)
    e.set_annotation([], [], [], [], [0], [], [])
    e.set_junctions(None)
    e.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    e.run()
    e.sync()


def test_the_chains_of_a_run_where_they_lie(eng, monkeypatch, run_set):
    reads = run_set
    run_reads(eng, reads)
    res = eng.download()
    n = reads.n
    assert int((res.info >> 8).min()) >= 1 and int(res.ex_off[-1]) > n
    table, ids = gr.pack_table([reads.qname(i).encode() for i in range(n)])
    ids = np.asarray(ids, np.uint32)
    refs = [c.encode() for c in reads.chrom_names]
    case = {"form": gr.PLAIN, "source": b"lr2rmats", "refs": refs, "tid": reads.tid, "rev": reads.rev, "ex_off": res.ex_off, "xs": res.ex_start[:int(res.ex_off[-1])],
            "xe": res.ex_end[:int(res.ex_off[-1])], "table": table, "gid": ids, "tids": ids, "gname": ids, "tname": ids, "sel": None, "start": None, "end": None, "cov": None, "m": n}
    want = gr.text(case)
    for wave in (None, 0, 1):
        if wave is not None:
            monkeypatch.setenv("L2R_GTX_WAVE", str(wave))
        eng.gtftext_begin(refs, b"lr2rmats", gr.PLAIN)
        eng.gtftext_rows(reads.tid, reads.rev, None, None, None, table, ids, ids)
        assert eng.gtftext_blocks(n) == (want.count(b"\n"), len(want))
        got = eng.gtftext_all(n, max_blocks=TILE + 1)
        assert got == want, first_difference(got, want)
        st = eng.gtftext_stats()
        assert st["route"] == 0 and st["guard_intact"] == 1
    monkeypatch.delenv("L2R_GTX_WAVE")
    assert check(eng, case)["route"] == 0                    # the same rows uploaded from l2r_download's arrays
    # form READ over the same chains with a selection and overrides; the host route fetches the chains itself
    sel = np.random.default_rng(3).integers(0, n, 300)
    rcase = gc.with_selection(dict(case, form=gr.READ), sel, 5, overrides=True)
    for route in (0, 1):
        if route:
            monkeypatch.setenv("L2R_GTX_ROUTE", "host")
        eng.gtftext_begin(refs, b"lr2rmats", gr.READ)
        eng.gtftext_rows(reads.tid, reads.rev, None, None, None, table, ids, ids, ids, ids)
        gc.engine_blocks(eng, rcase)
        assert eng.gtftext_all(rcase["m"]) == gr.text(rcase) and eng.gtftext_stats()["route"] == route
    monkeypatch.delenv("L2R_GTX_ROUTE")
    # n differing from the run's reads
    eng.gtftext_begin(refs, b"lr2rmats", gr.PLAIN)
    for bad_n in (n - 1, n + 1):
        with pytest.raises(capi.L2RError) as e:
            eng.gtftext_rows(reads.tid[:bad_n] if bad_n < n else np.append(reads.tid, 0), reads.rev[:bad_n] if bad_n < n else np.append(reads.rev, 0), None, None, None, table,
                             ids[:bad_n] if bad_n < n else np.append(ids, 0), ids[:bad_n] if bad_n < n else np.append(ids, 0))
        assert "the last run had %d reads" % n in str(e.value) and "rc=-1:" not in str(e.value)


def test_chains_need_a_run(mixed):
    case = head(mixed[gr.PLAIN], 3)
    e = capi.Engine(0)
    e.gtftext_begin(case["refs"], case["source"], case["form"])
    with pytest.raises(capi.L2RError):
        e.gtftext_rows(case["tid"], case["rev"], None, None, None, case["table"], case["gid"], case["tids"])
    e.close()


# ---------------------------------------------------------------------------------------------------- the commands

CONFIGS = {"default": {}, "host": {"L2R_GTX_ROUTE": "host"}, "off": {"L2R_GTX_ROUTE": "off"}, "small": {"L2R_GTX_BATCH": 3, "L2R_GTX_TEXT_MAX": 400}}


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtx")
    anno = synth.make_annotation(3000, 63, nchr=3)
    reads = synth.make_reads(anno, 400, 5, 63)
    sam, bam = str(d / "r.sam"), str(d / "r.bam")
    reads.write_sam(sam)
    synth.write_bam(reads, bam)
    toy_bam, uniq_bam = str(d / "toy.bam"), str(d / "uniq.bam")
    assert hostlib.records_to_bam(os.path.join(TOY, "toy.sam"), toy_bam) == 0
    assert hostlib.records_to_bam(os.path.join(HAND, "uniq.sam"), uniq_bam) == 0
    return {"sam": sam, "bam": bam, "toy_sam": os.path.join(TOY, "toy.sam"), "toy_bam": toy_bam, "uniq_sam": os.path.join(HAND, "uniq.sam"), "uniq_bam": uniq_bam,
            "cigar_sam": os.path.join(HAND, "cigar.sam"), "mg_gtf": os.path.join(HAND, "mg_reads.gtf")}


def four_ways(args, expect_blocks=True):
    """One command in the four configurations: identical files; the default configuration says `route device`."""
    outs = {}
    for tag, env in CONFIGS.items():
        r = hostlib.run_cli(args, env=dict(env, L2R_TIMING=1))
        assert r.returncode == 0, (tag, r.stderr.decode()[-1500:])
        outs[tag] = r.stdout
        lines = [ln for ln in r.stderr.decode().splitlines() if "gtf text: route" in ln]
        if expect_blocks:
            assert lines, (tag, r.stderr.decode()[-1500:])
            want = {"default": "route device", "host": "route host", "off": "route off", "small": "route device"}[tag]
            assert all(want in ln for ln in lines), (tag, lines)
    assert outs["default"] == outs["host"] == outs["off"] == outs["small"]
    r = hostlib.run_cli(args)                               # without L2R_TIMING nothing new is written anywhere
    assert r.returncode == 0 and r.stdout == outs["default"] and b"gtf text" not in r.stderr
    return outs["default"]


@pytest.mark.parametrize("src", ["sam", "bam", "toy_sam", "toy_bam", "cigar_sam"])
def test_cli_bam2gtf(cli_files, src):
    out = four_ways(["bam2gtf", cli_files[src]])
    assert out.count(b"\ttranscript\t") >= 1
    if src.startswith("toy"):
        with open(os.path.join(TOY, "expect.bam2gtf.gtf"), "rb") as fh:
            assert out == fh.read()
    if src == "cigar_sam":
        with open(os.path.join(HAND, "cigar.bam2gtf.gtf"), "rb") as fh:
            assert out == fh.read()
    if src == "bam":
        small = hostlib.run_cli(["bam2gtf", "-s", "Src", cli_files["bam"]], env={"L2R_READ_WINDOW": 65600})
        whole = hostlib.run_cli(["bam2gtf", "-s", "Src", cli_files["sam"]])
        assert small.returncode == 0 and small.stdout == whole.stdout == out.replace(b"\tlr2rmats\t", b"\tSrc\t")


@pytest.mark.parametrize("extra", [[], ["-I"], ["-s"], ["-I", "-s"]])
def test_cli_unique_gtf_from_alignments(cli_files, extra):
    for src in ("bam", "uniq_sam", "uniq_bam"):
        out = four_ways(["unique-gtf", "-m", "b"] + extra + [cli_files[src]])
        if src.startswith("uniq") and extra in ([], ["-s"]):
            with open(os.path.join(HAND, "uniq_s.unique.gtf" if extra else "uniq.unique.gtf"), "rb") as fh:
                assert out == fh.read()


@pytest.mark.parametrize("extra", [[], ["-I"], ["-s"]])
def test_cli_unique_gtf_from_a_gtf(cli_files, tmp_path, extra):
    rgtf = str(tmp_path / "reads.gtf")
    r = hostlib.run_cli(["bam2gtf", cli_files["sam"]], stdout_path=rgtf)
    assert r.returncode == 0
    for gtf, hdr in ((rgtf, cli_files["sam"]), (cli_files["mg_gtf"], os.path.join(HAND, "upd.sam"))):
        four_ways(["unique-gtf", "-m", "g", "-b", hdr] + extra + [gtf])
