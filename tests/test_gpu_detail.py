"""The detail table of `update-gtf -A` on the GPU: l2r_detail_* (k_detail_measure in both forms, k_scan_u32, k_detail_write on the LDS
and on the direct path, a lane or a wave per segment) and the command against tests/detail_restatement.py, at the edges of the read
count, the exon count, the flag patterns, the tile text, the digits, the names and the batch cut.  Every case asserts route 0 and an
intact guard, and every generated case lies inside the domain (checked on the CPU by the restatement, which raises otherwise)."""
import filecmp
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib, synth
from tests import detail_cases as dc
from tests import detail_restatement as dr
from tests.test_detail_cpu import edge_cases, error_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "toy")
HAND = os.path.join(ROOT, "tests", "golden", "hand")
TILE = capi.header_define("L2R_DETAIL_TILE")
LDS = capi.header_define("L2R_DETAIL_LDS_BYTES")


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


def check(e, case, max_rows=1 << 20, max_bytes=1 << 30, route=0):
    """The engine's text of a case against the restatement; route and guard; the stats of the last batch."""
    whole = dr.text(case)                               # (raises where a read lies outside the domain)
    text, n_bytes, st = dc.engine_text(e, case, max_rows, max_bytes)
    assert text == whole, first_difference(text, whole)
    assert n_bytes == len(whole)
    assert st["rows"] == len(case["tid"]) and st["route"] == route and st["guard_intact"] == 1
    return st


def head(case, n):
    x = int(case["ex_off"][n])
    c = dict(case)
    for k in ("tid", "qname", "info", "ref_tx"):
        c[k] = case[k][:n]
    c["ex_off"] = case["ex_off"][:n + 1]
    for k in ("xs", "xe", "f"):
        c[k] = case[k][:x]
    return c


@pytest.fixture(scope="module")
def mixed():
    """3 x TILE + 17 reads, made once."""
    rng = np.random.default_rng(7)
    return dc.make_case(70, rng.choice([1, 1, 2, 3, 4, 6, 9, 14, 25, 70], 3 * TILE + 17))


# ---------------------------------------------------------------------------------------------------- read and exon counts

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_read_counts(eng, mixed, n):
    st = check(eng, head(mixed, n))
    if n:
        assert st["tiles_lds"] + st["tiles_direct"] == (n + TILE - 1) // TILE and st["batches"] == 1


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 63, 64, 65, 129, 300, 2000])
def test_exons_per_read_in_both_forms(eng, monkeypatch, k):
    case = dc.make_case(100 + k, [k] * 7)
    for form in (0, 1):
        monkeypatch.setenv("L2R_DETAIL_WAVE", str(form))
        assert check(eng, case)["wave_form"] == form
    monkeypatch.delenv("L2R_DETAIL_WAVE")
    assert check(eng, case)["wave_form"] == (1 if k > 32 else 0)        # more than 32 exons per read on average: one wave per read


def test_the_form_follows_the_average(eng):
    assert check(eng, dc.make_case(5, [1, 1, 1, 300]))["wave_form"] == 1
    assert check(eng, dc.make_case(5, [1] * 40 + [300]))["wave_form"] == 0
    assert check(eng, dc.make_case(6, [32, 33, 31]))["wave_form"] == 0   # exactly 32 on average
    assert check(eng, dc.make_case(6, [32, 33, 32]))["wave_form"] == 1


@pytest.mark.parametrize("at", [0, TILE // 2, TILE - 1])
def test_one_long_read_among_short_ones(eng, monkeypatch, at):
    exons = [8] * TILE
    exons[at] = 2000
    for flags in ("random", dc.ALL_FLAGS):
        case = dc.make_case(200 + at, exons + [2, 300, 1], flags=flags)
        for form in (0, 1):
            monkeypatch.setenv("L2R_DETAIL_WAVE", str(form))
            check(eng, case)


# ---------------------------------------------------------------------------------------------------- flag patterns

def pattern_case():
    """Per exon count and per flag bit: the bit on no exon, on every exon, on the first alone, on exon n - 2 alone (the last junction) and on
    the last exon alone (which belongs to no junction list); donor and acceptor together at junction n - 2."""
    exons, flags = [], []
    for n in (1, 2, 3, 7, 64, 65, 70, 130):
        rows = [np.zeros(n, np.uint8)]
        for bit in (1, 2, 4, 8, 16, 6, 31):
            rows.append(np.full(n, bit, np.uint8))
            for at in {0, max(n - 2, 0), n - 1}:
                f = np.zeros(n, np.uint8)
                f[at] = bit
                rows.append(f)
        exons += [n] * len(rows)
        flags += rows
    case = dc.make_case(300, exons, flags=0)
    case["f"] = np.concatenate(flags)
    return case


def test_flag_patterns_per_list(eng, monkeypatch):
    case = pattern_case()
    text = dr.text(case)
    assert b"\t0\tNA\t0\tNA\t0\tNA\t0\tNA\t\n" in text and b"\t1\t1\n" in text
    for form in (0, 1):
        monkeypatch.setenv("L2R_DETAIL_WAVE", str(form))
        check(eng, case)
    # a junction flag on the last exon does not appear
    one = dc.make_case(301, [3], flags=0)
    one["f"][:] = [0, 0, 2 | 4 | 8 | 16]
    assert dr.text(one).endswith(b"\t0\tNA\t0\tNA\t0\tNA\t0\tNA\t\n")
    check(eng, one)


def test_digit_edges_names_and_chromosomes(eng, monkeypatch):
    for case in edge_cases():
        for form in (0, 1):
            monkeypatch.setenv("L2R_DETAIL_WAVE", str(form))
            check(eng, case)


@pytest.mark.parametrize("name_len", [0, 1, 254])
def test_names(eng, name_len):
    check(eng, dc.make_case(31, [1, 3, 2, 70, 1], name_len=(name_len, name_len), gene_len=(name_len, name_len), no_ref=0.0, refs=(b"1", b"L" * 200)))
    check(eng, dc.make_case(32, [1, 3, 2, 70, 1], name_len=(name_len, name_len), no_ref=1.0))           # NA through ref = -1
    check(eng, dc.make_case(33, [2, 2], n_tx=0))


# ---------------------------------------------------------------------------------------------------- the LDS edge and the stream-out

def set_names(case, names):
    case["names"] = b"".join(n + b"\0" for n in names)
    case["qname"] = np.cumsum([0] + [len(n) + 1 for n in names[:-1]]).astype(np.uint32)


def tile_text_case(target):
    """TILE reads whose text has exactly ``target`` bytes, and a short tile behind (it starts off a 16-byte boundary where target does)."""
    per = 52                                            # exons of the first tile's reads: about a kilobyte a line
    case = dc.make_case(41, [per] * TILE + [2, 1, 3], flags=0, name_len=(1, 1))
    base = sum(len(t) for t in dr.texts(case)[:TILE])
    spare = target - base                               # ... and the read names give the rest, a byte each
    assert 0 <= spare <= TILE * 253, (base, target)
    names = []
    for i in range(TILE + 3):
        k = min(253, spare) if i < TILE else 0
        names.append(b"n" * (1 + k))
        spare -= k
    set_names(case, names)
    assert sum(len(t) for t in dr.texts(case)[:TILE]) == target
    return case


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_text_at_the_lds_edge(eng, delta):
    st = check(eng, tile_text_case(LDS + delta))
    assert (st["tiles_lds"], st["tiles_direct"]) == ((2, 0) if delta <= 0 else (1, 1))


def test_tile_offsets_take_every_residue(eng):
    """The stream-out of k_detail_write (text_stream_out) with the second tile's span beginning at every offset modulo 16."""
    seen = set()
    for r in range(16):
        case = dc.make_case(47, [2, 5, 1, 9] * (TILE // 2) + [3], name_len=(4, 4))
        names = [b"read"] * (2 * TILE + 1)
        set_names(case, names)
        first = sum(len(t) for t in dr.texts(case)[:TILE])
        names[0] = b"read" + b"x" * ((r - first) % 16)
        set_names(case, names)
        second = sum(len(t) for t in dr.texts(case)[:TILE])              # where the second tile's span begins
        assert second % 16 == r
        seen.add(second % 16)
        st = check(eng, case)
        assert (st["tiles_lds"], st["tiles_direct"], st["batches"]) == (3, 0, 1)
    assert seen == set(range(16))


def test_oversized_tiles_take_the_direct_path(eng, monkeypatch):
    case = dc.make_case(43, [2000] * 3 + [1] * (TILE - 3) + [2] * 5, name_len=(100, 254))
    for form in (0, 1):
        monkeypatch.setenv("L2R_DETAIL_WAVE", str(form))
        st = check(eng, case)
        assert (st["tiles_lds"], st["tiles_direct"]) == (1, 1)


# ---------------------------------------------------------------------------------------------------- batches, routes, errors

def test_batch_invariance(eng, mixed):
    n = len(mixed["tid"])
    lens = [len(t) for t in dr.texts(mixed)]
    small = head(mixed, 40)
    assert check(eng, small, max_rows=1)["batches"] == 40
    assert check(eng, mixed, max_rows=3)["batches"] == (n + 2) // 3
    assert check(eng, mixed, max_rows=TILE + 1)["batches"] == (n + TILE) // (TILE + 1)
    tile_bytes = [sum(lens[a:a + TILE]) for a in range(0, n, TILE)]
    st = check(eng, mixed, max_bytes=min(tile_bytes) // 2)               # a byte cap that splits every tile
    assert st["batches"] >= 2 * len(tile_bytes) - 1
    assert check(eng, small, max_bytes=1)["batches"] == 40               # down to one row each


def test_lines_takes_what_the_cut_says(eng, mixed):
    case = head(mixed, 50)
    want = dr.texts(case)
    lens = [len(t) for t in want]
    dc.engine_rows(eng, case)
    for first, mr, mb in ((0, 7, 1 << 30), (10, 1 << 20, sum(lens[10:13])), (10, 1 << 20, sum(lens[10:13]) - 1), (10, 1 << 20, sum(lens[10:13]) + 1), (49, 5, 1)):
        k, text = eng.detail_lines(first, mr, mb)
        assert k == dr.cut(lens, first, mr, mb) and text == b"".join(want[first:first + k])
        st = eng.detail_stats()
        assert st["lines"] == k and st["bytes"] == len(text) and st["route"] == 0 and st["guard_intact"] == 1
    with pytest.raises(capi.L2RError):
        eng.detail_lines(50)
    with pytest.raises(capi.L2RError):
        eng.detail_lines(0, 0)


def test_out_needs_room(eng, mixed):
    case = head(mixed, 9)
    want = dr.text(case)
    dc.engine_rows(eng, case)
    with pytest.raises(capi.L2RError):
        eng.detail_lines(0, cap=len(want) - 1)
    buf = np.full(len(want) + 8, 0x55, np.uint8)
    assert eng.lib.l2r_detail_out(eng.ctx, buf.ctypes.data, len(want) - 1) != 0 and (buf == 0x55).all()      # too little room: nothing is written
    eng._chk(eng.lib.l2r_detail_out(eng.ctx, buf.ctypes.data, len(want)))
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0x55).all()


def test_every_domain_error(eng, monkeypatch):
    good = dc.make_case(51, [2, 1])
    for wave in (0, 1):
        monkeypatch.setenv("L2R_DETAIL_WAVE", str(wave))
        for case, read, kind in error_cases():
            with pytest.raises(capi.L2RError) as e:
                dc.engine_rows(eng, case)
            assert "rc=-1:" in str(e.value) and "read %d:" % read in str(e.value) and dr.KIND_TEXT[kind] in str(e.value), (kind, read, str(e.value))
            with pytest.raises(capi.L2RError) as e:          # nothing was written and nothing can be fetched
                eng.detail_lines(0)
            assert "rc=-1:" not in str(e.value)
            check(eng, good)                                 # ... and the next good call works


def test_order_of_calls(mixed):
    case = head(mixed, 3)
    e = capi.Engine(0)
    calls = [lambda: e.detail_rows(case["tid"], case["names"], case["qname"], dc.result_of(case)), lambda: e.detail_lines(0)]
    for call in calls:
        with pytest.raises(capi.L2RError) as err:
            call()
        assert "rc=-1:" not in str(err.value)
    e.detail_begin(case["refs"], case["anno"], case["tx_gid"], case["tx_gname"])
    with pytest.raises(capi.L2RError):
        calls[1]()
    calls[0]()
    assert e.detail_lines(0)[0] == 3
    with pytest.raises(capi.L2RError):                       # results that do not fit the rows: an argument error
        e.detail_rows(case["tid"][:2], case["names"], case["qname"][:2], dc.result_of(case), n=2)
    with pytest.raises(capi.L2RError):                       # ... which leaves no rows behind
        calls[1]()
    e.close()


def test_route_host_gives_the_same_bytes(eng, monkeypatch, mixed):
    monkeypatch.setenv("L2R_DETAIL_ROUTE", "host")
    check(eng, mixed, route=1)
    check(eng, head(mixed, 40), max_rows=3, route=1)
    for case, read, kind in error_cases():
        with pytest.raises(capi.L2RError) as e:
            dc.engine_rows(eng, case)
        assert "rc=-1:" in str(e.value) and "read %d:" % read in str(e.value) and dr.KIND_TEXT[kind] in str(e.value)


# ---------------------------------------------------------------------------------------------------- the results of a run

@pytest.fixture(scope="module")
def run_set():
    anno = synth.make_annotation(3000, 61, nchr=3)
    return anno.in_file_order(), synth.make_reads(anno, 700, 6, 61)


def run_reads(e, af, reads, want=capi.WANT_RESULTS):
    e.set_params(capi.default_params(full_level=3))
    e.set_outputs(want)
    e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    e.set_junctions(None)
    e.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    e.run()
    e.sync()


def test_the_results_of_a_run_where_they_lie(eng, monkeypatch, run_set):
    af, reads = run_set
    run_reads(eng, af, reads)
    res = eng.download()
    n, x = reads.n, int(res.ex_off[-1])
    names, qname = dr.pack_table([reads.qname(i).encode() for i in range(n)])
    anno, ids = dr.pack_table([af.gene_id(int(g)).encode() for g in af.tx_gene] + [af.gene_name(int(g)).encode() for g in af.tx_gene])
    refs = [c.encode() for c in reads.chrom_names]
    case = {"refs": refs, "tid": reads.tid, "names": names, "qname": np.asarray(qname, np.uint32), "anno": anno, "tx_gid": np.asarray(ids[:af.n_tx], np.uint32),
            "tx_gname": np.asarray(ids[af.n_tx:], np.uint32), "ex_off": res.ex_off, "xs": res.ex_start[:x], "xe": res.ex_end[:x], "f": res.ex_flag[:x],
            "info": res.info[:n], "ref_tx": res.ref_tx[:n]}
    want = dr.text(case)
    cls = {t.split(b"\t")[3] for t in dr.texts(case)}
    assert cls == {b"0", b"1", b"2"} and (case["f"] != 0).any() and (case["ref_tx"] < 0).any() and (case["ref_tx"] >= 0).any()
    for wave in (None, 0, 1):
        if wave is not None:
            monkeypatch.setenv("L2R_DETAIL_WAVE", str(wave))
        eng.detail_begin(refs, anno, case["tx_gid"], case["tx_gname"])
        assert eng.detail_rows(reads.tid, names, case["qname"]) == len(want)
        got = eng.detail_all(n, max_rows=TILE + 1)
        assert got == want, first_difference(got, want)
        st = eng.detail_stats()
        assert st["route"] == 0 and st["guard_intact"] == 1 and (wave is None or st["wave_form"] == wave)
    monkeypatch.delenv("L2R_DETAIL_WAVE")
    assert check(eng, case)["route"] == 0                    # the same rows uploaded from l2r_download's arrays
    monkeypatch.setenv("L2R_DETAIL_ROUTE", "host")           # the host route fetches the results itself
    eng.detail_begin(refs, anno, case["tx_gid"], case["tx_gname"])
    assert eng.detail_rows(reads.tid, names, case["qname"]) == len(want)
    assert eng.detail_all(n) == want and eng.detail_stats()["route"] == 1
    monkeypatch.delenv("L2R_DETAIL_ROUTE")
    for bad_n in (n - 1, n + 1):                             # n differing from the run's reads
        with pytest.raises(capi.L2RError) as e:
            eng.detail_rows(reads.tid[:bad_n] if bad_n < n else np.append(reads.tid, 0), names, case["qname"][:bad_n] if bad_n < n else np.append(case["qname"], 0))
        assert "the last run had %d reads" % n in str(e.value) and "rc=-1:" not in str(e.value)


def test_results_need_a_run_that_kept_them(run_set, mixed):
    af, reads = run_set
    case = head(mixed, 3)
    e = capi.Engine(0)
    e.detail_begin(case["refs"], case["anno"], case["tx_gid"], case["tx_gname"])
    with pytest.raises(capi.L2RError) as err:                # no run at all
        e.detail_rows(case["tid"], case["names"], case["qname"])
    assert "no completed run" in str(err.value) and "rc=-1:" not in str(err.value)
    run_reads(e, af, reads, want=capi.WANT_ACCEPTED)
    names, qname = dr.pack_table([reads.qname(i).encode() for i in range(reads.n)])
    e.detail_begin([c.encode() for c in reads.chrom_names])
    with pytest.raises(capi.L2RError) as err:
        e.detail_rows(reads.tid, names, np.asarray(qname, np.uint32))
    assert "kept no results" in str(err.value) and "rc=-1:" not in str(err.value)
    e.close()


# ---------------------------------------------------------------------------------------------------- the command

CONFIGS = {"default": {}, "host": {"L2R_DETAIL_ROUTE": "host"}, "off": {"L2R_DETAIL_ROUTE": "off"}, "small": {"L2R_DETAIL_BATCH": 3, "L2R_DETAIL_TEXT_MAX": 400},
           "shards": {"L2R_CHUNK_READS": None}}
ROUTE = {"default": "route device", "host": "route host", "off": "route off", "small": "route device", "shards": "route device"}
OUTS = ("gtf", "detail", "summary", "bed", "known", "novel", "unrec", "all")


def five_ways(tmp_path, make_args, n_reads, extra_env=None, route=None):
    """One command in the five configurations: identical files and stdout; the timing line names the route.  make_args(outs) -> (argv,
    the files it writes).  Returns the default configuration's files."""
    got = {}
    for tag, env in CONFIGS.items():
        env = dict(env, L2R_TIMING=1, **(extra_env or {}))
        if tag == "shards":
            env["L2R_CHUNK_READS"] = max(1, n_reads // 3 - 1)                                  # at least three engine shards
        d = tmp_path / tag
        d.mkdir()
        argv, files = make_args({k: str(d / k) for k in OUTS})
        r = hostlib.run_cli(argv, env=env)
        assert r.returncode == 0, (tag, r.stderr.decode()[-1500:])
        lines = [ln for ln in r.stderr.decode().splitlines() if "detail text: route" in ln]
        assert len(lines) == 1 and (route or ROUTE)[tag] in lines[0], (tag, lines)
        if tag == "small" and n_reads > 3 and not route:
            assert int(lines[0].split(" batches")[0].split()[-1]) >= n_reads // 3
        got[tag] = (files, r.stdout)
    for tag in CONFIGS:
        assert got[tag][1] == got["default"][1], tag
        for a, b in zip(got[tag][0], got["default"][0]):
            assert filecmp.cmp(a, b, shallow=False), (tag, a)
    d = tmp_path / "plain"
    d.mkdir()
    argv, files = make_args({k: str(d / k) for k in OUTS})
    r = hostlib.run_cli(argv, env=extra_env)                                                   # without L2R_TIMING nothing new is on stderr
    assert r.returncode == 0 and r.stdout == got["default"][1] and b"detail text" not in r.stderr
    for a, b in zip(files, got["default"][0]):
        assert filecmp.cmp(a, b, shallow=False), a
    return got["default"][0]


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("detail")
    anno = synth.make_annotation(3000, 63, nchr=3)
    reads = synth.make_reads(anno, 400, 5, 63)
    sam, bam, gtf = str(d / "r.sam"), str(d / "r.bam"), str(d / "a.gtf")
    reads.write_sam(sam)
    synth.write_bam(reads, bam)
    anno.write_gtf(gtf)
    return {"sam": sam, "bam": bam, "gtf": gtf, "n": reads.n}


def all_outputs(o, extra, aln, gtf):
    return (["update-gtf"] + extra + ["-A", o["detail"], "-y", o["summary"], "-E", o["bed"], "-k", o["known"], "-v", o["novel"], "-u", o["unrec"], "-a", o["all"],
                                      "-o", o["gtf"], aln, gtf], [o[k] for k in OUTS])


@pytest.mark.parametrize("src", ["sam", "bam"])
def test_cli_synthetic_set(tmp_path, cli_files, src):
    files = five_ways(tmp_path, lambda o: all_outputs(o, ["-l", "3"], cli_files[src], cli_files["gtf"]), cli_files["n"])
    detail = open(files[1], "rb").read()
    assert detail.startswith(dr.HEADER) and detail.count(b"\n") == cli_files["n"] + 1


def test_cli_threaded_tail(tmp_path, cli_files):
    five_ways(tmp_path, lambda o: all_outputs(o, ["-l", "3"], cli_files["bam"], cli_files["gtf"]), cli_files["n"], extra_env={"L2R_THREADS": 3, "L2R_TAIL_PART_READS": 50})


def test_cli_toy(tmp_path):
    def args(o):
        return ["update-gtf", "-l", "3", "-A", o["detail"], "-y", o["summary"], "-E", o["bed"], "-o", o["gtf"], os.path.join(TOY, "toy.sam"), os.path.join(TOY, "original.gtf")], \
               [o["gtf"], o["detail"], o["summary"], o["bed"]]
    n = sum(1 for ln in open(os.path.join(TOY, "toy.sam")) if not ln.startswith("@"))
    files = five_ways(tmp_path, args, n)
    for f, ext in zip(files, ("updated.gtf", "detail.txt", "summary.txt", "novel_exon.bed")):
        assert filecmp.cmp(f, os.path.join(TOY, "expect_l3." + ext), shallow=False), ext


@pytest.mark.parametrize("name", ["upd", "sj", "split", "mg", "uns"])
def test_cli_hand_cases(tmp_path, name):
    from tests.test_hand_known_answers import CASES
    cmd, inp, anno, expect = CASES[name]

    def args(o):
        return list(cmd) + ["-A", o["detail"], "-y", o["summary"], "-E", o["bed"], "-o", o["gtf"], os.path.join(HAND, inp), os.path.join(HAND, anno if isinstance(anno, str) else "anno.gtf")], \
               [o["gtf"], o["detail"], o["summary"], o["bed"]]
    n = sum(1 for ln in open(os.path.join(HAND, inp)) if not ln.startswith("@") and (name != "mg" or "\ttranscript\t" in ln))
    files = five_ways(tmp_path, args, n)
    assert filecmp.cmp(files[1], os.path.join(HAND, expect["detail"]), shallow=False)
    assert filecmp.cmp(files[0], os.path.join(HAND, expect["gtf"]), shallow=False)


# (No case with a read outside the engine's domain through the command: the alignment reader stops at a read name of 100 characters -- the
#  reference stores names in char[100] -- and the GTF reader at as much for gene ids and names, so the command never sees a name of 255 bytes;
#  test_every_domain_error above covers the -1 that the command's per-shard fall-back on the tail's writer answers.)
