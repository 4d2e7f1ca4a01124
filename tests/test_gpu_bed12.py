"""`bam2bed` on the GPU: l2r_bed_lines (k_bed_measure in both forms, k_scan_u32, k_bed_write on the LDS and on the direct path) and the
command against tests/bed12_restatement.py, at the edges of the record count, the operation count, the tile text and the digits."""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import bed12_cases as bc
from tests import bed12_restatement as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bed12")
TILE = capi.header_define("L2R_BED_TILE")
LDS = capi.header_define("L2R_BED_LDS_BYTES")


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(0)
    e.bed_begin(bc.REFS)
    yield e
    e.close()


def lines(e, recs):
    flag, tid, pos, mapq, cigars, names = br.columns(recs)
    return e.bed_lines(flag, tid, pos, mapq, cigars, names)


def check(e, recs, refs=bc.REFS, color=b"255,0,0"):
    want = br.text(recs, refs, color)
    got = lines(e, recs)
    assert got == want, first_difference(got, want)
    st = e.bed_stats()
    assert (st["records"], st["lines"], st["bytes"]) == (len(recs), want.count(b"\n"), len(want)) and e.bed_n_lines == want.count(b"\n")
    assert st["guard_intact"] == 1
    return st


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at %d: %r / %r" % (len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40])


@pytest.fixture(scope="module")
def mixed():
    """3 x TILE + 17 random records and their text, made once."""
    recs = bc.random_records(np.random.default_rng(77), 3 * TILE + 17, max_ops=20)
    return recs, br.text(recs, bc.REFS)


# ---------------------------------------------------------------------------------------------------- the table of the issue

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_record_counts(eng, mixed, n):
    st = check(eng, mixed[0][:n])
    assert st["tiles_lds"] + st["tiles_direct"] == (n + TILE - 1) // TILE and st["route"] == 0


@pytest.mark.parametrize("k", [0, 1, 31, 32, 33, 63, 64, 65, 129, 300])
def test_operations_per_record_in_both_forms(eng, monkeypatch, k):
    recs = [bc.ops_record(k, seed) for seed in range(5)] + [(4, -1, -1, 0, b"u", [])] + [bc.ops_record(k, 9, flag=16, tid=2, pos=12345)]
    want = br.text(recs, bc.REFS)
    for form in (0, 1):
        monkeypatch.setenv("L2R_BED_WAVE", str(form))
        assert lines(eng, recs) == want and eng.bed_stats()["wave_form"] == form
    monkeypatch.delenv("L2R_BED_WAVE")
    mapped = [r for r in recs if not r[0] & 4]                      # (k operations each: the unmapped record has none)
    assert lines(eng, mapped) == br.text(mapped, bc.REFS)
    assert eng.bed_stats()["wave_form"] == (1 if k > 32 else 0)     # more than 32 operations per record on average: one wave per record


@pytest.mark.parametrize("b", [1, 2, 63, 64, 65, 300])
def test_blocks_per_line_in_both_forms(eng, monkeypatch, b):
    recs = [bc.blocks_record(b, seed, pos=seed * 1000) for seed in range(3)]
    want = br.text(recs, bc.REFS)
    assert all(ln.split(b"\t")[9] == b"%d" % b for ln in want.splitlines())
    for form in (0, 1):
        monkeypatch.setenv("L2R_BED_WAVE", str(form))
        assert lines(eng, recs) == want


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_text_at_the_lds_edge(eng, delta):
    recs = bc.tile_text_records(TILE, LDS + delta)
    assert len(br.text(recs[:TILE], bc.REFS)) % 16 != 0
    st = check(eng, recs)
    assert (st["tiles_lds"], st["tiles_direct"]) == ((2, 0) if delta <= 0 else (1, 1))


def test_digit_edges(eng, monkeypatch):
    recs = bc.digit_edge_records()
    check(eng, recs)
    monkeypatch.setenv("L2R_BED_WAVE", "1")
    check(eng, recs)


@pytest.mark.parametrize("form", [0, 1])
def test_end_at_the_limit(eng, monkeypatch, form):
    monkeypatch.setenv("L2R_BED_WAVE", str(form))
    recs = bc.end_limit_records(0)
    assert b"\t2147483647\t" in br.text(recs, bc.REFS)
    check(eng, recs)
    with pytest.raises(capi.L2RError) as e:
        lines(eng, bc.end_limit_records(1))
    assert "record 1:" in str(e.value) and "2147483648 is beyond 2147483647" in str(e.value)


def test_line_offsets_take_every_residue(eng):
    recs = bc.residue_records()
    offs = np.cumsum([0] + [len(br.line(r, bc.REFS)) for r in recs])
    assert {int(o) % 16 for o in offs} == set(range(16))
    check(eng, recs)
    for k in range(1, 17):                                          # ... and so does the end of the text
        check(eng, recs[:k])


def test_flags(eng):
    want = br.text(bc.flag_records(), bc.REFS).splitlines()
    assert [ln.split(b"\t")[3][-2:] for ln in want[:5]] == [b"f0", b"16", b"/1", b"/2", b"/1"] and [ln.split(b"\t")[5] for ln in want[:6]] == [b"+", b"-", b"+", b"+", b"+", b"-"]
    check(eng, bc.flag_records())


def test_unmapped_records_first_last_and_a_whole_tile(eng):
    recs = bc.unmapped_records(TILE)
    assert recs[0][0] & 4 and recs[-1][0] & 4 and all(r[0] & 4 for r in recs[TILE:2 * TILE])
    check(eng, recs)
    st = check(eng, [r for r in recs if r[0] & 4])
    assert st["lines"] == 0 and st["bytes"] == 0


def test_goldens_through_the_engine(eng):
    e = capi.Engine(0)
    for name in ("rule", "nocigar", "mix"):
        refs, recs = br.read_sam(os.path.join(GOLDEN, name + ".sam"))
        e.bed_begin(refs)
        with open(os.path.join(GOLDEN, name + ".bed"), "rb") as fh:
            assert lines(e, recs) == fh.read()
    e.close()


# ---------------------------------------------------------------------------------------------------- further checks

def test_long_lines_take_the_direct_path(eng, monkeypatch):
    recs = [bc.blocks_record(300, seed) for seed in range(TILE)] + [bc.rec(name=b"short")]
    want = br.text(recs, bc.REFS)
    assert len(want.splitlines()[0]) > LDS // TILE
    for form in (0, 1):
        monkeypatch.setenv("L2R_BED_WAVE", str(form))
        st = check(eng, recs)
        assert (st["tiles_lds"], st["tiles_direct"]) == (1, 1)


def test_the_guard_is_checked_and_intact(monkeypatch, mixed):
    monkeypatch.setenv("L2R_CHECK", "1")
    e = capi.Engine(0)
    e.bed_begin(bc.REFS)
    for recs in (mixed[0], bc.tile_text_records(TILE, LDS + 1), bc.residue_records()[:5]):
        assert check(e, recs)["guard_intact"] == 1
    e.close()


def test_batch_invariance(eng, mixed):
    recs, want = mixed
    assert lines(eng, recs) == want
    assert b"".join(lines(eng, recs[k:k + 1]) for k in range(len(recs))) == want
    cuts = [0, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE, len(recs)]
    assert b"".join(lines(eng, recs[a:b]) for a, b in zip(cuts, cuts[1:])) == want


def test_windows_of_one_set_of_columns(eng, mixed):
    """Batches as the command makes them: the offset columns of the whole input, shifted."""
    recs, want = mixed
    flag, tid, pos, mapq, (cig_off, cig), names = br.columns(recs)
    name_off, blob = capi.pack_names(names)
    got, at = [], 0
    while at < len(recs):
        k = capi.bed_cut(flag, tid, (cig_off, cig), (name_off, blob), bc.REFS, at, 100, 6000)
        assert 1 <= k <= 100
        got.append(eng.bed_lines(flag[at:at + k], tid[at:at + k], pos[at:at + k], mapq[at:at + k], (cig_off[at:at + k + 1], cig), (name_off[at:at + k + 1], blob)))
        at += k
    assert b"".join(got) == want and len(got) > 10


def test_host_route(eng, monkeypatch, mixed):
    monkeypatch.setenv("L2R_BED_ROUTE", "host")
    st = check(eng, mixed[0])
    assert st["route"] == 1
    with pytest.raises(capi.L2RError) as e:
        lines(eng, bc.end_limit_records(1))
    assert "record 1:" in str(e.value)


@pytest.mark.parametrize("kind,text", [("tid", "with reference"), ("pos", "at position"), ("op", "operation code above 8"), ("end", "is beyond 2147483647")])
@pytest.mark.parametrize("form", [0, 1])
def test_domain_errors_and_their_atomicity(eng, monkeypatch, kind, text, form):
    monkeypatch.setenv("L2R_BED_WAVE", str(form))
    bad = {"tid": bc.rec(tid=len(bc.REFS)), "pos": bc.rec(pos=-1), "op": bc.rec(cigar=[(5, bc.M)] * 70 + [(3, 9)]), "end": bc.end_limit_records(1)[1]}
    recs = [bc.rec(name=b"g%d" % k) for k in range(TILE + 9)]
    recs[TILE + 2] = bad["op" if kind != "op" else "end"]
    recs[5] = bad[kind]
    assert len(lines(eng, recs[:5])) > 0
    with pytest.raises(capi.L2RError) as e:
        lines(eng, recs)
    assert "record 5:" in str(e.value) and text in str(e.value)
    with pytest.raises(capi.L2RError):                              # a failed call leaves no text
        eng.bed_text_out(1 << 20)
    check(eng, recs[:5])


def test_text_out_needs_room(eng):
    want = br.text(bc.flag_records(), bc.REFS)
    assert lines(eng, bc.flag_records()) == want
    with pytest.raises(capi.L2RError):
        eng.bed_text_out(len(want) - 1)
    assert eng.bed_text_out(len(want)) == want


def test_an_oversized_batch_is_an_error_of_its_own(eng):
    """Summed bounds of 2^32 - 64: records described by counts, the CIGAR array is never read."""
    import ctypes as C
    n_ops = ((1 << 32) - 64) // 22 // 4
    cig_off = np.arange(6, dtype=np.int64) * n_ops
    z = np.zeros(5, np.int32)
    recs, _keep = capi._bed_records(z.astype(np.uint16), z, z, z.astype(np.uint8), (cig_off, np.zeros(1, np.uint32)), [b"n"] * 5)
    recs.n_cigar = int(cig_off[-1])
    n_lines, n_bytes = C.c_int64(0), C.c_int64(0)
    assert eng.lib.l2r_bed_lines(eng.ctx, C.byref(recs), C.byref(n_lines), C.byref(n_bytes)) != 0
    msg = eng.lib.l2r_last_error().decode()
    assert "the batch" in msg and "2^32 - 64" in msg
    with pytest.raises(capi.L2RError):
        eng.bed_text_out(1 << 20)


def test_bed_lines_needs_a_begin():
    e = capi.Engine(0)
    with pytest.raises(capi.L2RError):
        lines(e, [bc.rec()])
    e.close()


# ---------------------------------------------------------------------------------------------------- the command

def golden_paths(name):
    return os.path.join(GOLDEN, name + ".sam"), os.path.join(GOLDEN, name + ".bed")


@pytest.mark.parametrize("name", ["rule", "mix"])
def test_cli_goldens_from_sam_and_bam(tmp_path, name):
    sam, bed = golden_paths(name)
    with open(bed, "rb") as fh:
        want = fh.read()
    r = hostlib.run_cli(["bam2bed", sam])
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()
    n_records = sum(1 for ln in open(sam, "rb") if not ln.startswith(b"@"))
    assert b"Converted alignments: %d lines of %d records" % (want.count(b"\n"), n_records) in r.stderr
    bam = str(tmp_path / "in.bam")
    assert hostlib.records_to_bam(sam, bam) == 0
    out = str(tmp_path / "out.bed")
    r = hostlib.run_cli(["bam2bed", "-o", out, bam])
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    with open(out, "rb") as fh:
        assert fh.read() == want
    rc, counts = hostlib.bed_run(sam, str(tmp_path / "lib.bed"))
    assert rc == 0 and counts[:3] == [n_records, want.count(b"\n"), len(want)]
    with open(str(tmp_path / "lib.bed"), "rb") as fh:
        assert fh.read() == want


def test_cli_a_sam_record_without_a_cigar_is_unmapped_to_the_reader():
    """tests/golden/bed12/README.md: the engine writes the line of a mapped record without a CIGAR, the SAM reader never hands it one."""
    r = hostlib.run_cli(["bam2bed", golden_paths("nocigar")[0]])
    assert r.returncode == 0 and r.stdout == b"" and b"0 lines of 1 records" in r.stderr


def test_cli_colour_and_usage(tmp_path):
    sam, bed = golden_paths("mix")
    with open(bed, "rb") as fh:
        want = fh.read()
    r = hostlib.run_cli(["bam2bed", "-c", "0,128,255", sam])
    assert r.returncode == 0 and r.stdout == want.replace(b"\t255,0,0\t", b"\t0,128,255\t")
    for bad in (["-c", "1,2", sam], ["-c", "256,0,0", sam], ["-c", "1,2,3,4", sam], ["-c", "red", sam], [], ["-x", sam], [sam, sam]):
        r = hostlib.run_cli(["bam2bed"] + bad)
        assert r.returncode == 2 and r.stdout == b"", (bad, r.stderr)


def test_cli_domain_error_names_the_record_of_the_file(tmp_path):
    sam = str(tmp_path / "bad.sam")
    with open(sam, "w") as fh:
        fh.write("@SQ\tSN:chr1\tLN:1000\n")
        for k, cig in enumerate(["10M", "4M2N4M", "10M5B10M", "3M"]):
            fh.write("r%d\t0\tchr1\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % (k, 10 + k, cig))
    for env in (None, {"L2R_BED_BATCH": 2}, {"L2R_BED_BATCH": 1}):
        r = hostlib.run_cli(["bam2bed", sam], env=env)
        assert r.returncode == 1 and b"operation code above 8" in r.stderr and b"record 2 of the file" in r.stderr, r.stderr
        assert b"Converted" not in r.stderr


def test_cli_small_batches_give_the_same_file(tmp_path, mixed):
    recs = mixed[0][:150]
    sam = str(tmp_path / "in.sam")
    with open(sam, "wb") as fh:
        for name in bc.REFS:
            fh.write(b"@SQ\tSN:%s\tLN:2147483647\n" % name)
        for flag, tid, pos, mapq, name, cig in recs:
            cigar = b"".join(b"%d%s" % (n, br.OPS[op].encode()) for n, op in cig) or b"*"
            fh.write(b"\t".join([name, b"%d" % flag, bc.REFS[tid], b"%d" % (pos + 1), b"%d" % mapq, cigar, b"*", b"0", b"0", b"*", b"*"]) + b"\n")
    # (the reader takes a mapped record without a CIGAR for unmapped)
    want = br.text([r if r[5] else (r[0] | 4,) + r[1:] for r in recs], bc.REFS)
    a = hostlib.run_cli(["bam2bed", sam])
    b = hostlib.run_cli(["bam2bed", sam], env={"L2R_BED_BATCH": 3, "L2R_BED_TEXT_MAX": 200})
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == want and b.stdout == want
