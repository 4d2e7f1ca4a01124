"""`bam2bed`, the parts that need no GPU: tests/bed12_restatement.py against the hand-written goldens (tests/golden/bed12), and the host side
of l2r_bed_lines -- the argument checks, bed_line_bound, bed_cut and the exact host routine bed_lines_host -- as a stand-alone program
under ASan + UBSan (tests/bed_dump.hip, `make -C lr2rmats_amd/csrc bed-dump`) against the restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import bed12_cases as bc
from tests import bed12_restatement as br
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BED_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "bed_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bed12")
NAMES = ("rule", "nocigar", "mix")
TILE = capi.header_define("L2R_BED_TILE")
BATCH_BYTES = (1 << 32) - 64


def golden(name):
    refs, recs = br.read_sam(os.path.join(GOLDEN, name + ".sam"))
    with open(os.path.join(GOLDEN, name + ".bed"), "rb") as fh:
        return refs, recs, fh.read()


# ---------------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_goldens(name):
    refs, recs, want = golden(name)
    assert br.text(recs, refs) == want


def test_the_three_lines_of_the_rule():
    lines = golden("rule")[2].split(b"\n") + golden("nocigar")[2].split(b"\n")
    assert lines[0] == b"chr1 99 239 r1 60 + 99 239 255,0,0 2 20,20 0,120".replace(b" ", b"\t")
    assert lines[1] == b"chr2 0 138 q/2 0 - 0 138 255,0,0 4 0,9,0,9 0,50,89,129".replace(b" ", b"\t")
    assert lines[3] == b"chrM 7 7 p/1 255 + 7 7 255,0,0 1 0 0".replace(b" ", b"\t")


def test_the_goldens_hold_what_they_should():
    refs, recs, want = golden("mix")
    assert [r[0] & 4 for r in recs[:3]] == [0, 4, 0] and recs[0][0] & 16
    assert {len(r[4]) for r in recs} >= {1, 254} and {r[3] for r in recs} >= {0, 9, 10, 99, 100, 255}
    assert want.count(b"\n") == len(recs) - 1


def test_colour_strings():
    for good in ("255,0,0", "0,128,255", "0,0,0", "007,1,02"):
        assert hostlib.bed_color_ok(good)
    for bad in ("", "255,0", "255,0,0,0", "256,0,0", "1,2,3 ", " 1,2,3", "1,,3", "a,b,c", "1.0,2,3", "-1,2,3", "1,2,3,", "0255,0,0"):
        assert not hostlib.bed_color_ok(bad)


# ---------------------------------------------------------------------------------------------------- the host side (bed_dump)

@pytest.fixture(scope="module")
def bed_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "bed-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return BED_DUMP


def case_bytes(records, refs, color=b"255,0,0", first=0, max_records=1 << 20, max_bytes=1 << 30):
    flag, tid, pos, mapq, (cig_off, cig), names = br.columns(records)
    name_off, blob = capi.pack_names(names)
    ref_off, ref_blob = capi.pack_names(refs)
    head = struct.pack("<8q", len(records), len(cig), len(refs), len(color), first, max_records, max_bytes, 0)
    return head + b"".join(a.tobytes() for a in (flag, tid, pos, mapq, cig_off, cig, name_off, blob, ref_off, ref_blob)) + color


def counts_case_bytes(n_ops, name_len, refs, flag=None, first=0, max_records=1 << 20, max_bytes=1 << 30, color=b"255,0,0"):
    """Records described by their counts alone: no CIGAR word and no name byte is in the file."""
    n = len(n_ops)
    cig_off = np.zeros(n + 1, np.int64); cig_off[1:] = np.cumsum(np.asarray(n_ops, np.int64))
    name_off = np.zeros(n + 1, np.int64); name_off[1:] = np.cumsum(np.asarray(name_len, np.int64))
    ref_off, ref_blob = capi.pack_names(refs)
    head = struct.pack("<8q", n, int(cig_off[-1]), len(refs), len(color), first, max_records, max_bytes, 1)
    cols = (np.zeros(n, np.uint16) if flag is None else np.asarray(flag, np.uint16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8))
    return head + b"".join(a.tobytes() for a in cols + (cig_off, name_off, ref_off, ref_blob)) + color


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


def check(got, records, refs, color=b"255,0,0"):
    """Text, line count and bounds of a dump against the restatement."""
    assert int(got["rc"][0]) == 0, bytes(got.get("error", b"")).decode()
    try:
        want = br.text(records, refs, color)
    except br.BedDomainError as e:
        assert int(got["lines_rc"][0]) != 0
        msg = bytes(got["error"]).decode()
        assert "record %d:" % e.record in msg and br.KIND_TEXT[e.kind] in msg, (msg, e.record, e.kind)
        return
    assert int(got["lines_rc"][0]) == 0, bytes(got.get("error", b"")).decode()
    assert bytes(got["text"]) == want
    assert int(got["n_lines"][0]) == want.count(b"\n") == sum(1 for r in records if not r[0] & 4)
    true_len = [len(br.line(r, refs, color)) for r in records]
    assert all(int(b) >= t for b, t in zip(got["bound"], true_len)), [(int(b), t) for b, t in zip(got["bound"], true_len) if int(b) < t][:5]
    assert all(int(b) == 0 for b, r in zip(got["bound"], records) if r[0] & 4)


EDGE_SETS = {
    "digits": bc.digit_edge_records, "end_ok": lambda: bc.end_limit_records(0), "residues": bc.residue_records, "flags": bc.flag_records,
    "unmapped": lambda: bc.unmapped_records(TILE), "worst_bound": bc.bound_worst_records,
    "ops": lambda: [bc.ops_record(k) for k in (0, 1, 31, 32, 33, 63, 64, 65, 129, 300)],
    "blocks": lambda: [bc.blocks_record(b) for b in (1, 2, 63, 64, 65, 300)],
    "nothing": lambda: [], "only_unmapped": lambda: [(4, -1, -1, 0, b"u", [])],
}


def test_host_routine_on_the_goldens(bed_dump, tmp_path):
    sets = [golden(n) for n in NAMES]
    for got, (refs, recs, want) in zip(dump(bed_dump, tmp_path, [case_bytes(recs, refs) for refs, recs, _ in sets]), sets):
        check(got, recs, refs)
        assert bytes(got["text"]) == want


def test_host_routine_on_the_edges(bed_dump, tmp_path):
    sets = [f() for f in EDGE_SETS.values()]
    for got, recs in zip(dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS) for recs in sets]), sets):
        check(got, recs, bc.REFS)


def test_host_routine_on_random_records_and_colours(bed_dump, tmp_path):
    rng = np.random.default_rng(12)
    sets = [bc.random_records(rng, int(rng.integers(1, 60)), max_ops=int(rng.choice([3, 12, 80]))) for _ in range(40)]
    colors = [b"255,0,0", b"0,128,255", b"", b"255,255,255,"]
    for k, (got, recs) in enumerate(zip(dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS, colors[k % 4]) for k, recs in enumerate(sets)]), sets)):
        check(got, recs, bc.REFS, colors[k % 4])


def test_a_window_of_larger_columns_gives_the_same_text(bed_dump, tmp_path):
    """cig_off need not start at 0: the CIGAR words of records in front stay in the array."""
    recs = bc.random_records(np.random.default_rng(5), 30)
    flag, tid, pos, mapq, (cig_off, cig), names = br.columns(recs)
    k = 11
    name_off, blob = capi.pack_names(names[k:])
    ref_off, ref_blob = capi.pack_names(bc.REFS)
    head = struct.pack("<8q", len(recs) - k, len(cig), len(bc.REFS), 7, 0, 1 << 20, 1 << 30, 0)
    case = head + b"".join(a.tobytes() for a in (flag[k:], tid[k:], pos[k:], mapq[k:], cig_off[k:], cig, name_off, blob, ref_off, ref_blob)) + b"255,0,0"
    check(dump(bed_dump, tmp_path, [case])[0], recs[k:], bc.REFS)


# ---------------------------------------------------------------------------------------------------- domain errors

BAD = {
    "tid": lambda: bc.rec(tid=len(bc.REFS), name=b"bad"), "tid_negative": lambda: bc.rec(tid=-1, name=b"bad"), "pos": lambda: bc.rec(pos=-1, name=b"bad"),
    "op": lambda: bc.rec(cigar=[(5, bc.M), (3, 9), (5, bc.M)], name=b"bad"), "op15": lambda: bc.rec(cigar=[(5, 15)], name=b"bad"),
    "end": lambda: bc.end_limit_records(1)[1],
}


def two_bad(kind, other="op"):
    """Good records around two bad ones: the smaller index is `kind`'s."""
    recs = [bc.rec(name=b"g%d" % k, pos=k) for k in range(9)]
    recs[3] = BAD[kind]()
    recs[6] = BAD[other if other != kind else "end"]()
    return recs


@pytest.mark.parametrize("kind", sorted(BAD))
def test_domain_errors_name_the_smallest_bad_record(bed_dump, tmp_path, kind):
    recs = two_bad(kind)
    with pytest.raises(br.BedDomainError) as e:
        br.text(recs, bc.REFS)
    assert e.value.record == 3 and e.value.kind == kind.split("_")[0].rstrip("15")
    got = dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS)])[0]
    check(got, recs, bc.REFS)
    assert "text" not in got


def test_an_unmapped_record_is_never_an_error(bed_dump, tmp_path):
    recs = [bc.rec(), (4, 99, -5, 0, b"u", [(1, 14)]), bc.rec(name=b"z")]
    check(dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS)])[0], recs, bc.REFS)


def test_argument_checks(bed_dump, tmp_path):
    recs = [bc.rec(name=b"n" * 255)]
    got = dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS)])[0]
    assert int(got["rc"][0]) != 0 and "a name of 255 bytes" in bytes(got["error"]).decode()
    desc = bytearray(case_bytes([bc.rec(), bc.rec()], bc.REFS))
    flag, tid, pos, mapq, (cig_off, cig), names = br.columns([bc.rec(), bc.rec()])
    at = 64 + flag.nbytes + tid.nbytes + pos.nbytes + mapq.nbytes
    desc[at:at + 24] = np.array([0, 2, 1], np.int64).tobytes()
    got = dump(bed_dump, tmp_path, [bytes(desc)])[0]
    assert int(got["rc"][0]) != 0 and "cig_off descends at record 1" in bytes(got["error"]).decode()


# ---------------------------------------------------------------------------------------------------- cuts

def replay_cut(bound, first, max_records, max_bytes):
    """What the rule of l2r_bed_cut makes of the bounds."""
    out, at = [], first
    while at < len(bound):
        k, total = 0, 0
        while at + k < len(bound) and k < max_records and (k == 0 or (total + bound[at + k] < max_bytes and total + bound[at + k] < BATCH_BYTES)):
            total += bound[at + k]
            k += 1
        out.append(k)
        at += k
    return out


@pytest.mark.parametrize("max_records,max_bytes", [(1, 1 << 30), (3, 1 << 30), (1 << 20, 200), (7, 1000), (1 << 20, 1), (5, 5000)])
def test_cuts_make_progress_and_respect_both_limits(bed_dump, tmp_path, max_records, max_bytes):
    recs = bc.random_records(np.random.default_rng(3), 120, max_ops=40)
    got = dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS, max_records=max_records, max_bytes=max_bytes)])[0]
    bound, cut = [int(b) for b in got["bound"]], [int(c) for c in got["cut"]]
    assert sum(cut) == len(recs) and min(cut) >= 1 and max(cut) <= max_records
    at = 0
    for k in cut:
        assert k == 1 or sum(bound[at:at + k]) < max_bytes
        at += k
    assert cut == replay_cut(bound, 0, max_records, max_bytes)
    if max_bytes == 1:                                                # a record whose bound exceeds max_bytes alone is taken, by itself
        starts = np.cumsum([0] + cut)
        assert all(sum(1 for b in bound[starts[k]:starts[k + 1]] if b) <= 1 for k in range(len(cut))) and max(bound) > max_bytes
        assert all(cut[k] == 1 for k in range(len(cut)) if bound[starts[k]])


def test_cut_from_a_later_record(bed_dump, tmp_path):
    recs = bc.random_records(np.random.default_rng(4), 50)
    got = dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS, first=17, max_records=8, max_bytes=2000)])[0]
    assert sum(int(c) for c in got["cut"]) == len(recs) - 17
    assert [int(c) for c in got["cut"]] == replay_cut([int(b) for b in got["bound"]], 17, 8, 2000)


def test_cut_at_the_batch_limit_with_records_described_by_counts(bed_dump, tmp_path):
    """A bound of 2^32 - 64 is refused; one byte less is a batch of its own.  Counts only: no such CIGAR is allocated."""
    fixed = 4 * 10 + 2 + 3 + 1 + 7 + 10 + 12 + len(bc.REFS[0])            # bed_line_bound without the name and the blocks
    n_ops = (BATCH_BYTES - fixed) // 22 - 1
    name_at = BATCH_BYTES - fixed - 22 * (n_ops + 1)                      # the name length at which the bound is 2^32 - 64
    assert 0 < name_at <= 254
    cases = [counts_case_bytes([3, n_ops, 2], [4, name_at - 1, 4], bc.REFS), counts_case_bytes([3, n_ops, 2], [4, name_at, 4], bc.REFS),
             counts_case_bytes([3, n_ops, 2], [4, name_at, 4], bc.REFS, flag=[0, 4, 0]),
             counts_case_bytes([n_ops // 2, n_ops // 2, n_ops // 2], [4, 4, 4], bc.REFS, max_bytes=1 << 40)]
    below, at, unmapped, summed = dump(bed_dump, tmp_path, cases)
    assert int(below["bound"][1]) == BATCH_BYTES - 1 and [int(c) for c in below["cut"]] == [1, 1, 1]
    assert int(at["bound"][1]) == BATCH_BYTES and "cut" not in at
    msg = bytes(at["cut_error"]).decode()
    assert "record 1:" in msg and "beyond one batch" in msg
    assert int(unmapped["bound"][1]) == 0 and [int(c) for c in unmapped["cut"]] == [3]
    assert [int(c) for c in summed["cut"]] == [1, 1, 1]                   # no batch's summed bounds reach 2^32 - 64, whatever max_bytes says


def test_python_bed_cut_equals_the_program(bed_dump, tmp_path):
    recs = bc.random_records(np.random.default_rng(8), 64)
    got = dump(bed_dump, tmp_path, [case_bytes(recs, bc.REFS, max_records=9, max_bytes=1500)])[0]
    flag, tid, pos, mapq, cigars, names = br.columns(recs)
    cut, at = [], 0
    while at < len(recs):
        cut.append(capi.bed_cut(flag, tid, cigars, names, bc.REFS, at, 9, 1500))
        at += cut[-1]
    assert cut == [int(c) for c in got["cut"]]
