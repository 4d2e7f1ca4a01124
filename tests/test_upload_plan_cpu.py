"""CPU: the upload's plan (lr2rmats_amd/csrc/l2r_plan.hip.h -- sortedness, exon sample, reads per tile, tile cut, slab layout, tile
records, the summary-made tile index, super-block sums) against its restatement (tests/upload_plan_restatement.py), member by member
and exactly: everything is integers but `est`, which both sides make with the same three double operations.

tests/plan_dump.hip is the plan as a stand-alone host program (`make -C lr2rmats_amd/csrc plan-dump`: ASan + UBSan on the host code, no
HIP call, no GPU).  Every case is the smallest input at which one rule of the plan can go wrong; a report of either sanitizer fails
the case."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import upload_plan_restatement as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
PLAN_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "plan_dump")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:halt_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
MARKS = (b"AddressSanitizer", b"runtime error:", b"LeakSanitizer", b"UndefinedBehaviorSanitizer")
M, I, D, N_ = 0, 1, 2, 3                                          # CIGAR operations


@pytest.fixture(scope="module")
def plan_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "plan-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return PLAN_DUMP


class Case:
    """Records as (tid, pos, [(length, op), ...]); summaries, where a case has them, as three words per record."""

    def __init__(self, records, summary=None, cig_off=None, n_cigar_words=None, **opts):
        self.tid = [r[0] for r in records]
        self.pos = [r[1] for r in records]
        self.cig = [(ln << 4) | op for r in records for ln, op in r[2]]
        self.cig_off = list(np.cumsum([0] + [len(r[2]) for r in records])) if cig_off is None else cig_off
        if n_cigar_words is not None:                             # (a case whose cig_off does not span the words)
            self.cig = self.cig + [16] * (n_cigar_words - len(self.cig))
        self.summary = summary
        self.opts = opts

    def write(self, path):
        o = self.opts
        head = [len(self.tid), len(self.cig), int(self.summary is not None), o.get("min_intron", 3), o.get("max_delet", 50),
                int(o.get("want_slab", True)), int(o.get("want_index", True)), int(o.get("stream_sorted", True)),
                o.get("last_key", ur.INT64_MIN), o.get("exb", -1) if o.get("exb") is not None else -1, 0, 0]
        with open(path, "wb") as fh:
            fh.write(struct.pack("<12q", *head))
            fh.write(np.asarray(self.tid, "<i4").tobytes()); fh.write(np.asarray(self.pos, "<i4").tobytes())
            fh.write(np.asarray(self.cig_off, "<i8").tobytes()); fh.write(np.asarray(self.cig, "<u4").tobytes())
            if self.summary is not None:
                fh.write(np.asarray(self.summary, "<u4").reshape(-1).tobytes())

    def restated(self):
        return ur.upload_plan(self.tid, self.pos, self.cig_off, self.cig, self.summary, **self.opts)


def _read_dump(path):
    out = {}
    with open(path, "rb") as fh:
        while True:
            head = fh.read(40)
            if not head:
                return out
            name, typ = head[:24].split(b"\0")[0].decode(), head[24:32].split(b"\0")[0].decode()
            count = struct.unpack("<q", head[32:])[0]
            out[name] = np.frombuffer(fh.read(count * np.dtype(typ).itemsize), typ)


def _engine_plan(exe, case, tmp_path):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "plan.bin")
    case.write(src)
    env = dict(os.environ)
    env.update(SAN_ENV)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    for m in MARKS:
        assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
    return _read_dump(dst)


def _compare(exe, case, tmp_path):
    """Every member the program wrote against the restatement, exactly; returns the restatement."""
    got, want = _engine_plan(exe, case, tmp_path), case.restated()
    assert int(got.pop("rc")[0]) == 0
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, v in got.items():
        w = want[name]
        if name == "est":
            assert float(v[0]) == w, (name, float(v[0]), w)
        elif isinstance(w, (list, np.ndarray)):
            assert [int(x) for x in v] == [int(x) for x in w], name
        else:
            assert len(v) == 1 and int(v[0]) == int(w), (name, int(v[0]), w)
    return want


def _mi(n_ops, length=10):
    """A CIGAR of n_ops operations without a cut: M I M I ... (n_ops odd: ends with M)."""
    return [(length, M if k % 2 == 0 else I) for k in range(n_ops)]


def _cuts(n_cuts, length=10):
    """A CIGAR of n_cuts + 2 operations with n_cuts cuts: M, then N operations, then M."""
    return [(length, M)] + [(length, N_)] * n_cuts + [(length, M)]


def _rows(p):
    return list(np.diff(p["sbase"]) // ur.SLAB_STRIDE)


# ---- empty and single input
def test_empty_and_single_upload(plan_dump, tmp_path):
    p = _compare(plan_dump, Case([]), tmp_path)
    assert p["tile_first"] == [0, 0] and p["n_tiles"] == 0 and p["slab_ok"] and not p["have_index"] and p["sorted"]
    p = _compare(plan_dump, Case([(2, 77, [(50, M)])]), tmp_path)
    assert p["tile_first"] == [0, 1] and p["n_tiles"] == 1 and p["have_index"] and _rows(p) == [2]
    assert list(p["rec"][:6]) == [0, 1, 0, 2, 2, 78]


# ---- the 256-read limit, the chromosome change
def test_tile_ends_at_256_reads_and_at_a_chromosome_change(plan_dump, tmp_path):
    one = [(0, 100 + k, [(50, M)]) for k in range(257)]
    assert _compare(plan_dump, Case(one[:256]), tmp_path)["tile_first"] == [0, 256]
    p = _compare(plan_dump, Case(one), tmp_path)
    assert p["tile_first"] == [0, 256, 257] and p["n_tiles256"] == 2
    two = [(0, 100 + k, [(50, M)]) for k in range(100)] + [(1, 5 + k, [(50, M)]) for k in range(100)]
    assert _compare(plan_dump, Case(two), tmp_path)["tile_first"] == [0, 100, 200]
    # (unsorted records: plain runs, whatever the chromosome; no slab layout)
    p = _compare(plan_dump, Case(two[::-1]), tmp_path)
    assert p["tile_first"] == [0, 200] and not p["sorted"] and not p["slab_layout"]


# ---- TILE_POS_CAP
def test_tile_ends_where_the_exon_bounds_exceed_the_staged_positions(plan_dump, tmp_path):
    # 200 reads of 21 operations: (21 + 3) >> 1 = 12 each, 2400 = TILE_POS_CAP in all
    assert 200 * 12 == ur.TILE_POS_CAP
    fit = [(0, 100, _mi(21)) for _ in range(200)]
    p = _compare(plan_dump, Case(fit), tmp_path)
    assert p["tile_first"] == [0, 200] and p["reads_per_tile"] == 256
    # ... the last of them with 23 operations: one position too many
    p = _compare(plan_dump, Case(fit[:199] + [(0, 100, _mi(23))]), tmp_path)
    assert p["tile_first"] == [0, 199, 200]
    # (without the slab layout the bound does not cut)
    assert _compare(plan_dump, Case(fit[:199] + [(0, 100, _mi(23))], want_slab=False), tmp_path)["tile_first"] == [0, 200]


# ---- SLAB_TILE_SPAN
def test_tile_ends_where_reads_begin_2_17_bases_apart(plan_dump, tmp_path):
    def reads(gap):
        return [(0, 1000, [(50, M)])] + [(0, 1000 + gap, [(50, M)]) for _ in range(9)]
    assert _compare(plan_dump, Case(reads(ur.TILE_SPAN - 1)), tmp_path)["tile_first"] == [0, 10]
    assert _compare(plan_dump, Case(reads(ur.TILE_SPAN)), tmp_path)["tile_first"] == [0, 1, 10]
    # the classic layout: the cut waits for 8 reads
    assert _compare(plan_dump, Case(reads(ur.TILE_SPAN - 1), want_slab=False), tmp_path)["tile_first"] == [0, 10]
    assert _compare(plan_dump, Case(reads(ur.TILE_SPAN), want_slab=False), tmp_path)["tile_first"] == [0, 8, 10]


# ---- SLAB_ROWS
def test_slab_rows_and_the_outlier(plan_dump, tmp_path):
    short = [(0, 100, [(50, M)]) for _ in range(10)]
    assert (45 + 3) >> 1 == ur.SLAB_ROWS and (47 + 3) >> 1 == ur.SLAB_ROWS + 1
    p = _compare(plan_dump, Case(short + [(0, 100, _mi(45))]), tmp_path)
    assert not p["wide_cigar"] and _rows(p) == [ur.SLAB_ROWS] and p["dense_rows"] == 10 * 2 + 46
    # one row more than a slab has: an outlier -- the tile's rows do not grow, the dense area has room for it
    p = _compare(plan_dump, Case(short + [(0, 100, _mi(47))]), tmp_path)
    assert not p["wide_cigar"] and _rows(p) == [2] and p["dense_rows"] == 10 * 2 + 48
    assert p["slab_total"] == 2 * ur.SLAB_STRIDE and list(p["rec"][:4]) == [0, 11, 0, 2]


# ---- wide_cigar, many_exon_reads
def test_wide_cigar_and_many_exon_reads(plan_dump, tmp_path):
    p = _compare(plan_dump, Case([(0, 100, _mi(32)) for _ in range(4)]), tmp_path)
    assert not p["wide_cigar"] and p["slab_tiles"] and p["make_index"]
    # one operation more in 4 reads: long CIGARs -- SLAB_ROWS rows per tile, the dense area as large as the counted bound, no index
    p = _compare(plan_dump, Case([(0, 100, _mi(32)) for _ in range(3)] + [(0, 100, _mi(33))], exb=77), tmp_path)
    assert p["wide_cigar"] and p["slab_long"] and not p["slab_tiles"] and not p["make_index"] and not p["have_index"]
    assert _rows(p) == [ur.SLAB_ROWS] and p["dense_rows"] == 77
    # 200 reads of long CIGARs, one of them with 25 exons (more than a slab has rows): 0.5 % of the sample exactly -- a rarity
    rich = (0, 100, [(10, M)] + [(10, N_), (10, M)] * 24)
    base = [(0, 100, _mi(33)) for _ in range(200)]
    p = _compare(plan_dump, Case(base[:199] + [rich], exb=1000), tmp_path)
    assert p["wide_cigar"] and not p["many_exon_reads"] and p["slab_long"] and p["slab_ok"]
    # ... two of them: the classic layout
    p = _compare(plan_dump, Case(base[:198] + [rich, rich], exb=1000), tmp_path)
    assert p["wide_cigar"] and p["many_exon_reads"] and not p["slab_layout"] and not p["slab_ok"]


# ---- reads per tile
def test_exon_estimate_halves_the_tile(plan_dump, tmp_path):
    # est * reads * 1.25 against LDS_EXON_CAP = 3072: 256 reads hold up to 9.6 exons per read, 128 up to 19.2
    for n_cuts, rpt in ((8, 256), (9, 128), (18, 128), (19, 64)):
        p = _compare(plan_dump, Case([(0, 100, _cuts(n_cuts)) for _ in range(40)]), tmp_path)
        assert p["est"] == n_cuts + 1.0 and p["reads_per_tile"] == rpt and not p["wide_cigar"], (n_cuts, p["est"], p["reads_per_tile"])
    # 9.6 itself, as nearly as 43 cuts in 5 reads say it: whatever the doubles make of it, both sides make the same
    _compare(plan_dump, Case([(0, 100, _cuts(c)) for c in (9, 9, 9, 8, 8)]), tmp_path)
    # a shorter N or a D within the thresholds does not cut; a longer D does
    p = _compare(plan_dump, Case([(0, 100, [(10, M), (2, N_), (10, M), (50, D), (10, M), (51, D), (10, M)])]), tmp_path)
    assert p["est"] == 2.0


def test_sparse_windows_pick_128_reads_on_the_classic_layout(plan_dump, tmp_path):
    # two windows of 256 reads whose first 128 reads sit together and whose other 128 begin 200 kb further on: every window is bad
    # for 256 reads (30 x the cost) and good for 128 (1.6 x)
    recs = [(0, w * 400000 + (200000 if k >= 128 else 0) + 1000, [(50, M)]) for w in range(2) for k in range(256)]
    p = _compare(plan_dump, Case(recs, want_slab=False), tmp_path)
    assert p["reads_per_tile"] == 128 and p["tile_first"] == [0, 128, 256, 384, 512]
    # (the slab layout cuts tile by tile instead)
    p = _compare(plan_dump, Case(recs), tmp_path)
    assert p["reads_per_tile"] == 256 and p["tile_first"] == [0, 128, 256, 384, 512]


# ---- the summary-made index
def _summ(ref_len=50, n_n=0, min_n=0xffff, max_d=0, min_seg=0xffff):
    return (ref_len, n_n | (min_n << 16), max_d | (min_seg << 16))


def test_summaries_never_exact_at_255_exons(plan_dump, tmp_path):
    recs = [(0, 100, [(50, M)]), (0, 100, [(50, M)]), (1, 100, [(50, M)]), (1, 100, [(50, M)])]
    summ = [_summ(), _summ(n_n=253, min_n=40, min_seg=7), _summ(), _summ(n_n=254, min_n=40, min_seg=7)]
    p = _compare(plan_dump, Case(recs, summ), tmp_path)
    assert p["tile_first"] == [0, 2, 4] and p["nn"] == [0, 253, 0, 254]
    assert p["tile_stat"] == [253, 40, 0, 7, 254, 40, 0, ur.INT32_MIN]
    assert p["sup_stat"] == [253 + 254 + 4, 40, 0, ur.INT32_MIN]


def test_summaries_never_exact_at_the_slot_limit(plan_dump, tmp_path):
    # 17 reads of 240 exons and one of 15: 4095 = SLOT_LOC_LIMIT - 1 exons; one exon more
    for last, min_seg in ((14, 9), (15, ur.INT32_MIN)):
        recs = [(0, 100, [(50, M)]) for _ in range(18)]
        summ = [_summ(n_n=239, min_n=30, min_seg=9) for _ in range(17)] + [_summ(n_n=last, min_n=30, min_seg=9)]
        assert 17 * 240 + last + 1 == ur.SLOT_LOC_LIMIT - (1 if last == 14 else 0)
        p = _compare(plan_dump, Case(recs, summ), tmp_path)
        assert p["tile_stat"] == [17 * 239 + last, 30, 0, min_seg]


def test_summaries_longest_d_and_last_base(plan_dump, tmp_path):
    recs = [(0, 100, [(50, M)]), (0, 200, [(50, M)]), (1, ur.INT32_MAX - 10, [(50, M)])]
    summ = [_summ(ref_len=5000, max_d=0xfffe), _summ(ref_len=60, max_d=0xffff), _summ(ref_len=100)]
    p = _compare(plan_dump, Case(recs, summ), tmp_path)
    rec = np.asarray(p["rec"]).reshape(-1, 8)
    assert p["tile_stat"][2] == ur.INT32_MAX and p["tile_stat"][6] == 0           # 65535: that long or longer
    assert list(rec[:, 6]) == [5100, ur.INT32_MAX]                                # the last base beyond 32 bits is clamped
    # (without the tile index the summaries are not looked at; without summaries the statistics are k_tile_index's to make)
    p = _compare(plan_dump, Case(recs, summ, want_index=False), tmp_path)
    assert not p["have_index"] and p["nn"] == [] and p["tile_stat"] == list(ur.EMPTY_STAT) * 2
    p = _compare(plan_dump, Case(recs), tmp_path)
    assert p["have_index"] and p["nn"] == [] and list(np.asarray(p["rec"]).reshape(-1, 8)[:, 6]) == [0, 0]


# ---- super-block sums
def test_super_block_sums_cross_1024_tiles(plan_dump, tmp_path):
    rng = np.random.default_rng(1025)
    recs = [(t, 100, [(50, M)]) for t in range(1025)]
    summ = [_summ(n_n=int(rng.integers(0, 30)), min_n=int(rng.integers(20, 900)), max_d=int(rng.integers(0, 80)), min_seg=int(rng.integers(5, 400)))
            for _ in range(1025)]
    summ[1024] = _summ(n_n=3, min_n=11, max_d=99, min_seg=2)
    p = _compare(plan_dump, Case(recs, summ), tmp_path)
    assert p["n_tiles"] == 1025 and len(p["sup_stat"]) == 8
    assert p["sup_stat"][4:] == [3 + 1, 11, 99, 2]
    assert p["sup_stat"][0] == sum(s[1] & 0xffff for s in summ[:1024]) + 1024


# ---- an upload that continues others
def test_continuation_keeps_or_loses_the_order(plan_dump, tmp_path):
    recs = [(1, 500, [(50, M)]), (1, 600, [(50, M)])]
    p = _compare(plan_dump, Case(recs, stream_sorted=True, last_key=ur.read_key(1, 501)), tmp_path)
    assert p["sorted_here"] and not p["sorted"] and not p["slab_layout"] and p["last_key"] == ur.read_key(1, 600)
    p = _compare(plan_dump, Case(recs, stream_sorted=True, last_key=ur.read_key(1, 500)), tmp_path)
    assert p["sorted"] and p["slab_layout"]
    p = _compare(plan_dump, Case(recs, stream_sorted=False, last_key=ur.read_key(0, 5)), tmp_path)
    assert p["sorted_here"] and not p["sorted"]
    p = _compare(plan_dump, Case([], stream_sorted=True, last_key=ur.read_key(1, 501)), tmp_path)
    assert p["sorted"] and p["last_key"] == ur.read_key(1, 501)


# ---- what the plan rejects
@pytest.mark.parametrize("case,message", [
    (Case([(0, 10, [(50, M)]), (-1, 20, [(50, M)])]), "[l2r_upload_reads] record 1 has no reference (unmapped); the reference aborts on it (bam2gtf.c:100)"),
    (Case([(0, 10, [(50, M)]) for _ in range(3)], cig_off=[0, 2, 1, 3]), "[l2r_upload_reads] cig_off not monotone at 1"),
    (Case([(0, 10, [(50, M)]) for _ in range(3)], n_cigar_words=4), "[l2r_upload_reads] cig_off does not span n_cigar"),
    (Case([(0, 10, [(50, M)]) for _ in range(3)], cig_off=[1, 2, 3, 3]), "[l2r_upload_reads] cig_off does not span n_cigar"),
], ids=["no_reference", "descending_cig_off", "cig_off_short_of_n_cigar", "cig_off_not_from_0"])
def test_rejected_records_give_the_engine_message(plan_dump, tmp_path, case, message):
    got = _engine_plan(plan_dump, case, tmp_path)
    assert sorted(got) == ["error", "rc"] and int(got["rc"][0]) == -1
    assert got["error"].tobytes().decode() == message
    with pytest.raises(ur.PlanError) as e:
        case.restated()
    assert str(e.value) == message


# ---- the two forms of the tile cut in the restatement agree (tests/test_gpu_tile_split.py tunes its thresholds against the first)
def test_restated_tile_cuts_agree():
    from lr2rmats_amd import synth
    anno = synth.make_annotation(1500, 11)
    reads = synth.make_reads(anno, 2500, 5, 12)
    p = ur.upload_plan(reads.tid, reads.pos, reads.cig_off, reads.cig, synth.cigar_summary(reads.cig_off, reads.cig))
    firsts = ur._tile_firsts(reads)
    assert p["slab_tiles"] and p["reads_per_tile"] == ur.TILE_READS and list(firsts) == p["tile_first"]
    st = ur._tile_stats(reads, firsts)
    assert [int(v) for v in np.stack(st[:4], 1).reshape(-1)] == p["tile_stat"]
