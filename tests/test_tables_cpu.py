"""CPU: the annotation's and the junction table's tables (lr2rmats_amd/csrc/l2r_tables.hip.h -- site dictionaries with their parts, bucket
and reach-back directories, cursor keys and their directory, TX_MONO / TX_COMPACT, the junction directories, the two host cursors, the
cache file) against their restatement (tests/tables_restatement.py), member by member and exactly: everything is integers.

tests/tables_dump.hip is the tables as a stand-alone host program (`make -C lr2rmats_amd/csrc tables-dump`: ASan + UBSan on the host code,
no HIP call, no GPU).  Every case is the smallest input at which one rule of the tables can go wrong; a report of either sanitizer fails
the case."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import tables_restatement as tr
from tests import window_cases as wc
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
TABLES_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "tables_dump")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEAD_BYTES, HEAD_N = 144, 16                                      # CacheHead: its size, and where its twelve lengths begin


def build_tables_dump():
    """The program's path, built where it is not (tests/test_gpu_parity.py runs it too); skips without hipcc."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "tables-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return TABLES_DUMP


@pytest.fixture(scope="module")
def tables_dump():
    return build_tables_dump()


class Case:
    """txs: (tid, rev, [(start, end), ...]) in file order, the header's span that of the exons unless (.., start, end) says otherwise -- or
    the seven arrays of an annotation by name;
    sj: rows (tid, don, acc, unique, multi); reads: (tid, pos) and, with `moves`, which of them reach the junction check.  `arrays`
    replaces named arrays of the annotation (the cases the engine rejects)."""

    def __init__(self, txs=None, sj=None, reads=(), moves=None, starts=(0, 0), **arrays):
        self.anno = None
        if isinstance(txs, dict):
            self.anno = dict(txs)
        elif txs is not None:
            off = np.cumsum([0] + [len(t[2]) for t in txs])
            self.anno = dict(tx_tid=[t[0] for t in txs], tx_start=[t[3] if len(t) > 3 else t[2][0][0] for t in txs],
                             tx_end=[t[4] if len(t) > 3 else t[2][-1][1] for t in txs], tx_rev=[t[1] for t in txs], tx_ex_off=list(off),
                             ex_start=[e[0] for t in txs for e in t[2]], ex_end=[e[1] for t in txs for e in t[2]])
            self.anno.update(arrays)
        self.sj = None if sj is None else [[r[k] for r in sj] for k in range(5)]
        self.reads = list(reads)
        self.moves = [1] * len(self.reads) if moves is None else list(moves)
        self.starts = starts

    def write(self, path):
        a, s = self.anno, self.sj
        head = [int(a is not None), len(a["tx_tid"]) if a else 0, len(a["ex_start"]) if a else 0, int(s is not None), len(s[0]) if s else 0,
                len(self.reads), self.starts[0], self.starts[1], 0, 0, 0, 0]
        with open(path, "wb") as fh:
            fh.write(struct.pack("<12q", *head))
            if a:
                for name, typ in (("tx_tid", "<i4"), ("tx_start", "<i4"), ("tx_end", "<i4"), ("tx_rev", "u1"), ("tx_ex_off", "<i8"), ("ex_start", "<i4"), ("ex_end", "<i4")):
                    fh.write(np.asarray(a[name], typ).tobytes())
            if s:
                for col in s:
                    fh.write(np.asarray(col, "<i4").tobytes())
            fh.write(np.asarray([r[0] for r in self.reads], "<i4").tobytes()); fh.write(np.asarray([r[1] for r in self.reads], "<i4").tobytes())
            fh.write(np.asarray(self.moves, "u1").tobytes())

    def restated(self):
        out = {}
        tid, pos = [r[0] for r in self.reads], [r[1] for r in self.reads]
        if self.anno:
            out.update(tr.annotation_tables(**self.anno))
            if self.reads:
                out["anno_after"] = [tr.cursor_after(out["key"], t, p) for t, p in self.reads]
                out["anno_replay"], out["anno_replay_end"] = tr.cursor_replay(out["key_raw"], self.starts[0], tid, pos)
        if self.sj and self.sj[0]:
            out.update(tr.junction_tables(*self.sj))
            if self.reads:
                out["sj_after"] = [tr.cursor_after(out["sj_key"], t, p) for t, p in self.reads]
                out["sj_replay"], out["sj_replay_end"] = tr.cursor_replay(out["sj_key_raw"], self.starts[1], tid, pos, self.moves)
        elif self.sj:
            out.update(sj_key=[], sj_key_raw=[], sj_cbase=[], sj_cdir=[], sj_dbase=[], sj_ddir=[], sj_row=[], sj_ntid=0)
        return out


def _entries(words):
    """SiteEnt as the restatement has it: (k1, k2, tx_base, flags, pair mask, single mask)"""
    w = np.asarray(words, "<u4").reshape(-1, 8)
    s = w.view("<i4")
    return [(int(s[i, 0]), int(s[i, 1]), int(s[i, 2]), int(w[i, 3]), int(w[i, 4]) | int(w[i, 5]) << 32, int(w[i, 6]) | int(w[i, 7]) << 32) for i in range(len(w))]


def _dump(exe, case, tmp_path, cache=None):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "tables.bin")
    case.write(src)
    env = dict(os.environ)
    env.update(SAN_ENV)
    r = subprocess.run([exe, src, dst] + ([str(cache)] if cache else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    for m in MARKS:
        assert m not in r.stderr, "sanitizer report\n" + r.stderr.decode(errors="replace")[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-1500:])
    got = _read_dump(dst)
    for name in ("st_ent", "en_ent"):
        if name in got:
            got[name] = _entries(got[name])
    return got


def _compare(exe, case, tmp_path, cache=None):
    """Every member the program wrote against the restatement, exactly; returns the restatement (with the cache state, where there is one)."""
    got, want = _dump(exe, case, tmp_path, cache), case.restated()
    assert int(got.pop("rc")[0]) == 0
    state = int(got.pop("state")[0]) if cache else None
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, v in got.items():
        w = want[name]
        if name in ("st_ent", "en_ent"):
            assert v == w, name
        elif isinstance(w, list):
            assert [int(x) for x in v] == w, name
        else:
            assert len(v) == 1 and int(v[0]) == int(w), (name, int(v[0]), w)
    if cache:
        want["state"] = state
    return want


def _fill(n, tid=0):
    """n transcripts of one exon: they take a place in the file order and enter no dictionary"""
    return [(tid, 0, [(50, 60)])] * n


# ---- parts
@pytest.mark.parametrize("gap", [63, 64])
def test_members_63_and_64_transcripts_apart(tables_dump, tmp_path, gap):
    # the exon (2000, 2100) is the second of transcript 0 and of transcript `gap`: pair members and acceptors of one START key
    txs = [(0, 0, [(1000, 1100), (2000, 2100)])] + _fill(gap - 1) + [(0, 1, [(500, 600), (2000, 2100)])]
    t = _compare(tables_dump, Case(txs), tmp_path)
    both = 1 | 1 << 63
    if gap == 63:
        assert t["st_ent"] == [(500, 600, 63, 0, 1, 0), (1000, 1100, 0, 0, 1, 0), (2000, 2100, 0, 0, both, both)] and t["n_wide"] == 0
    else:
        assert t["st_ent"] == [(500, 600, 64, 0, 1, 0), (1000, 1100, 0, 0, 1, 0), (2000, 2100, 0, tr.SE_WIDE, 1, 1), (2000, 2100, 64, tr.SE_WIDE, 1, 1)]
        assert t["n_wide"] == 1 and t["st_dir"][-1] == 4
    assert [e[3] for e in t["en_ent"]] == [0, 0]


def test_far_member_of_the_other_kind_and_keys_that_share_k1(tables_dump, tmp_path):
    # (2000, 2100): pairs 0 and 1, acceptors 0, 1 and 64; (2000, 2500): pair 64, the same acceptors -- the singles belong to both keys,
    # and in each the member 64 transcripts on is of the other kind than the near ones
    txs = [(0, 0, [(1000, 1100), (2000, 2100)])] * 2 + _fill(62) + [(0, 1, [(500, 600), (2000, 2500)])]
    t = _compare(tables_dump, Case(txs), tmp_path)
    W = tr.SE_WIDE
    assert t["st_ent"][2:] == [(2000, 2100, 0, W, 3, 3), (2000, 2100, 64, W, 0, 1), (2000, 2500, 0, W, 0, 3), (2000, 2500, 64, W, 1, 1)]
    assert t["n_wide"] == 2
    # END: two junctions from one donor, 64 transcripts apart
    txs = [(0, 0, [(1000, 1100), (2000, 2100)])] + _fill(63) + [(0, 1, [(1000, 1100), (3000, 3100)])]
    t = _compare(tables_dump, Case(txs), tmp_path)
    assert t["en_ent"] == [(1100, 2000, 0, W, 1, 1), (1100, 2000, 64, W, 0, 1), (1100, 3000, 0, W, 0, 1), (1100, 3000, 64, W, 1, 1)]
    assert t["st_ent"][0] == (1000, 1100, 0, W, 1, 0) and t["n_wide"] == 3


# ---- bucket grid
def test_bucket_grid_ends_with_the_largest_site_or_exon_end(tables_dump, tmp_path):
    for last, buckets in (((511, 511), 1), ((512, 512), 2), ((300, 511), 1), ((300, 512), 2)):
        t = _compare(tables_dump, Case([(0, 0, [(100, 200), last])]), tmp_path)
        assert t["tid_base"] == [0, buckets] and len(t["st_dir"]) == buckets + 1 == len(t["en_dir"]) == len(t["st_rdir"]), last
    assert t["st_dir"] == [0, 2, 2] and t["st_rdir"] == [0, 1, 2]             # ((300, 512) reaches into the bucket its end alone made)


def test_chromosomes_without_buckets_share_the_next_word(tables_dump, tmp_path):
    # chromosome 1: a single-exon transcript only (cursor buckets, no site buckets); chromosome 2: nothing at all
    txs = [(0, 0, [(100, 200), (300, 400)]), (1, 0, [(100, 700)]), (3, 0, [(100, 200), (600, 700)])]
    t = _compare(tables_dump, Case(txs), tmp_path)
    assert t["tid_base"] == [0, 1, 1, 1, 3] and t["n_tid_dir"] == 4
    assert t["kb_base"] == [0, 1, 3, 3, 5] and t["n_tid_key"] == 4 and t["key_dir"] == [0, 1, 1, 2, 2, 3]


# ---- the reach-back directory
def test_rdir_is_lowered_where_an_exon_reaches_in(tables_dump, tmp_path):
    t = _compare(tables_dump, Case([(0, 0, [(100, 200), (600, 1700)])]), tmp_path)
    assert t["st_dir"] == [0, 1, 2, 2, 2] and t["st_rdir"] == [0, 1, 1, 1, 2]
    # two such exons: the earlier entry wins
    t = _compare(tables_dump, Case([(0, 0, [(100, 200), (600, 1700)]), (0, 0, [(100, 200), (700, 1600)])]), tmp_path)
    assert t["st_dir"] == [0, 1, 3, 3, 3] and t["st_rdir"] == [0, 1, 1, 1, 3]
    # an exon whose key has parts: its first part
    t = _compare(tables_dump, Case([(0, 0, [(100, 200), (600, 1700)])] + _fill(63) + [(0, 0, [(300, 400), (600, 1700)])]), tmp_path)
    assert [e[:3] for e in t["st_ent"]] == [(100, 200, 0), (300, 400, 64), (600, 1700, 0), (600, 1700, 64)]
    assert t["st_dir"] == [0, 2, 4, 4, 4] and t["st_rdir"] == [0, 2, 2, 2, 4]


# ---- transcripts that enter no dictionary, TX_COMPACT
def test_transcripts_without_sites_and_the_conditions_of_compact(tables_dump, tmp_path):
    two = [(100, 200), (300, 400)]
    txs = [(0, 0, two),                                   # compact
           (0, 0, [(100, 200), (100, 400)]),              # exon starts do not rise: not even TX_MONO
           (0, 0, [(100, 200), (300, 250)]),              # an exon that ends before it begins
           (-1, 0, two),                                  # no chromosome
           (0, 0, [(100, 200)]),                          # one exon
           (0, 0, two, 90, 400), (0, 0, two, 100, 410)]   # the header's span is not the exons'
    t = _compare(tables_dump, Case(txs), tmp_path)
    assert t["hdr"][6::12] == [3, 0, 1, 1, 1, 1, 1] and t["n_compact"] == 1
    assert t["key_raw"][3] == 400 and t["key_raw"][0] == (1 << 32) | 400          # (tid + 1: a transcript without chromosome sorts first)
    # only the transcripts with a chromosome and two exons have sites: 0, 1, 2, 5, 6
    members = 0
    for e in t["st_ent"] + t["en_ent"]:
        members |= e[4] << e[2]
    assert members == 0b1100111
    # nothing but such transcripts: headers and cursor keys, no entry, no bucket
    t = _compare(tables_dump, Case([(-1, 1, two), (2, 0, [(100, 200)])]), tmp_path)
    assert t["st_ent"] == [] and t["tid_base"] == [0] and t["st_dir"] == [0] and t["kb_base"] == [0, 0, 0, 1] and t["n_tid_key"] == 3


# ---- cursor keys
def test_cursor_keys_and_their_directory(tables_dump, tmp_path):
    k = lambda end: tr.host_key(0, end)
    t = _compare(tables_dump, Case([(0, 0, [(100, 1000)]), (0, 0, [(200, 500)]), (0, 0, [(300, 1100)])]), tmp_path)
    assert t["key"] == [k(1000), k(1000), k(1100)] and t["key_raw"] == [k(1000), k(500), k(1100)]
    # a bucket's word: the first key at or behind its first base; the closing word
    t = _compare(tables_dump, Case([(0, 0, [(100, 511)]), (0, 0, [(100, 512)]), (0, 0, [(100, 513)]), (1, 0, [(5, 9)])]), tmp_path)
    assert t["kb_base"] == [0, 2, 3] and t["key_dir"] == [0, 1, 3, 4]
    t = _compare(tables_dump, Case([]), tmp_path)
    assert t["hdr"] == [] and t["key"] == [] and t["tid_base"] == [0] and t["kb_base"] == [0] and t["key_dir"] == [0] and t["st_dir"] == [0]


# ---- what the tables reject
_TWO = [(0, 0, [(100, 200), (300, 400)]), (0, 0, [(100, 200), (300, 400)])]
_ROWS = [(0, 100, 200, 1, 0), (0, 100, 300, 1, 0), (1, 50, 60, 1, 0)]


def _swapped(rows, i):
    rows = list(rows)
    rows[i - 1], rows[i] = rows[i], rows[i - 1]
    return rows


@pytest.mark.parametrize("case,message", [
    (Case(_TWO, tx_ex_off=[0, 3, 2]), "[l2r_set_annotation] bad exon offsets at transcript 1"),
    (Case(_TWO, tx_ex_off=[0, 2, 5]), "[l2r_set_annotation] bad exon offsets at transcript 1"),
    (Case(_TWO, tx_ex_off=[-1, 2, 4]), "[l2r_set_annotation] bad exon offsets at transcript 0"),
    (Case(_TWO, tx_ex_off=[0, 4, 4]), "[l2r_set_annotation] transcript 1 has no exon"),
    (Case(_TWO, ex_start=[100, 300, -100, 300]), "[l2r_set_annotation] negative exon coordinate"),
    (Case(sj=_swapped(_ROWS, 2)), "[l2r_set_junctions] rows are not sorted by (tid, don, acc) at row 2"),
    (Case(sj=[(0, 100, 200, 1, 0), (0, 99, 300, 1, 0)]), "[l2r_set_junctions] rows are not sorted by (tid, don, acc) at row 1"),
    (Case(sj=_swapped(_ROWS, 1)), "[l2r_set_junctions] rows are not sorted by (tid, don, acc) at row 1"),
], ids=["offsets_descend", "offsets_past_the_exons", "offsets_negative", "no_exon", "negative_coordinate", "sj_tid", "sj_don", "sj_acc"])
def test_rejected_tables_give_the_engine_message(tables_dump, tmp_path, case, message):
    got = _dump(tables_dump, case, tmp_path)
    assert sorted(got) == ["error", "rc"] and int(got["rc"][0]) == -1
    assert got["error"].tobytes().decode() == message
    with pytest.raises(tr.TablesError) as e:
        case.restated()
    assert str(e.value) == message


# ---- junction directories
def test_junction_directories(tables_dump, tmp_path):
    # rows without a chromosome and a negative donor: keys all the same, no bucket of their own; acceptors at 511 and 512
    rows = [(-1, 5, 9, 1, 0), (0, -7, 511, 2, 1), (0, 100, 512, 3, 0), (0, 200, 90, 4, 0)]
    for n, cbase in ((2, [0, 1]), (3, [0, 2]), (4, [0, 2])):
        t = _compare(tables_dump, Case(sj=rows[:n]), tmp_path)
        assert t["sj_cbase"] == cbase and t["sj_ntid"] == 1, n
    assert t["sj_cdir"] == [1, 2, 4] and t["sj_dbase"] == [0, 1] and t["sj_ddir"] == [1, 4]
    assert t["sj_key"][3] == t["sj_key"][2] == tr.host_key(0, 512) and t["sj_key_raw"][3] == tr.host_key(0, 90)
    assert t["sj_row"][4:8] == [-7, 511, 2, 1]
    t = _compare(tables_dump, Case(sj=[(2, 600, 700, 1, 1)]), tmp_path)
    assert t["sj_cbase"] == [0, 0, 0, 2] and t["sj_cdir"] == [0, 0, 1] and t["sj_dbase"] == [0, 0, 0, 2] and t["sj_ddir"] == [0, 0, 1]
    # the donors where two chromosomes meet: the first chromosome's last bucket ends where the second's rows begin
    rows = [(0, 100, 2000, 1, 0), (0, 600, 700, 1, 0), (0, 1023, 1100, 1, 0), (1, 0, 50, 1, 0), (1, 512, 600, 1, 0)]
    t = _compare(tables_dump, Case(sj=rows), tmp_path)
    assert t["sj_dbase"] == [0, 2, 4] and t["sj_ddir"] == [0, 1, 3, 4, 5]
    assert t["sj_cbase"] == [0, 4, 6] and t["sj_cdir"] == [0, 0, 0, 0, 3, 4, 5]
    # (no table: l2r_set_junctions takes an empty one as none)
    _compare(tables_dump, Case(sj=[]), tmp_path)


# ---- the two host cursors
def _literal_replay(items, reads, start=0, moves=None):
    """check_trans(): the cursor steps while the item under it lies before the read -- on a smaller chromosome, or on the same and ending
    at or before the read's first base (pos is 0-based) -- one read after the other; a read that does not reach the check leaves it alone."""
    cur, seen = start, []
    for i, (tid, pos) in enumerate(reads):
        if moves is not None and not moves[i]:
            seen.append(0)
            continue
        while cur < len(items) and (items[cur][0] < tid or (items[cur][0] == tid and items[cur][1] <= pos + 1)):
            cur += 1
        seen.append(cur)
    return seen, cur


_CUR_TXS = [(0, 0, [(150, 300)]), (0, 0, [(100, 900)]), (0, 0, [(200, 250), (400, 500)]), (0, 0, [(600, 700)]), (1, 0, [(10, 20)]), (1, 0, [(30, 800)]), (3, 0, [(5, 6)])]
_CUR_SJ = [(0, 100, 900, 1, 0), (0, 150, 300, 1, 0), (0, 200, 500, 1, 0), (1, 5, 20, 1, 0), (1, 6, 800, 1, 0), (3, 1, 6, 1, 0)]
_CUR_SORTED = [(0, 0), (0, 248), (0, 249), (0, 298), (0, 299), (0, 499), (0, 898), (0, 899), (0, 5000), (1, 0), (1, 19), (2, 7), (3, 5), (4, 0)]


def test_cursors_against_a_literal_replay(tables_dump, tmp_path):
    ends = [(t[0], t[2][-1][1]) for t in _CUR_TXS]
    accs = [(r[0], r[2]) for r in _CUR_SJ]
    # sorted reads: the cursor behind a sorted upload is what the replay has reached at its last read
    moves = [i % 3 != 1 for i in range(len(_CUR_SORTED))]
    t = _compare(tables_dump, Case(_CUR_TXS, _CUR_SJ, _CUR_SORTED, moves), tmp_path)
    assert t["anno_after"] == _literal_replay(ends, _CUR_SORTED)[0] == t["anno_replay"]
    assert t["sj_after"] == _literal_replay(accs, _CUR_SORTED)[0]
    assert (t["sj_replay"], t["sj_replay_end"]) == _literal_replay(accs, _CUR_SORTED, 0, moves)
    assert t["anno_after"] == [0, 0, 0, 0, 1, 1, 1, 4, 4, 4, 5, 6, 7, 7]
    # reads that go backwards: the replayed cursor never does, and an upload that continues another starts where that one ended
    back = [_CUR_SORTED[i] for i in (4, 0, 9, 2, 12, 1, 13, 5)]
    moves = [1, 0, 1, 1, 0, 1, 1, 1]
    for starts in ((0, 0), (2, 1), (7, 6)):
        t = _compare(tables_dump, Case(_CUR_TXS, _CUR_SJ, back, moves, starts), tmp_path)
        assert (t["anno_replay"], t["anno_replay_end"]) == _literal_replay(ends, back, starts[0])
        assert (t["sj_replay"], t["sj_replay_end"]) == _literal_replay(accs, back, starts[1], moves)
    assert t["anno_after"] != t["anno_replay"]


# ---- the model of tests/window_cases.py says the same
@pytest.mark.parametrize("family,name", [("window", "win_63_gapped"), ("slice", "st_168_m40")])
def test_entry_keys_and_cursor_agree_with_the_window_cases(tables_dump, tmp_path, family, name):
    case = wc.case(family, name)
    tid, pos = case.rows[len(case.rows) // 2][:2]
    t = _compare(tables_dump, Case(case.txs, reads=[(tid, pos)]), tmp_path)
    st, en, nb = wc._dictionaries(case.txs)
    assert [(0, e[0], e[1]) for e in t["st_ent"]] == st and [(0, e[0], e[1]) for e in t["en_ent"]] == en
    assert list(np.diff(t["tid_base"])) == [nb[0]]
    assert t["anno_after"] == [wc.window(case.txs, tid, pos + 1, pos + 2)[0]]


# ---- the cache file
_CACHE_TXS = [(0, 0, [(100, 200), (600, 1700)])] + _fill(63) + [(0, 1, [(300, 400), (600, 1700)]), (-1, 0, [(5, 6), (8, 9)]), (2, 1, [(1000, 1100), (1200, 1300)])]


def _cut(raw, n):
    return raw[:n]


def _flip(raw, at, by=1):
    return raw[:at] + bytes([raw[at] ^ by]) + raw[at + 1:]


def _length_word(raw, k, value):
    at = HEAD_N + 8 * k
    old = struct.unpack_from("<Q", raw, at)[0]
    return raw[:at] + struct.pack("<Q", old + 1 if value is None else value) + raw[at + 8:]


def test_cache_file_is_read_back_or_ignored(tables_dump, tmp_path):
    case = Case(_CACHE_TXS)
    _compare(tables_dump, case, tmp_path)
    cache = tmp_path / "cache"
    first = _compare(tables_dump, case, tmp_path, cache)
    files = os.listdir(cache)
    assert first["state"] == 1 and len(files) == 1 and files[0].startswith("l2r_anno_") and files[0].endswith(".tables")
    path = cache / files[0]
    good = path.read_bytes()
    again = _compare(tables_dump, case, tmp_path, cache)
    assert again["state"] == 2 and path.read_bytes() == good
    assert len(good) > HEAD_BYTES and good[:8] == b"L2RANNO3"
    # a file made for another annotation, under this one's name
    other = tmp_path / "other"
    _compare(tables_dump, Case(_CACHE_TXS[:-1]), tmp_path, other)
    foreign = (other / os.listdir(other)[0]).read_bytes()
    assert foreign != good
    damaged = dict(cut_by_a_byte=_cut(good, len(good) - 1), half_a_header=_cut(good, HEAD_BYTES // 2), payload_byte=_flip(good, HEAD_BYTES + 100),
                   one_more_entry=_length_word(good, 4, None), huge_length=_length_word(good, 5, 0x7ffffff1), magic=_flip(good, 7), foreign=foreign)
    for what, raw in damaged.items():
        path.write_bytes(raw)
        t = _compare(tables_dump, case, tmp_path, cache)
        assert t["state"] == 1, what                        # (and every member is the restatement's: _compare)
        assert path.read_bytes() == good and os.listdir(cache) == files, what
