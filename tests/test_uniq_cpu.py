"""`unique-gtf`'s merge_trans, the parts that need no GPU: the host side of l2r_uniq_merge -- the argument checks, the route test, the
cluster cut and the exact host routine uniq_host -- as a stand-alone program under ASan + UBSan (tests/uniq_dump.hip,
`make -C lr2rmats_amd/csrc uniq-dump`) against tests/uniq_restatement.py, against the hand-derived answers of tests/golden/hand, and
against the command's own host loop (host/tail.c m_merge) through `unique-gtf -m g` without a device."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi, hostlib
from tests import uniq_cases as uc
from tests import uniq_restatement as ur
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNIQ_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "uniq_dump")
HAND = os.path.join(ROOT, "tests", "golden", "hand")
ARRAYS = ("merged", "uniq_of", "u_src", "u_start", "u_end", "u_cov")
CASES = dict(uc.cases(), **uc.tile_cases())


@pytest.fixture(scope="module")
def uniq_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "uniq-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return UNIQ_DUMP


def case_bytes(trans, s=0, d=0, D=ur.INT_MAX, f=0.8, columns=None, n=None):
    tid, rev, ex_off, xs, xe = columns if columns is not None else ur.columns(trans)
    bits = int(np.asarray(f, np.float32).view(np.uint32))
    head = struct.pack("<8q", len(tid) if n is None else n, len(xs), s, d, D, bits, len(ex_off), 0)
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in (tid, rev, ex_off, xs, xe))


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


def check(got, trans, opts, name=""):
    want = ur.merge(trans, **opts)
    assert int(got["rc"][0]) == 0
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), (name, k, got[k][:20], want[k][:20])
    assert np.array_equal(got["hits"], want["hits"]) and int(got["end_ext"][0]) == want["end_ext"], name
    assert int(got["in_order"][0]) == int(ur.in_order(trans)), name
    if ur.in_order(trans):
        heads = ur.heads(trans)
        assert np.array_equal(got["head"], heads), (name, got["head"][:20], heads[:20])
        firsts = list(np.flatnonzero(heads)) + [len(trans)]
        assert int(got["n_clusters"][0]) == int(heads.sum()) and int(got["largest"][0]) == (max(np.diff(firsts)) if len(trans) else 0), name
    return want


def test_the_tile_constant():
    assert capi.header_define("L2R_UNIQ_PMAX_TILE") == uc.TILE


# ---------------------------------------------------------------------------------------------------- the restatement by hand

def test_restatement_on_the_cases_derived_by_hand():
    """What the cases are built to show, written down from the rule (not from a program's output)."""
    c = uc.cases()
    r = ur.merge(*_args(c["mutation_forward"]))
    assert (list(r["merged"]), list(r["u_start"]), list(r["u_end"]), list(r["u_cov"])) == ([0, 1, 1, 1], [100], [1030], [4]) and r["end_ext"] == 2
    r = ur.merge(*_args(c["early_stop"]))
    assert list(r["merged"]) == [0, 0, 0] and list(r["u_src"]) == [0, 1, 2]
    r = ur.merge(*_args(c["strand_between"]))
    assert (list(r["merged"]), list(r["uniq_of"])) == ([0, 0, 1, 0, 0, 1], [0, 1, 0, 2, 3, 2])
    r = ur.merge(*_args(c["strand_free"]))
    assert (list(r["merged"]), list(r["uniq_of"])) == ([0, 1, 1, 0, 1, 1], [0, 0, 0, 1, 1, 1])
    r = ur.merge(*_args(c["mixed_counts"]))
    assert list(r["merged"]) == [0, 0, 1, 1, 0] and list(r["u_cov"]) == [2, 2, 1]
    r = ur.merge(*_args(c["contained"]))
    assert list(r["merged"]) == [0, 1, 1, 0, 0, 0, 1, 1] and list(r["hits"]) == [0, 4, 0] and list(r["u_cov"]) == [1, 1, 1, 1]
    r = ur.merge(*_args(c["inner_walk_first_fit"]))
    assert list(r["merged"]) == [0, 0]
    for name, merged in (("D_at", [0, 1, 0, 0, 1]), ("D_beyond", [0, 0, 0, 0, 0]), ("d_at", [0, 1, 1, 0, 1]), ("d_beyond", [0, 1, 0, 0, 1])):
        assert list(ur.merge(*_args(c[name]))["merged"]) == merged, name
    assert list(ur.heads(c["cluster_edge"][0])) == [1, 0, 0, 1, 0]
    assert list(ur.heads(c["chromosome_change"][0])) == [1, 0, 1, 0, 1]
    assert list(ur.merge(*_args(c["chromosome_change"]))["merged"]) == [0, 1, 0, 1, 0]
    for k in (64, 65, 128, 129):
        trans, targets = uc.lane_round_case(k)
        r = ur.merge(trans)
        assert len(r["u_src"]) == k and list(r["uniq_of"][k:]) == targets and list(np.flatnonzero(r["u_cov"] == 2)) == targets
        assert int(ur.heads(trans).sum()) == 1
    assert int(ur.heads(c["own_clusters"][0]).sum()) == 2 * uc.TILE + 1 and int(ur.heads(c["one_cluster"][0]).sum()) == 1


def _args(case):
    trans, o = case
    return trans, o.get("s", 0), o.get("d", 0), o.get("D", ur.INT_MAX), o.get("f", 0.8)


def test_the_single_exon_fraction_is_compared_as_float():
    trans, r, above, below = uc.fraction_case()
    assert ur.fraction(101, 103, 100, 102) == r and below < r < above
    assert [int(ur.merge(trans, f=f)["merged"][1]) for f in (below, r, above)] == [1, 1, 0]


def test_the_generated_set_holds_every_kind():
    """... by the restatement; test_generated_set asserts the same of uniq_host's own counts."""
    trans = uc.generated()
    r = ur.merge(trans, **uc.GENERATED_OPTS)
    assert 1900 <= len(trans) <= 2000 and ur.in_order(trans) and {t[0] for t in trans} == {0, 1, 2}
    assert min(r["hits"]) >= 1 and r["end_ext"] >= 1 and 0.2 <= r["merged"].mean() <= 0.8


# ---------------------------------------------------------------------------------------------------- uniq_host (uniq_dump)

def test_every_case(uniq_dump, tmp_path):
    names = sorted(CASES)
    got = dump(uniq_dump, tmp_path, [case_bytes(CASES[k][0], **CASES[k][1]) for k in names])
    for k, g in zip(names, got):
        check(g, CASES[k][0], CASES[k][1], k)


def test_fraction_at_the_ulp(uniq_dump, tmp_path):
    trans, r, above, below = uc.fraction_case()
    got = dump(uniq_dump, tmp_path, [case_bytes(trans, f=f) for f in (below, r, above)])
    assert [int(g["merged"][1]) for g in got] == [1, 1, 0]
    for g, f in zip(got, (below, r, above)):
        check(g, trans, dict(f=f))


def test_unsorted_input(uniq_dump, tmp_path):
    trans, opts = uc.unsorted_case()
    assert not ur.in_order(trans)
    (got,) = dump(uniq_dump, tmp_path, [case_bytes(trans, **opts)])
    want = check(got, trans, opts)
    assert "head" not in got and want["merged"].sum() > 0


def test_generated_set(uniq_dump, tmp_path):
    trans = uc.generated()
    (got,) = dump(uniq_dump, tmp_path, [case_bytes(trans, **uc.GENERATED_OPTS)])
    # the host alone: every kind of hit, an end raised, and a merged share between 20 % and 80 %
    assert min(got["hits"]) >= 1 and int(got["end_ext"][0]) >= 1 and 0.2 <= got["merged"].mean() <= 0.8
    assert int(got["hits"].sum()) == int(got["merged"].sum()) and len(got["u_src"]) + int(got["merged"].sum()) == len(trans)
    check(got, trans, uc.GENERATED_OPTS)


def sam_transcripts(path):
    """(names, transcripts) of a SAM file whose CIGARs hold M and N only."""
    refs, names, trans = [], [], []
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        if ln.startswith("@SQ"):
            refs.append(f[1][3:])
        if ln.startswith("@"):
            continue
        pos, chain, start = int(f[3]), [], int(f[3])
        for length, op in re.findall(r"(\d+)([MN])", f[5]):
            if op == "N":
                chain.append((start, pos - 1))
                start = pos + int(length)
            pos += int(length)
        chain.append((start, pos - 1))
        names.append(f[0])
        trans.append((refs.index(f[2]), int(f[1]) & 16 != 0, chain))
    return refs, names, trans


def gtf_transcript_rows(path):
    """(chromosome, start, end, strand, transcript_id, coverage or None) of every transcript line."""
    rows = []
    for ln in open(path):
        f = ln.rstrip("\n").split("\t")
        if len(f) > 8 and f[2] == "transcript":
            cov = re.search(r'transcript_cov "(\d+)"', f[8])
            rows.append((f[0], int(f[3]), int(f[4]), f[6], re.search(r'transcript_id "([^"]*)"', f[8]).group(1), int(cov.group(1)) if cov else None))
    return rows


@pytest.mark.parametrize("s, expected", [(0, "uniq.unique.gtf"), (1, "uniq_s.unique.gtf")])
def test_hand_derived_answers(uniq_dump, tmp_path, s, expected):
    refs, names, trans = sam_transcripts(os.path.join(HAND, "uniq.sam"))
    (got,) = dump(uniq_dump, tmp_path, [case_bytes(trans, s=s)])
    rows = [(refs[trans[r][0]], int(a), int(b), "+-"[trans[r][1]], names[r], int(c)) for r, a, b, c in zip(got["u_src"], got["u_start"], got["u_end"], got["u_cov"])]
    assert rows == gtf_transcript_rows(os.path.join(HAND, expected))


def test_argument_checks(uniq_dump, tmp_path):
    tid, rev, ex_off, xs, xe = ur.columns([(0, 0, [(1, 5), (9, 12)]), (0, 1, [(3, 4)])])
    bad = {
        "2147483648 transcripts": case_bytes(None, columns=(tid[:1], rev[:1], ex_off, xs, xe), n=1 << 31),
        "negative size": case_bytes(None, columns=(tid[:1], rev[:1], ex_off, xs, xe), n=-1),
        "does not start at 0": case_bytes(None, columns=(tid, rev, ex_off + 1, np.append(xs, 1), np.append(xe, 1))),
        "descends at transcript 1": case_bytes(None, columns=(tid, rev, np.asarray([0, 2, 1], np.int64), xs, xe)),
        "transcript 1 has no exon": case_bytes(None, columns=(tid, rev, np.asarray([0, 3, 3], np.int64), xs, xe)),
        "transcript 1: tid -2": case_bytes(None, columns=(np.asarray([0, -2], np.int32), rev, ex_off, xs, xe)),
        "transcript 0: a negative coordinate": case_bytes(None, columns=(tid, rev, ex_off, np.asarray([1, -9, 3], np.int32), xe)),
        "transcript 1: a negative coordinate": case_bytes(None, columns=(tid, rev, ex_off, xs, np.asarray([5, 12, -1], np.int32))),
    }
    names = sorted(bad)
    got = dump(uniq_dump, tmp_path, [bad[k] for k in names] + [case_bytes(None, columns=(np.asarray([-1, 0], np.int32), rev, ex_off, xs, xe))])
    for k, g in zip(names, got):
        assert int(g["rc"][0]) == -1 and k in g["error"].tobytes().decode(), (k, g["error"].tobytes())
    assert int(got[-1]["rc"][0]) == 0                                # tid -1 (a chromosome outside the header) is in the domain


# ---------------------------------------------------------------------------------------------------- beyond three tiles

WALK = uc.walk_cases()
GOLDEN = os.path.join(ROOT, "tests", "golden", "uniq")


def list_sizes(cols, u_src):
    """Entries of every cluster's list."""
    return np.bincount((np.cumsum(ur.heads_columns(cols)) - 1)[u_src])


def test_the_generator_is_unchanged():
    """loci() took one more parameter: generated() is, element for element, the set recorded before (tests/golden/uniq)."""
    want = np.load(os.path.join(GOLDEN, "generated_columns.npz"))
    for got, k in zip(ur.columns(uc.generated()), ("tid", "rev", "ex_off", "xs", "xe")):
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k


def test_heads_of_columns_is_heads():
    for trans, _o in list(CASES.values()) + [c[:2] for c in WALK.values()]:
        assert np.array_equal(ur.heads_columns(ur.columns(trans)), ur.heads(trans))
    for cols in (uc.reach_columns(3, 2 * uc.TILE + 5), uc.step_columns(63, (-1, 0), None), uc.step_columns(uc.TILE - 1, (2147483646, 2147483647), 2147483646)):
        assert np.array_equal(ur.heads_columns(cols), ur.heads(ur.as_list(cols)))


def test_restatement_on_the_walk_cases():
    """What the walk cases are built to show, written down from the rule."""
    for name, (trans, opts, (merged, uniq_of)) in WALK.items():
        assert ur.in_order(trans), name
        r = ur.merge(trans, **opts)
        k = len(merged)
        assert (list(r["merged"][-k:]), list(r["uniq_of"][-k:])) == (merged, uniq_of), name
        if name.startswith("deep_mutation"):
            j, end = uniq_of[0], trans[0][2][-1][1]
            assert (int(r["u_end"][j]), int(r["u_cov"][j]), r["end_ext"], list(r["hits"])) == (end + 750, 4, 3, [3, 0, 0]) and int(ur.heads(trans).sum()) == 1
        elif name.startswith("several"):
            c = int(name.rsplit("_", 1)[1])
            assert int(ur.heads(trans).sum()) == c and len(r["u_src"]) == 65 * c and int(r["merged"].sum()) == k * c
        else:                                                       # one cluster, and the last offer alone may merge
            assert int(ur.heads(trans).sum()) == 1 and int(r["merged"].sum()) == sum(merged)
    # the lanes of the pair in front of the fillers: the list holds n_fill + 2 entries when the offer comes, entry k is judged by lane
    # (n_fill + 1 - k) % 64 of round (n_fill + 1 - k) // 64
    assert [((f + 0) % 64, (f + 1) % 64, (f + 1) // 64) for f in uc.STOP_HIT_FILL] == [(0, 1, 0), (61, 62, 0), (62, 63, 0), (63, 0, 1), (0, 1, 1), (62, 63, 1), (63, 0, 2), (0, 1, 2)]


def test_restatement_on_the_reach_and_step_cases():
    """The closed form against the running maximum, at every size."""
    for p, r in uc.REACH_PAIRS + uc.REACH_ROUND_PAIRS:
        cols = uc.reach_columns(p, r)
        n = len(cols[0])
        head, clusters, largest = uc.reach_expected(p, r, n)
        assert n >= r + 1 + uc.TILE + 3 and np.array_equal(ur.heads_columns(cols), head) and clusters == int(head.sum()) == n - (r - p)
        assert largest == int(np.diff(np.append(np.flatnonzero(head), n)).max()) == r - p + 1
        assert int(cols[4][2 * p + 1]) == int(cols[3][2 * r]) and int(cols[3].min()) >= 1       # the long end EQUALS r's start
    for p in uc.STEP_SLOTS:
        for chroms in uc.STEP_CHROMS:
            for long_end in uc.STEP_ENDS:
                cols = uc.step_columns(p, chroms, long_end)
                assert ur.heads_columns(cols).all() and int(cols[4][2 * p + 1]) >= int(cols[3][2 * p + 2::2].max()) and int(cols[0][p]) < int(cols[0][p + 1])
    small = uc.reach_columns(0, 1)
    r = ur.merge(ur.as_list(small))
    assert not r["merged"].any() and list(r["u_src"]) == list(range(len(small[0])))


def closed_form(got, cols, head, name):
    """A case of columns in which nothing merges, as uniq_dump answers it."""
    n = len(cols[0])
    assert int(got["rc"][0]) == 0 and int(got["in_order"][0]) == 1, name
    assert np.array_equal(got["head"], head) and int(got["n_clusters"][0]) == int(head.sum()), (name, int(got["n_clusters"][0]))
    assert int(got["largest"][0]) == int(np.diff(np.append(np.flatnonzero(head), n)).max()), name


def nothing_merges(got, cols, name):
    n = len(cols[0])
    assert not got["merged"].any() and np.array_equal(got["uniq_of"], np.arange(n)) and np.array_equal(got["u_src"], np.arange(n)), name
    assert np.array_equal(got["u_start"], cols[3][0::2]) and np.array_equal(got["u_end"], cols[4][1::2]) and (got["u_cov"] == 1).all(), name
    assert not got["hits"].any() and int(got["end_ext"][0]) == 0, name


def test_walk_cases(uniq_dump, tmp_path):
    names = sorted(WALK)
    got = dump(uniq_dump, tmp_path, [case_bytes(WALK[k][0], **WALK[k][1]) for k in names])
    for k, g in zip(names, got):
        check(g, WALK[k][0], WALK[k][1], k)


def test_reach_and_step_cases_up_to_the_wave(uniq_dump, tmp_path):
    """... tid 2147483647 among them: (uint32_t)tid + 1u in uniq_key, where tid + 1 overflowed."""
    cases = [((p, r), uc.reach_columns(p, r), uc.reach_expected(p, r, r + 1 + uc.N_TAIL)[0]) for p, r in uc.REACH_PAIRS if r < uc.ROUND]
    for p in uc.STEP_SLOTS[:-1]:
        for chroms in uc.STEP_CHROMS:
            for long_end in uc.STEP_ENDS:
                cols = uc.step_columns(p, chroms, long_end)
                cases.append(((p, chroms, long_end), cols, np.ones(len(cols[0]), np.uint8)))
    assert any(int(cols[0].max()) == 2147483647 for _n, cols, _h in cases)
    got = dump(uniq_dump, tmp_path, [case_bytes(None, columns=cols) for _n, cols, _h in cases])
    for (name, cols, head), g in zip(cases, got):
        closed_form(g, cols, head, name)
        nothing_merges(g, cols, name)


def test_reach_and_step_cases_at_the_round(uniq_dump, tmp_path):
    """head, n_clusters and largest alone."""
    cases = [((p, r), uc.reach_columns(p, r), uc.reach_expected(p, r, r + 1 + uc.N_TAIL)[0]) for p, r in uc.REACH_PAIRS + uc.REACH_ROUND_PAIRS if r >= uc.ROUND]
    for chroms in uc.STEP_CHROMS:
        for long_end in uc.STEP_ENDS:
            cols = uc.step_columns(uc.STEP_SLOTS[-1], chroms, long_end)
            cases.append(((chroms, long_end), cols, np.ones(len(cols[0]), np.uint8)))
    got = dump(uniq_dump, tmp_path, [case_bytes(None, columns=cols) for _n, cols, _h in cases])
    for (name, cols, head), g in zip(cases, got):
        closed_form(g, cols, head, name)


@pytest.mark.parametrize("which", ["dense", "wide"])
def test_larger_generated_sets(uniq_dump, tmp_path, which):
    trans, cols = getattr(uc, which)()
    assert ur.in_order(trans) and {t[0] for t in trans} == {0, 1, 2} and 0.99 * getattr(uc, which.upper() + "_N") <= len(trans)
    (got,) = dump(uniq_dump, tmp_path, [case_bytes(None, columns=cols, **uc.GENERATED_OPTS)])
    # the host alone: every kind of hit, an end raised, and a merged share between 20 % and 80 %
    assert min(got["hits"]) >= 1 and int(got["end_ext"][0]) >= 1 and 0.2 <= got["merged"].mean() <= 0.8
    if which == "dense":                                            # lists of more than two lane rounds
        assert list_sizes(cols, got["u_src"]).max() >= 130
    else:                                                           # both scans beyond their first round of 16 384 words
        assert int(got["n_clusters"][0]) > 16384 and len(got["u_src"]) > 16384
    check(got, trans, uc.GENERATED_OPTS, which)


# ---------------------------------------------------------------------------------------------------- the command's own loop

def write_gtf(path, trans, refs):
    with open(path, "w") as fh:
        for i, (tid, rev, chain) in enumerate(trans):
            attr = 'gene_id "g%d"; transcript_id "t%d";' % (i, i)
            fh.write("%s\tsrc\ttranscript\t%d\t%d\t.\t%s\t.\t%s\n" % (refs[tid], chain[0][0], chain[-1][1], "+-"[rev], attr))
            for s, e in chain:
                fh.write("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (refs[tid], s, e, "+-"[rev], attr))


def write_header(path, refs):
    with open(path, "w") as fh:
        fh.write("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:100000000\n" % r for r in refs))


@pytest.mark.parametrize("intersect", [False, True])
def test_cli_without_a_context_equals_uniq_host(uniq_dump, tmp_path, intersect):
    """`unique-gtf -m g` where no device can be opened runs host/tail.c's m_merge loop: its transcript lines against uniq_host's list."""
    trans, refs = uc.generated()[:400], ["chrA", "chrB", "chrC"]
    o = uc.GENERATED_OPTS
    write_gtf(str(tmp_path / "in.gtf"), trans, refs)
    write_header(str(tmp_path / "hdr.sam"), refs)
    out = str(tmp_path / "out.gtf")
    args = ["unique-gtf", "-m", "g", "-b", str(tmp_path / "hdr.sam"), "-d", str(o["d"]), "-D", str(o["D"]), "-f", str(o["f"])] + (["-I"] if intersect else [])
    r = hostlib.run_cli(args + [str(tmp_path / "in.gtf")], stdout_path=out, env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1", "L2R_TIMING": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"merge_trans" not in r.stderr                            # (no context: the line of the engine's route is not written)
    (got,) = dump(uniq_dump, tmp_path, [case_bytes(trans, **o)])
    rows = gtf_transcript_rows(out)
    if intersect:
        want = [(refs[trans[i][0]], trans[i][2][0][0], trans[i][2][-1][1], "+-"[trans[i][1]], "t%d" % i, 1) for i in np.flatnonzero(got["merged"])]
    else:
        want = [(refs[trans[r_][0]], int(a), int(b), "+-"[trans[r_][1]], "t%d" % r_, int(c)) for r_, a, b, c in zip(got["u_src"], got["u_start"], got["u_end"], got["u_cov"])]
    assert rows == want and len(rows) > 50
