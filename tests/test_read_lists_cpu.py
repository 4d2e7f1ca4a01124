"""The read lists of `update-gtf -a / -k / -v / -u`, the parts that need no GPU: tests/read_list_restatement.py against hand-made piece
patterns and the hand-written goldens (tests/golden/read_lists), the goldens against the oracle CLI, and the host side of
l2r_gtftext_anno / _reads / _list -- the argument checks, rl_select, rl_block_bytes, the batch cut and the exact host routine rl_text_host
-- as a stand-alone program under ASan + UBSan (tests/lists_dump.hip, `make -C lr2rmats_amd/csrc lists-dump`) against the restatement.
(A block of 2^32 - 64 bytes needs some 10^8 exons: that kind alone is not provoked.)"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lr2rmats_amd import capi
from tests import read_list_cases as rc
from tests import read_list_restatement as rr
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LISTS_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "lists_dump")
HAND = os.path.join(ROOT, "tests", "golden", "hand")
GOLDEN = os.path.join(ROOT, "tests", "golden", "read_lists")
SYMBOLS = ["l2r_gtftext_anno", "l2r_gtftext_reads", "l2r_gtftext_list", "l2r_gtftext_list_out"]
LIST_FILE = {rr.ALL: "all", rr.KNOWN: "known", rr.NOVEL: "novel", rr.UNRECOG: "unrecog"}


# ---------------------------------------------------------------------------------------------------- the restatement

def test_piece_patterns_by_hand():
    for flags, want in rc.PATTERNS:
        assert rr.pieces(flags) == want, flags
    assert len(rc.PATTERNS[-1][1]) == 13


def test_lists_by_hand():
    """Six reads, one per class, through the four lists and the four settings of has_sj and split."""
    case = rc.flag_case(1, [[rc.NJ, 0, 0]] * 6, info=(rc.KNOWN, rc.UNRECOG, rc.NOVEL_PASS, rc.NOVEL_FAIL, rc.NOVEL_UNCHECKED, 0x03))
    reads = lambda lst: [(b[0], b[3]) for b in rr.select(case, lst)]
    assert reads(rr.ALL) == [(i, -1) for i in range(6)] and reads(rr.KNOWN) == [(0, -1)] and reads(rr.UNRECOG) == [(1, -1)]
    assert reads(rr.NOVEL) == [(2, -1), (3, 0), (4, 0)]                  # has_sj and split: the reads without SJ_PASS come as pieces
    case["split"] = False
    assert reads(rr.NOVEL) == [(2, -1)]
    case["has_sj"] = False
    assert reads(rr.NOVEL) == [(2, -1), (3, -1), (4, -1)]                # no junction table: whole, whatever SJ_PASS says
    case["split"] = True
    assert reads(rr.NOVEL) == [(2, -1), (3, -1), (4, -1)]


def test_a_piece_by_hand():
    """Q2 on a reverse read of reference 2: the transcript line on reference 0, 0 .. 0, `+`; the exon lines ascending with `-`."""
    case = rc.flag_case(2, [[rc.NJ, 0, 0]], rev=True, n_tx=1, no_ref=0.0)
    case["tid"][:] = 2
    case["xs"], case["xe"] = np.asarray([10, 300, 5000], np.int32), np.asarray([20, 400, 6000], np.int32)
    rc.set_names(case, [b"readQ"])
    case["anno"], case["tx_gid"], case["tx_gname"], case["ref_tx"] = b"G1\0N1\0", np.asarray([0], np.uint32), np.asarray([3], np.uint32), np.asarray([0], np.int32)
    a = b'gene_id "G1"; transcript_id "readQ.split.0"; gene_name "N1"; transcript_name "readQ.split.0";'
    r = b"chrUn_KI270302v1_random\tlr2rmats\texon\t"
    assert rr.text(case, rr.NOVEL) == (b"c\tlr2rmats\ttranscript\t0\t0\t.\t+\t.\t" + a + b' transcript_cov "1";\n' + r + b"10\t20\t.\t-\t.\t" + a + b"\n" +
                                       r + b"300\t400\t.\t-\t.\t" + a + b"\n" + r + b"5000\t6000\t.\t-\t.\t" + a + b"\n")
    w = a.replace(b".split.0", b"")
    assert rr.text(case, rr.ALL) == (b"chrUn_KI270302v1_random\tlr2rmats\ttranscript\t10\t6000\t.\t-\t.\t" + w + b' transcript_cov "1";\n' + r + b"5000\t6000\t.\t-\t.\t" + w + b"\n" +
                                     r + b"300\t400\t.\t-\t.\t" + w + b"\n" + r + b"10\t20\t.\t-\t.\t" + w + b"\n")
    case["ref_tx"][:] = -1
    assert b'gene_id "NA"; transcript_id "readQ"; gene_name "NA"; transcript_name "readQ";' in rr.text(case, rr.ALL)


def test_symbols_in_header_library_and_binding():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(capi.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s
        assert s in capi.EXPORTS, s
    for m in ("gtftext_anno", "gtftext_reads", "gtftext_list", "gtftext_list_out"):
        assert hasattr(capi.Engine, m), m
    for k, name in enumerate(("ALL", "KNOWN", "NOVEL", "UNRECOG")):
        assert capi.header_define("L2R_GTX_LIST_" + name) == k == getattr(capi, "GTX_LIST_" + name) == getattr(rr, name)
    assert capi.header_define("L2R_GTX_PIECE_NAME_MAX") == rr.PIECE_NAME_MAX
    assert capi.GTX_STAT_NAMES[12:] == ["k_rl_select", "piece_blocks"]


# ---------------------------------------------------------------------------------------------------- the host side (lists_dump)

@pytest.fixture(scope="module")
def lists_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "lists-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return LISTS_DUMP


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


def check_sound(got, case, lists=rr.LISTS):
    """Selection, text, lines and the bytes of every block of a dump against the restatement."""
    assert int(got["rc"][0]) == 0
    for lst in lists:
        sel, want = rr.select(case, lst), rr.texts(case, lst)
        tag = "_%d" % lst
        assert list(zip(*[got[k + tag].tolist() for k in ("read", "first", "count", "piece")])) == sel, lst
        assert int(got["pieces" + tag][0]) == sum(1 for b in sel if b[3] >= 0)
        assert int(got["text_rc" + tag][0]) == 0 and not got["kind" + tag].any()
        assert got["text" + tag].tobytes() == b"".join(want), lst
        assert got["bytes" + tag].tolist() == [len(t) for t in want]                             # rl_block_bytes == len(text), block by block
        assert got["lines" + tag].tolist() == [t.count(b"\n") for t in want]
        assert int(got["n_lines" + tag][0]) == sum(t.count(b"\n") for t in want)
        assert got["text_cut" + tag].tobytes() == b"".join(want)


def test_classes_alone_and_mixed(lists_dump, tmp_path):
    cases = rc.class_cases()
    seen = set()
    for got, case in zip(dump(lists_dump, tmp_path, [rc.case_file(c) for c in cases]), cases):
        check_sound(got, case)
        seen |= {(lst, b[3] >= 0) for lst in rr.LISTS for b in rr.select(case, lst)}
    assert seen == {(rr.ALL, False), (rr.KNOWN, False), (rr.UNRECOG, False), (rr.NOVEL, False), (rr.NOVEL, True)}


def test_piece_patterns_strands_and_names(lists_dump, tmp_path):
    cases = rc.piece_cases() + rc.name_cases()
    for got, case in zip(dump(lists_dump, tmp_path, [rc.case_file(c) for c in cases]), cases):
        check_sound(got, case)
    first = rc.piece_cases()[0]
    assert [(b[0], b[1], b[1] + b[2] - 1) for b in rr.select(first, rr.NOVEL)] == [(i, a, b) for i, (_, p) in enumerate(rc.PATTERNS) for a, b in p]
    assert b".split.12" in rr.text(first, rr.NOVEL)
    rev = rr.texts(rc.piece_cases()[1], rr.NOVEL)[0].split(b"\n")
    assert b"\t+\t" in rev[0] and all(b"\t-\t" in ln for ln in rev[1:-1])                         # `-` on the exon lines only
    starts = [int(ln.split(b"\t")[3]) for ln in rev[1:-1]]
    assert starts == sorted(starts) and len(starts) == 5                                          # ... which ascend
    long_names = rr.texts(rc.name_cases()[-2], rr.NOVEL)
    assert max(len(re.search(rb'transcript_name "([^"]*)"', t).group(1)) for t in long_names) == 99


def test_every_domain_error_in_its_order(lists_dump, tmp_path):
    cases = rc.error_cases()
    kinds = set()
    for got, (case, lst, block, kind) in zip(dump(lists_dump, tmp_path, [rc.case_file(c[0]) for c in cases]), cases):
        assert rr.error(case, lst) == (block, kind)
        tag = "_%d" % lst
        assert int(got["rc"][0]) == 0 and int(got["text_rc" + tag][0]) == -1
        bad = np.flatnonzero(got["kind" + tag])
        assert int(bad[0]) == block and int(got["kind" + tag][block]) == rr.KIND_CODE[kind], (kind, got["kind" + tag].tolist())
        msg = got["error" + tag].tobytes().decode()
        assert "block %d:" % block in msg and rr.KIND_TEXT[kind] in msg, msg
        assert int(got["bytes" + tag][block]) == 0 and int(got["lines" + tag][block]) == 0
        check_sound(got, case, rc.sound_lists(case, lst, block))
        kinds.add(kind)
    assert kinds == set(rr.KINDS) - {"big"}


def test_argument_errors(lists_dump, tmp_path):
    good = rc.make_case(80, [2, 3, 1])
    bad = []
    c = dict(good); c["ex_off"] = good["ex_off"].copy(); c["ex_off"][1] += 1; bad.append((c, "ex_off gives"))       # ex_off against the exon counts of info
    c = dict(good); c["ex_off"] = good["ex_off"] + 1; bad.append((c, "does not start at 0"))
    for got, (case, what) in zip(dump(lists_dump, tmp_path, [rc.case_file(c) for c, _ in bad]), bad):
        assert int(got["rc"][0]) == -2 and what in got["error"].tobytes().decode()


def test_the_batch_cut(lists_dump, tmp_path):
    case = rc.make_case(81, [1, 2, 3, 5, 8, 2, 1, 40, 2, 3] * 3, flags="pieces")
    lens = {lst: [len(t) for t in rr.texts(case, lst)] for lst in rr.LISTS}
    cuts = [(0, 1, 1 << 30), (0, 3, 1 << 30), (2, 1 << 20, 1), (0, 1 << 20, sum(lens[rr.ALL][:3])), (0, 1 << 20, sum(lens[rr.ALL][:3]) - 1), (1, 7, 2000)]
    for got, (first, mb, mby) in zip(dump(lists_dump, tmp_path, [rc.case_file(case, f, b, y) for f, b, y in cuts]), cuts):
        for lst in rr.LISTS:
            want, at = [], first
            while at < len(lens[lst]):
                k = rr.cut(lens[lst], at, mb, mby)
                want.append(k)
                at += k
            assert got["cut_%d" % lst].tolist() == want, (lst, first, mb, mby)
            assert got["text_cut_%d" % lst].tobytes() == b"".join(rr.texts(case, lst)[first:])


# ---------------------------------------------------------------------------------------------------- the goldens of the hand cases

# per hand case: the command's options, the reads that passed the junction check (SJ_PASS; the others of the novel class are split
# candidates), the rows of the junction table, -s
HAND_CASES = {"upd": (["-l", "5"], "upd.sam", (), False, False),
              "split": (["-s", "-l", "5", "-J", "1", "-j", os.path.join(HAND, "split_sj.tab")], "split.sam", ("a1", "w1", "w2"), True, True)}


def hand_case(name):
    """The case of a hand input from its hand-derived detail table (tests/golden/hand/<name>.detail.txt): -l 5, so every read is FULL."""
    _, sam, passed, has_sj, split = HAND_CASES[name]
    refs = [ln.split("\t")[1][3:].encode() for ln in open(os.path.join(HAND, sam)) if ln.startswith("@SQ")]
    rows = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(HAND, name + ".detail.txt"))][1:]
    genes = sorted({(r[4], r[5]) for r in rows if r[4] != "NA"})
    anno, ids = rr.pack_table([g[0].encode() for g in genes] + [g[1].encode() for g in genes])
    names, qname = rr.pack_table([r[0].encode() for r in rows])
    info, xs, xe, f = [], [], [], []
    for r in rows:
        n = int(r[6])
        word = 0x04 | (0x01 if r[3] == "0" else 0x02 if r[3] == "1" else 0) | (0x08 if r[2] == "-" else 0) | (0x40 if r[0] in passed else 0)
        info.append(word | n << 8)
        xs += [int(v) for v in r[7].split(",")]
        xe += [int(v) for v in r[8].split(",")]
        flags = [0] * n
        for col, bit in ((14, rc.NJ), (16, rc.UJ)):
            for j in ([] if r[col] == "NA" else r[col].split(",")):
                flags[int(j)] |= bit
        f += flags
    return {"refs": refs, "src": b"lr2rmats", "tid": np.asarray([refs.index(r[1].encode()) for r in rows], np.int32), "names": names, "qname": np.asarray(qname, np.uint32),
            "tid_name": None, "anno": anno, "tx_gid": np.asarray(ids[:len(genes)], np.uint32), "tx_gname": np.asarray(ids[len(genes):], np.uint32),
            "ex_off": np.cumsum([0] + [int(r[6]) for r in rows]).astype(np.int64), "xs": np.asarray(xs, np.int32), "xe": np.asarray(xe, np.int32), "f": np.asarray(f, np.uint8),
            "info": np.asarray(info, np.uint32), "ref_tx": np.asarray([-1 if r[4] == "NA" else genes.index((r[4], r[5])) for r in rows], np.int32),
            "has_sj": has_sj, "split": split}


def golden(name, lst):
    with open(os.path.join(GOLDEN, "%s.%s.gtf" % (name, LIST_FILE[lst])), "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_goldens_equal_the_restatement_and_the_host_routine(lists_dump, tmp_path, name):
    case = hand_case(name)
    got = dump(lists_dump, tmp_path, [rc.case_file(case)])[0]
    check_sound(got, case)
    for lst in rr.LISTS:
        assert rr.text(case, lst) == golden(name, lst), (name, lst)
    if name == "split":
        novel = golden(name, rr.NOVEL)
        assert novel.count(b".split.0") == 2 * (6 + 3) and b"chrA\tlr2rmats\ttranscript\t0\t0\t.\t+\t.\tgene_id \"GC\"; transcript_id \"p2.split.0\"" in novel
        assert golden(name, rr.KNOWN) == b"" and golden(name, rr.UNRECOG) == b""
    else:
        assert golden(name, rr.NOVEL).count(b"\ttranscript\t") == 9 and golden(name, rr.ALL).count(b"\ttranscript\t") == 13
        assert golden(name, rr.ALL).index(b"exon\t12500\t12600") < golden(name, rr.ALL).index(b"exon\t11000\t11100")      # r1 is on `-`: descending


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_goldens_equal_the_oracle_cli(oracle, tmp_path, name):
    extra, sam = HAND_CASES[name][:2]
    o = {lst: str(tmp_path / (LIST_FILE[lst] + ".gtf")) for lst in rr.LISTS}
    argv = ["update-gtf"] + extra + ["-a", o[rr.ALL], "-k", o[rr.KNOWN], "-v", o[rr.NOVEL], "-u", o[rr.UNRECOG], "-o", str(tmp_path / "out.gtf"),
                                     os.path.join(HAND, sam), os.path.join(HAND, "anno.gtf")]
    assert oracle.run_cli(argv) == 0
    for lst in rr.LISTS:
        assert open(o[lst], "rb").read() == golden(name, lst), (name, lst)


# ---------------------------------------------------------------------------------------------------- the writer the command falls back on

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from lr2rmats_amd import hostlib
from oracle import pyoracle as po
outs, cuts, argv = sys.argv[1:5], [int(v) for v in sys.argv[5].split(",")], sys.argv[6:]
job = hostlib.Job(argv, open_outputs=False)
a, r, sj, p = job.annotation_arrays(), job.read_arrays(), job.junction_arrays(), job.prm
op = po.default_params(min_exon=p.min_exon, min_intron=p.min_intron, max_delet=p.max_delet, ss_dis=p.ss_dis, end_dis=p.end_dis,
                       full_level=p.full_level, split_trans=p.split_trans, use_multi=p.use_multi, min_sj_cnt=p.min_sj_cnt,
                       force_strand=p.force_strand, single_exon_ovlp_frac=p.single_exon_ovlp_frac)
res = po.classify_soa(r["tid"], r["pos"], r["rev"], r["cig_off"], r["cig"], a["tx_tid"], a["tx_start"], a["tx_end"], a["tx_rev"],
                      a["tx_ex_off"], a["ex_start"], a["ex_end"], sj=sj, params=op)
info = (res.info & 0x7f) | (np.diff(res.ex_off).astype(np.uint32) << 8)
n = int(info.shape[0])
bounds = [0] + [c for c in cuts if 0 < c < n] + [n]
for lst, path in enumerate(outs):
    for lo, hi in zip(bounds[:-1], bounds[1:]):                  # shard by shard, as the command comes here
        if job.list_rows(lst, lo, hi, path, res.ex_off, res.ex_start, res.ex_end, res.ex_flag, info, res.ref_tx):
            sys.exit(3)
sys.exit(0)
"""


@pytest.fixture(scope="module")
def synth_files(oracle, tmp_path_factory):
    from lr2rmats_amd import synth
    from tests import util
    d = tmp_path_factory.mktemp("lists")
    anno = synth.make_annotation(6000, 31, nchr=6, shuffle_within_gene=True)
    reads = synth.make_reads(anno, 3000, 5, 31, xs_conflict_frac=0.03)
    sam, gtf, tab = str(d / "r.sam"), str(d / "a.gtf"), str(d / "sj.tab")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    af = anno.in_file_order()
    base = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=3))
    util.junction_table(af, reads, base, 31, cover=0.6)[0].write(tab)
    return sam, gtf, tab


@pytest.mark.parametrize("with_sj", [False, True])
def test_fall_back_writer_equals_the_oracle_cli(oracle, tmp_path, synth_files, with_sj):
    import sys
    sam, gtf, tab = synth_files
    extra = ["-s", "-l", "3", "-J", "1", "-j", tab] if with_sj else ["-l", "3"]
    oo = [str(tmp_path / ("o.%s.gtf" % LIST_FILE[lst])) for lst in rr.LISTS]
    ho = [str(tmp_path / ("h.%s.gtf" % LIST_FILE[lst])) for lst in rr.LISTS]
    assert oracle.run_cli(["update-gtf"] + extra + ["-a", oo[0], "-k", oo[1], "-v", oo[2], "-u", oo[3], "-o", str(tmp_path / "o.gtf"), sam, gtf]) == 0
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT] + ho + ["1,700,701,2222", "update-gtf"] + extra + ["-o", str(tmp_path / "h.gtf"), sam, gtf], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    for a, b in zip(oo, ho):
        assert open(a, "rb").read() == open(b, "rb").read(), b
    assert all(os.path.getsize(f) > 1000 for f in oo)
    if with_sj:
        assert b".split." in open(oo[2], "rb").read()
