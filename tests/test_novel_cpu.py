"""The novel list of `update-gtf`, the parts that need no GPU: the host side of l2r_novel_* -- the predicates, the argument checks, the
selection, the route test, the exact host routine novel_host and the BED text with its batch cut -- as a stand-alone program under
ASan + UBSan (tests/novel_dump.hip, `make -C lr2rmats_amd/csrc novel-dump`) against tests/novel_restatement.py."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import novel_cases as nc
from tests import novel_restatement as nr
from tests import uniq_restatement as ur
from tests.test_upload_plan_cpu import MARKS, SAN_ENV, _read_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lr2rmats_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NOVEL_DUMP = os.path.join(ROOT, "lr2rmats_amd", "lib", "novel_dump")


@pytest.fixture(scope="module")
def novel_dump():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", CSRC, "novel-dump", "HIPCC=" + HIPCC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return NOVEL_DUMP


def case_bytes(reads, tx_gene=(), na_gene=0, has_sj=0, split=0, s=0, d=0, D=ur.INT_MAX, f=0.8, refs=nc.REFS, have=(0, 0), sizes=None):
    tid, info, ref, xs, xe, fl = nr.columns(reads)
    bits = int(np.asarray(f, np.float32).view(np.uint32))
    n, nx = sizes if sizes is not None else (len(tid), len(xs))
    names = b"".join(refs)
    off = np.zeros(len(refs) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in refs])
    head = struct.pack("<14q", n, nx, len(refs), len(tx_gene), na_gene, has_sj, split, s, d, D, bits, len(names), have[0], have[1])
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in (tid, info, ref, xs, xe, fl, np.asarray(tx_gene, np.uint32), off)) + names


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


def same(g, want, name):
    """A dump of novel_dump against the restatement's result."""
    for k in ("src", "start", "end", "cov"):
        assert list(g["e_" + k]) == want["entries"][k], (name, k)
    for l in range(6):
        got = [list(r) for r in zip(*(g["%s%d" % (k, l)].tolist() for k in ("tid", "a", "b", "score", "meta")))]
        assert got == want["rows"][l], (name, l, got[:5], want["rows"][l][:5])
    assert list(g["items"]) == want["items"] and list(g["counts"]) == want["counts"], (name, list(g["counts"]), want["counts"])
    assert int(g["hits"][0]) == want["hits"] and int(g["widened"][0]) == want["widened"], name
    assert g["bed"].tobytes() == want["bed"] == g["bed_cut"].tobytes(), (name, g["bed"].tobytes()[:200], want["bed"][:200])


# ---------------------------------------------------------------------------------------------------- the restatement by hand

def test_the_bits_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "lr2rmats_hip.h")).read()
    for name, value in (("KNOWN", nr.KNOWN), ("KNOWN_SITE", nr.KNOWN_SITE), ("FULL", nr.FULL), ("REV", nr.REV), ("SJ_PASS", nr.SJ_PASS)):
        assert int(re.search(r"^#define\s+L2R_INFO_%s\s+(0x[0-9a-f]+)u" % name, text, re.M).group(1), 16) == value
    for name, value in (("NOVEL_EXON", nr.NE), ("NOVEL_DON", nr.ND), ("NOVEL_ACC", nr.NA), ("NOVEL_JUNC", nr.NJ)):
        assert int(re.search(r"^#define\s+L2R_EXF_%s\s+(0x[0-9a-f]+)u" % name, text, re.M).group(1), 16) == value


def novel(name, table=None):
    reads, opts = (table or nc.cases())[name]
    return nr.novel(reads, ref_names=nc.REFS, **opts)


def test_restatement_on_the_cases_derived_by_hand():
    """What the cases are built to show, written down from the rule (not from a program's output)."""
    assert novel("empty")["counts"] == [0] * 8 and novel("empty")["bed"] == b""
    one = novel("one")
    assert one["counts"] == [1, 1, 0, 2, 2, 1, 0, 0] and one["bed"] == b"chr2\t99\t150\tT_exon\t1\t-\nchr2\t199\t250\tT_exon\t1\t-\n"
    assert novel("no_offer")["counts"] == [0, 0, 0, 0, 0, 0, 0, 1] and novel("no_offer")["bed"] == b""
    assert novel("known_not_full")["counts"] == [0, 0, 0, 0, 0, 0, 0, 1]
    # FULL && !KNOWN && KNOWN_SITE: two of sixteen without a table, the one with SJ_PASS with one; KNOWN: eight
    assert (novel("bits_no_sj")["offers"], novel("bits_sj")["offers"], novel("bits_no_sj")["known"]) == (2, 1, 8)
    w = novel("widened_end")
    assert w["entries"] == {"src": [0], "start": [100], "end": [450], "cov": [2]} and w["bed"] == b"chr1\t299\t450\tT_exon\t2\t+\n" and w["widened"] == 1
    w = novel("widened_start", nc.unordered_cases())
    assert w["entries"] == {"src": [0], "start": [90], "end": [400], "cov": [2]} and w["bed"] == b"chr1\t89\t200\tT_exon\t2\t+\n"
    c = novel("contained")
    assert c["entries"] == {"src": [0], "start": [100], "end": [600], "cov": [1]} and c["hits"] == 1 and c["widened"] == 0
    s = novel("single_exon_hit")
    assert s["entries"]["cov"] == [2, 1] and s["entries"]["end"] == [210, 5100] and s["bed"] == b"chr1\t99\t210\tS_exon\t2\t+\n"
    assert novel("opposite_strands")["counts"][1] == 2 and novel("same_strands_merge")["counts"][1] == 1
    assert novel("opposite_strands")["rows"][nr.EXON] == [[0, 100, 200, 2, 0]]                 # one key: the first strand, both coverages
    assert novel("inner_then_terminal")["bed"] == b"chr1\t299\t400\tI_exon\t3\t+\n"
    assert novel("two_tids_one_exon")["bed"] == b"chr1\t99\t200\tT_exon\t1\t+\nchr2\t99\t200\tT_exon\t1\t+\n"
    d = novel("donor_is_acceptor")
    assert d["rows"][nr.DON] == [[0, 200, 0, 0, 0]] and d["rows"][nr.ACC] == [[0, 200, 0, 0, 0]] and d["counts"][4] == 2
    f = novel("last_exon_flags")
    # (both entries are of gene 0, the newest gene when chr1 ends: one gene)
    assert f["counts"] == [1, 2, 0, 1, 0, 0, 0, 0] and f["bed"] == b"chr1\t299\t400\tT_exon\t1\t+\n"
    assert novel("start_zero")["bed"] == b"chr1\t-1\t50\tS_exon\t1\t+\nchr1\t-1\t9\tT_exon\t1\t-\nchr1\t19\t30\tT_exon\t1\t-\n"
    g = novel("genes")
    # (transcripts 0, 2, 3 are of genes 0, 1, 2)  chr1: genes 0, 1, NA; chr2: 0 again, 2; chrX: 2 is the newest row and is not counted again, 0 is
    assert [r[:2] for r in g["rows"][nr.GENE]] == [[0, 0], [0, 1], [0, 4], [1, 0], [1, 2], [2, 0]] and g["counts"][0] == 6
    assert [r[:2] for r in g["rows"][nr.KNOWN_GENE]] == [[0, 0], [0, 1], [1, 0], [1, 2], [2, 0]] and g["counts"][7] == 5
    assert novel("gene_called_na")["counts"][0] == 1 and novel("gene_called_na")["counts"][7] == 1
    assert novel("third_word")["counts"][5] == 3 and novel("third_word")["items"][nr.JUNC] == 4
    assert novel("all_equal")["counts"][7] == 1 and novel("all_distinct")["counts"][7] == 300         # (two chromosomes, the gene the newest at the first one's end)
    for n in (4095, 4096, 4097):
        assert novel("items_%d" % n)["items"][nr.KNOWN_GENE] == n
    m = novel("mixed_twice")
    assert m["hits"] > 0 and m["widened"] == 0 and all(len(r) > 0 for r in m["rows"])


def test_the_cases_are_in_order_and_the_others_are_not():
    for name, (reads, opts) in nc.cases().items():
        assert nr.in_order(reads, opts.get("has_sj", 0)), name
    for name, (reads, opts) in nc.unordered_cases().items():
        assert not nr.in_order(reads), name


def test_sorting_by_key_is_the_backward_scans_but_for_the_gene_at_a_chromosome_s_end():
    """The argument of the device route on the restatement alone: with tid not descending the kept rows are the first items of every
    key -- and for the gene lists that minus the items whose gene is the newest kept row's of a smaller tid."""
    for name in ("mixed_257", "mixed_twice", "genes", "third_word"):
        reads, opts = nc.cases()[name]
        want = nr.novel(reads, **opts)
        for l in range(4):
            seen, first = set(), []
            for r in want["rows"][l]:
                assert tuple(r[:3]) not in seen
                seen.add(tuple(r[:3]))
                first.append(r[:3])
            assert len(first) == len(want["rows"][l])
    g = nr.novel(*[nc.cases()["genes"][0]], **nc.cases()["genes"][1])
    assert [2, 2] not in [r[:2] for r in g["rows"][nr.GENE]]                    # (tid 2, gene 2): a first item of its key, yet not kept


# ---------------------------------------------------------------------------------------------------- novel_host (novel_dump)

def test_every_case(novel_dump, tmp_path):
    cases = dict(nc.cases())
    cases.update(nc.unordered_cases())
    for k in (1, 2, 63, 64, 65, 200):
        cases["chain_%d" % k] = (nc.long_chains(k), dict(nc.BASE))
    names = sorted(cases)
    got = dump(novel_dump, tmp_path, [case_bytes(cases[k][0], **cases[k][1]) for k in names])
    for k, g in zip(names, got):
        reads, opts = cases[k]
        assert int(g["rc"][0]) == 0, (k, g.get("error", np.zeros(0, np.uint8)).tobytes())
        assert list(g["bits"]) == nr.bits_of(reads, opts.get("has_sj", 0), opts.get("split", 0)), k
        assert int(g["in_order"][0]) == int(nr.in_order(reads, opts.get("has_sj", 0))), k
        same(g, nr.novel(reads, ref_names=nc.REFS, **opts), k)


def test_chains_widen_at_every_length():
    for k in (1, 2, 63, 64, 65, 200):
        w = nr.novel(nc.long_chains(k), ref_names=nc.REFS, **nc.BASE)
        assert w["entries"]["cov"] == [2, 1, 1] and w["widened"] == 1 and w["entries"]["end"][0] == 1000 + 100 * (k - 1) + 57, k
        assert ("\t%d\t" % (1000 + 100 * (k - 1) + 57)).encode() in w["bed"], k


def test_split_route_reads_are_counted_and_refused(novel_dump, tmp_path):
    reads = nc.bit_combinations()
    (g,) = dump(novel_dump, tmp_path, [case_bytes(reads, has_sj=1, split=1, **nc.BASE)])
    assert int(g["rc"][0]) == -3 and int(g["split"][0]) == 1 == nr.novel(reads, has_sj=1, split=1, **nc.BASE)["split"]
    assert list(g["bits"]) == nr.bits_of(reads, 1, 1) and sum(1 for b in g["bits"] if b & 4) == 1
    (g,) = dump(novel_dump, tmp_path, [case_bytes(reads, has_sj=0, split=1, **nc.BASE)])         # -s without a table splits nothing
    assert int(g["rc"][0]) == 0 and int(g["split"][0]) == 0


def test_the_checks_at_their_edges(novel_dump, tmp_path):
    edges = nc.edge_cases()
    names = sorted(edges)
    got = dump(novel_dump, tmp_path, [case_bytes(edges[k][0], **edges[k][1]) for k in names])
    for k, g in zip(names, got):
        reads, opts, refusal = edges[k]
        bad = nr.bad_read(reads, len(nc.REFS), len(opts["tx_gene"]))
        if refusal is None:
            assert bad is None and int(g["rc"][0]) == 0, k
            same(g, nr.novel([r for r in reads], ref_names=nc.REFS, **opts), k)
        else:
            assert refusal == "read %d: %s" % bad, k
            assert int(g["rc"][0]) == -1 and refusal in g["error"].tobytes().decode(), (k, g["error"].tobytes())


def test_the_totals_and_the_begin(novel_dump, tmp_path):
    one = nc.widened_end()
    bad = {
        "2147483648 reads in all": case_bytes(one, have=((1 << 31) - 2, 0), **nc.BASE),
        "4294967232 exons in all": case_bytes(one, have=(0, (1 << 32) - 64 - 4), **nc.BASE),
        "negative size": case_bytes([], sizes=(-1, 0), **nc.BASE),
        "0 references": case_bytes(one, refs=[], **nc.BASE),
    }
    names = sorted(bad)
    got = dump(novel_dump, tmp_path, [bad[k] for k in names] + [case_bytes(one, have=((1 << 31) - 3, (1 << 32) - 64 - 5), **nc.BASE)])
    for k, g in zip(names, got):
        assert int(g["rc"][0]) == -1 and k in g["error"].tobytes().decode(), (k, g["error"].tobytes())
    assert int(got[-1]["rc"][0]) == 0                                # one below both bounds


def test_a_reference_name_of_254_bytes(novel_dump, tmp_path):
    refs = [b"c" * 254, b"chr2", b"chrX"]
    reads, opts = nc.cases()["mixed_65"]
    (g,) = dump(novel_dump, tmp_path, [case_bytes(reads, refs=refs, **opts)])
    want = nr.novel(reads, ref_names=refs, **opts)
    assert g["bed"].tobytes() == want["bed"] == g["bed_cut"].tobytes() and want["bed"].startswith(b"c" * 254 + b"\t")
