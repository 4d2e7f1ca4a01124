"""The novel list of `update-gtf` through the command: the engine's sink (l2r_novel_*: the updated GTF, the -E file and the seven counts of
summary.txt) on several shards with one tail thread and with four, with L2R_NOVEL_ROUTE=host and =off, against the oracle CLI: the same
bytes in every file; the stderr line names the route and its numbers are summary.txt's; -s with -j keeps the host tail, -s without -j
takes the device."""
import filecmp
import os
import re

import pytest

from lr2rmats_amd import hostlib, synth
from tests import util
from tests.test_gpu_summary import HAND, OUTS, TOY, args

pytestmark = pytest.mark.gpu

LINE = re.compile(r"\[update_gtf\] novel list: route (device|host|off), (\d+) reads in (\d+) adds, (\d+) offers, (\d+) entries \((\d+) hits\), (\d+) exons, (\d+) sites, (\d+) junctions, "
                  r"(\d+) genes, (\d+) known genes, (\d+) bytes, (\d+) batches, (\d+) clusters, largest (\d+)$")
# the line's groups against summary.txt
KEYS = {5: "Added_Novel_Transcripts", 7: "Added_Novel_Exons", 8: "Added_Novel_Sites", 9: "Added_Novel_Splice_Junctions", 10: "Updated_Genes", 11: "Genes_of_Known_Transcripts_from_BAM"}
SEED = 61           # (the set of tests/test_gpu_summary.py)


def every_way(oracle, tmp_path, extra, aln, gtf, n_reads, split_with_table=False):
    """The command five ways: the same bytes in every file; the line names the route, and on the engine's routes its numbers are
    summary.txt's."""
    shards = max(1, (n_reads or 6) // 3 - 1)
    parts = max(1, (n_reads or 6) // 5)
    configs = {"off": dict(L2R_NOVEL_ROUTE="off", L2R_THREADS=1), "t1": dict(L2R_NOVEL_ROUTE="device", L2R_THREADS=1, L2R_CHUNK_READS=shards, L2R_NOVEL_BATCH=3),
               "t4": dict(L2R_NOVEL_ROUTE="device", L2R_THREADS=4, L2R_TAIL_PART_READS=parts, L2R_CHUNK_READS=shards, L2R_NOVEL_TEXT_MAX=200),
               "host": dict(L2R_NOVEL_ROUTE="host", L2R_THREADS=4, L2R_TAIL_PART_READS=parts)}
    route = {"off": "off", "t1": "device", "t4": "device", "host": "host"}
    d = tmp_path / "oracle"
    d.mkdir()
    want = {k: str(d / k) for k in OUTS}
    assert oracle.run_cli(args(want, extra, aln, gtf)) == 0
    text = open(want["summary"]).read()
    for tag, env in configs.items():
        d = tmp_path / tag
        d.mkdir()
        o = {k: str(d / k) for k in OUTS}
        r = hostlib.run_cli(args(o, extra, aln, gtf), env=dict(env, L2R_TIMING=1))
        assert r.returncode == 0, (tag, r.stderr.decode()[-1500:])
        lines = [ln for ln in r.stderr.decode().splitlines() if "novel list: route" in ln]
        assert len(lines) == 1 and LINE.match(lines[0]), (tag, lines, r.stderr.decode()[-800:])
        m = LINE.match(lines[0])
        assert m.group(1) == ("off" if split_with_table else route[tag]), (tag, lines[0])
        if m.group(1) != "off":
            assert n_reads is None or int(m.group(2)) == n_reads, (tag, lines[0])
            for g, key in KEYS.items():
                assert int(m.group(g)) == int(re.search(r"^%s\t(\d+)$" % key, text, re.M).group(1)), (tag, key, lines[0])
            assert int(m.group(12)) == os.path.getsize(want["gtf"]) + os.path.getsize(want["bed"]), (tag, lines[0])
            if "L2R_CHUNK_READS" in env and n_reads is not None and n_reads >= 9:
                assert int(m.group(3)) >= 3, (tag, lines[0])
        for k in OUTS:
            assert filecmp.cmp(o[k], want[k], shallow=False), (tag, k)
    return want


@pytest.mark.parametrize("name", ["upd", "upd_c", "dis2", "sj", "mg", "split"])
def test_cli_hand_cases(oracle, tmp_path, name):
    """... upd_c with -c and dis2 with -d 2 (the merge parameters that reach l2r_novel_begin), sj with a junction table and no -s, mg with
    -m g input, split with -s and a table: the host tail."""
    from tests.test_hand_known_answers import CASES as HAND_CASES
    cmd, inp, anno, _ = HAND_CASES[name]
    path = os.path.join(HAND, inp)
    n = sum(1 for ln in open(path) if not ln.startswith("@")) if inp.endswith(".sam") else None          # (-m g: the reads are a GTF's transcripts)
    every_way(oracle, tmp_path, list(cmd)[1:], path, os.path.join(HAND, anno if isinstance(anno, str) else "anno.gtf"), n, split_with_table=name == "split")


def test_cli_toy(oracle, tmp_path):
    n = sum(1 for ln in open(os.path.join(TOY, "toy.sam")) if not ln.startswith("@"))
    every_way(oracle, tmp_path, ["-l", "3"], os.path.join(TOY, "toy.sam"), os.path.join(TOY, "original.gtf"), n)


@pytest.fixture(scope="module")
def run_set(oracle):
    anno = synth.make_annotation(3000, SEED, nchr=3)
    af, reads = anno.in_file_order(), synth.make_reads(anno, 700, 6, SEED)
    base = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=3))
    j, _sj = util.junction_table(af, reads, base, SEED, cover=0.6)
    return anno, reads, j


@pytest.mark.parametrize("how", ["plain", "merge", "s_without_j", "s_with_j"])
def test_cli_synthetic_set(oracle, tmp_path, run_set, how):
    """... the generated set: as it is, with -c -d -D -f away from their defaults, with -s and no table (the device), with -s and a table
    (route off, equal to the oracle)."""
    anno, reads, j = run_set
    sam, gtf, tab = str(tmp_path / "r.sam"), str(tmp_path / "a.gtf"), str(tmp_path / "sj.tab")
    reads.write_sam(sam)
    anno.write_gtf(gtf)
    j.write(tab)
    extra = {"plain": ["-l", "3"], "merge": ["-l", "3", "-c", "-d", "2", "-D", "50", "-f", "0.5"], "s_without_j": ["-s", "-l", "3"], "s_with_j": ["-s", "-l", "3", "-J", "1", "-j", tab]}[how]
    want = every_way(oracle, tmp_path, extra, sam, gtf, reads.n, split_with_table=how == "s_with_j")
    text = open(want["summary"]).read()
    assert all(int(re.search(r"^%s\t(\d+)$" % k, text, re.M).group(1)) > 0 for k in ("Added_Novel_Transcripts", "Added_Novel_Exons", "Updated_Genes", "Genes_of_Known_Transcripts_from_BAM"))
