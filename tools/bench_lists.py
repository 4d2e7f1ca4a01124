"""Diagnostics on the GPU box: the engine side of the read lists of `lr2rmats update-gtf -a / -k / -v / -u` (l2r_gtftext_reads with the
results of a run where they lie in HBM, l2r_gtftext_list, l2r_gtftext_lines + l2r_gtftext_out) on the records of a BASELINE workload and
on an ONT-like set, classified against their annotation with a junction table and -s.  Not part of the product.
    tools/bench_lists.py [reads of cfg3 = 10000000] [reads of the ONT-like set = 1000000] [rounds = 3]
(`make -C lr2rmats_amd/csrc lists-host` first: the host routine is timed in a program of its own.)

Per set the reads are run once without a junction table; from that run's exon chains a junction table is made (80 % of the junctions
seen), and the reads are run again with it and -s -J 1, as the pipeline's second pass runs them; their results stay in HBM.  Then, per
list, over `rounds` warm passes (median and spread): the wall time of the whole list + lines + out sequence -- select, scan, take, the
measure kernel, the download of the lengths, per batch the scan, the write kernel and the download of the text -- and the text bytes per
second that makes; from ONE more pass with L2R_GTX_TIMING=1 (every launch bracketed by HIP events and waited for) the device time of the
selection, the measure and the write.  Beside them, from the same run: k_gtx_write's device time and text bytes per second on the same
records (form PLAIN over the run's chains), and rl_select + rl_text_host (csrc/l2r_readlistplan.hip.h) over the whole set on one core of
this host, which is also the check of the text (two byte sums per list).  One JSON line per set."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from lr2rmats_amd import capi, synth, workload                      # noqa: E402
from tests import read_list_cases as rc                             # noqa: E402
from tests import read_list_restatement as rr                       # noqa: E402

n_cfg3 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
n_ont = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
LISTS_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "lists_host")
BATCH, TEXT_MAX = 1 << 20, 1 << 30
LIST_NAME = {rr.ALL: "all", rr.KNOWN: "known", rr.NOVEL: "novel", rr.UNRECOG: "unrecognised"}


def names_of(n):
    """The QNAME table "read%08d\\0" and the ids into it."""
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10
    rows = np.concatenate([np.tile(np.frombuffer(b"read", np.uint8), (n, 1)), (digits + 48).astype(np.uint8), np.zeros((n, 1), np.uint8)], axis=1)
    return rows.reshape(-1), (np.arange(n, dtype=np.int64) * 13).astype(np.uint32)


def sums_of(sums, text, at):
    """The two sums lists_dump makes of a text of gigabytes, continued over the bytes ``text`` at position ``at``."""
    for a in range(0, len(text), 1 << 26):
        part = text[a:a + (1 << 26)].astype(np.uint64)
        sums[0] += int(part.sum())
        sums[1] += int((part * (1 + (np.arange(at + a, at + a + len(part), dtype=np.uint64) % 251))).sum())


def host_routine(case, tmp):
    """Per list: (seconds of rl_select, seconds of rl_text_host on one core, the sums of its text, its bytes)"""
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "text.bin")
    with open(src, "wb") as fh:
        fh.write(rc.case_file(case, 0, BATCH, TEXT_MAX, sums_only=1))
    r = subprocess.run([LISTS_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    os.remove(src); os.remove(dst)
    out = {}
    for m in re.finditer(r"list (\d), (\d+) blocks, (\d+) lines, (\d+) bytes, select ([0-9.]+) s, text ([0-9.]+) s", r.stderr.decode()):
        out[int(m.group(1))] = (float(m.group(5)), float(m.group(6)), int(m.group(4)))
    return out


def run(eng, af, reads, sj, split):
    eng.set_params(capi.default_params(full_level=3, split_trans=split, min_sj_cnt=1))
    eng.set_outputs(capi.WANT_RESULTS)
    eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    eng.set_junctions(sj)
    eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    eng.run()
    eng.sync()


def one_pass(eng, lst, buf, sums=None):
    """list + lines + out over the reads that are in place: (blocks, bytes, stats behind the last batch, the selection's ms)"""
    m, _, n_bytes = eng.gtftext_list(lst)
    select_ms = eng.gtftext_stats()["k_rl_select"]
    first, got = 0, 0
    while first < m:
        k, text = eng.gtftext_lines(first, BATCH, TEXT_MAX, buf=buf)
        first += k
        if sums is not None:
            sums_of(sums, text, got)
        got += len(text)
    assert got == n_bytes
    return m, n_bytes, eng.gtftext_stats(), select_ms


def gtx_write(eng, reads, refs, table, ids, buf):
    """(device ms of k_gtx_write, bytes of the GTF text) over the chains of the same run, form PLAIN"""
    eng.gtftext_begin(refs, b"lr2rmats", capi.GTX_PLAIN)
    eng.gtftext_rows(reads.tid, reads.rev, None, None, None, table, ids, ids)
    os.environ["L2R_GTX_TIMING"] = "1"
    ms, n_bytes = 0.0, 0
    for rnd in range(2):                                             # (the first pass warms buffers and code objects)
        _, n_bytes = eng.gtftext_blocks(reads.n)
        first = 0
        while first < reads.n:
            first += eng.gtftext_lines(first, BATCH, TEXT_MAX, buf=buf)[0]
        ms = eng.gtftext_stats()["k_gtx_write"]
    del os.environ["L2R_GTX_TIMING"]
    return ms, n_bytes


eng = capi.Engine(0)
cfg = workload.CONFIGS["cfg3"]
t0 = time.perf_counter()
anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
af = anno.in_file_order()
sets = [("cfg3", synth.make_reads(anno, n_cfg3, cfg["n_exons"], cfg["seed"] * 1000)),
        ("ONT-like (cfg5's read model)", synth.make_reads(anno, n_ont, 12, 5000, ont=True, micro_exons=3))]
print("inputs made in %.1f s" % (time.perf_counter() - t0), flush=True)
refs = [c.encode() for c in anno.chrom_names]
genes = [af.gene_id(g).encode() for g in range(af.n_genes)] + [af.gene_name(g).encode() for g in range(af.n_genes)]
anno_names, gene_ids = rr.pack_table(genes)
gene_ids = np.asarray(gene_ids, np.uint32)
tx_gid, tx_gname = gene_ids[af.tx_gene], gene_ids[af.n_genes + af.tx_gene]
with tempfile.TemporaryDirectory() as tmp:
    for label, reads in sets:
        n = reads.n
        table, ids = names_of(n)
        run(eng, af, reads, None, 0)
        base = eng.download()
        j = synth.make_junctions(af, base.ex_off, base.ex_start, base.ex_end, reads.tid, 7, cover=0.8)
        run(eng, af, reads, (j.tid, j.don, j.acc, j.uniq, j.multi), 1)
        res = eng.download()
        n_exons = int(res.ex_off[-1])
        buf = np.zeros(TEXT_MAX + 64, np.uint8)
        case = {"refs": refs, "src": b"lr2rmats", "tid": reads.tid, "names": table.tobytes(), "qname": ids, "tid_name": None, "anno": anno_names, "tx_gid": tx_gid,
                "tx_gname": tx_gname, "ex_off": res.ex_off, "xs": res.ex_start[:n_exons], "xe": res.ex_end[:n_exons], "f": res.ex_flag[:n_exons], "info": res.info[:n],
                "ref_tx": res.ref_tx[:n], "has_sj": True, "split": True}
        host = host_routine(case, tmp)
        eng.gtftext_begin(refs, b"lr2rmats", capi.GTX_READ)
        eng.gtftext_anno(anno_names, tx_gid, tx_gname)
        eng.gtftext_reads(reads.tid, table, ids, None, None, True, True)
        per_list, ok = {}, True
        for lst in rr.LISTS:
            one_pass(eng, lst, buf)                                  # warm: buffers, code objects
            walls = []
            for _ in range(rounds):
                t0 = time.perf_counter(); one_pass(eng, lst, buf); walls.append(time.perf_counter() - t0)
            os.environ["L2R_GTX_TIMING"] = "1"
            sums = [0, 0]
            m, n_bytes, st, select_ms = one_pass(eng, lst, buf, sums)
            del os.environ["L2R_GTX_TIMING"]
            walls.sort()
            med = walls[len(walls) // 2]
            h_sel, h_text, h_bytes = host.get(lst, (0.0, 0.0, -1))
            ok = ok and h_bytes == n_bytes
            write_ms = st["k_gtx_write"]
            per_list[LIST_NAME[lst]] = dict(blocks=m, piece_blocks=int(st["piece_blocks"]), text_bytes=n_bytes, measure_form=int(st["wave_form"]), sequence_s_median=med,
                                            sequence_s_min=walls[0], sequence_s_max=walls[-1], text_bytes_per_s_sequence=n_bytes / med if med else 0.0,
                                            select_ms=round(select_ms, 4), measure_ms=round(st["k_gtx_measure"], 4), scan_ms=round(st["k_scan_u32"], 4), write_ms=round(write_ms, 4),
                                            text_bytes_per_s_k_rl_write=n_bytes / (write_ms / 1e3) if write_ms else 0.0, rl_select_host_s=h_sel, rl_text_host_s=h_text,
                                            text_bytes_per_s_host=h_bytes / h_text if h_text else 0.0, equals_host_bytes=h_bytes == n_bytes)
        gtx_ms, gtx_bytes = gtx_write(eng, reads, refs, table, ids, buf)
        out = dict(set=label, reads=n, exons_per_read=n_exons / max(n, 1), rounds=rounds, lists=per_list, k_gtx_write_ms=round(gtx_ms, 4), gtx_text_bytes=gtx_bytes,
                   text_bytes_per_s_k_gtx_write=gtx_bytes / (gtx_ms / 1e3) if gtx_ms else 0.0)
        print("| list (%s) | blocks | select ms | measure ms | write ms | text GB/s of the write kernel |\n|---|---|---|---|---|---|" % label)
        for k, v in per_list.items():
            print("| %s | %d | %.3f | %.3f | %.3f | %.1f |" % (k, v["blocks"], v["select_ms"], v["measure_ms"], v["write_ms"], v["text_bytes_per_s_k_rl_write"] / 1e9))
        print("| k_gtx_write, form PLAIN (same records) | %d | | | %.3f | %.1f |" % (n, gtx_ms, out["text_bytes_per_s_k_gtx_write"] / 1e9))
        print(json.dumps(out), flush=True)
        assert ok
eng.close()
