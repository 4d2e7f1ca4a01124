"""Diagnostics on the GPU box: the engine side of the detail table of `lr2rmats update-gtf -A` (l2r_detail_rows with the results of a run
where they lie in HBM, l2r_detail_lines + l2r_detail_out) on the records of a BASELINE workload and on an ONT-like set, classified against
their annotation.  Not part of the product.
    tools/bench_detail.py [reads of cfg3 = 10000000] [reads of the ONT-like set = 1000000] [rounds = 3]
(`make -C lr2rmats_amd/csrc detail-host` first: the host routine is timed in a program of its own.)

Per set the reads are run once against the annotation, as the command runs them; their results stay in HBM.  Then, over `rounds` warm
passes (median and spread): the wall time of the whole rows + lines + out sequence -- the upload of the name ids, the measure kernel, the
download of the lengths, per batch the scan, the write kernel and the download of the text -- and the text bytes per second that makes;
from ONE more pass with L2R_DETAIL_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel.  Beside
them, from the same run: k_gtx_write's device time and text bytes per second on the same records (l2r_gtftext_* over the run's chains,
L2R_GTX_TIMING=1), and detail_text_host (csrc/l2r_detailplan.hip.h) over the whole set on one core of this host, which is also the check
of the text (two byte sums of both).  One JSON line per set."""
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
from tests import detail_cases as dc                                # noqa: E402
from tests import detail_restatement as dr                          # noqa: E402

n_cfg3 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
n_ont = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DETAIL_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "detail_host")
BATCH, TEXT_MAX = 1 << 20, 1 << 30


def names_of(n):
    """The QNAME table "read%08d\\0" and the ids into it."""
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10
    rows = np.concatenate([np.tile(np.frombuffer(b"read", np.uint8), (n, 1)), (digits + 48).astype(np.uint8), np.zeros((n, 1), np.uint8)], axis=1)
    return rows.reshape(-1), (np.arange(n, dtype=np.int64) * 13).astype(np.uint32)


def sums_of(sums, text, at):
    """The two sums detail_dump makes of a text of gigabytes, continued over the bytes ``text`` at position ``at``."""
    for a in range(0, len(text), 1 << 26):
        part = text[a:a + (1 << 26)].astype(np.uint64)
        sums[0] += int(part.sum())
        sums[1] += int((part * (1 + (np.arange(at + a, at + a + len(part), dtype=np.uint64) % 251))).sum())


def host_routine(case, tmp):
    """(seconds of detail_text_host on one core, the sums of its text, its bytes)"""
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "text.bin")
    with open(src, "wb") as fh:
        fh.write(dc.case_file(case, 0, BATCH, TEXT_MAX, sums_only=1))
    r = subprocess.run([DETAIL_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    secs = float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1))
    raw = open(dst, "rb").read()
    os.remove(src); os.remove(dst)
    sums = np.frombuffer(raw[-16:], "<u8")
    return secs, [int(sums[0]) % (1 << 64), int(sums[1]) % (1 << 64)], int(re.search(r"(\d+) bytes", r.stderr.decode()).group(1))


def one_pass(eng, reads, table, ids, buf, sums=None):
    """rows + lines + out over the results that are in place: (bytes, stats behind the last batch, direct tiles, tiles)"""
    n = reads.n
    n_bytes = eng.detail_rows(reads.tid, table, ids)
    first, got, direct, tiles = 0, 0, 0, 0
    while first < n:
        k, text = eng.detail_lines(first, BATCH, TEXT_MAX, buf=buf)
        first += k
        if sums is not None:
            sums_of(sums, text, got)
            st = eng.detail_stats()
            direct += int(st["tiles_direct"]); tiles += int(st["tiles_lds"] + st["tiles_direct"])
        got += len(text)
    assert got == n_bytes
    return n_bytes, eng.detail_stats(), direct, tiles


def gtx_write(eng, reads, refs, table, ids, buf):
    """(device ms of k_gtx_write, bytes of the GTF text) over the chains of the same run"""
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
anno_names, gene_ids = dr.pack_table(genes)
gene_ids = np.asarray(gene_ids, np.uint32)
tx_gid, tx_gname = gene_ids[af.tx_gene], gene_ids[af.n_genes + af.tx_gene]
with tempfile.TemporaryDirectory() as tmp:
    for label, reads in sets:
        n = reads.n
        table, ids = names_of(n)
        eng.set_params(capi.default_params(full_level=3))
        eng.set_outputs(capi.WANT_RESULTS)
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(None)
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        eng.run()
        eng.sync()
        res = eng.download()
        n_exons = int(res.ex_off[-1])
        eng.detail_begin(refs, anno_names, tx_gid, tx_gname)
        buf = np.zeros(TEXT_MAX + 64, np.uint8)
        one_pass(eng, reads, table, ids, buf)                        # warm: buffers, code objects
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter(); n_bytes = one_pass(eng, reads, table, ids, buf)[0]; walls.append(time.perf_counter() - t0)
        os.environ["L2R_DETAIL_TIMING"] = "1"
        sums = [0, 0]
        n_bytes, st, direct, tiles = one_pass(eng, reads, table, ids, buf, sums)
        del os.environ["L2R_DETAIL_TIMING"]
        ms = {k: st[k] for k in ("k_detail_measure", "k_scan_u32", "k_detail_write")}
        gtx_ms, gtx_bytes = gtx_write(eng, reads, refs, table, ids, buf)
        case = {"refs": refs, "tid": reads.tid, "names": table.tobytes(), "qname": ids, "anno": anno_names, "tx_gid": tx_gid, "tx_gname": tx_gname, "ex_off": res.ex_off,
                "xs": res.ex_start[:n_exons], "xe": res.ex_end[:n_exons], "f": res.ex_flag[:n_exons], "info": res.info[:n], "ref_tx": res.ref_tx[:n]}
        host_s, host_sums, host_bytes = host_routine(case, tmp)
        ok = host_sums == [sums[0] % (1 << 64), sums[1] % (1 << 64)] and host_bytes == n_bytes
        walls.sort()
        med = walls[len(walls) // 2]
        out = dict(set=label, rows=n, exons_per_row=n_exons / max(n, 1), text_bytes=n_bytes, rounds=rounds, measure_form=int(st["wave_form"]),
                   batches=int(st["batches"]), tiles=tiles, tiles_direct=direct, sequence_s_median=med, sequence_s_min=walls[0], sequence_s_max=walls[-1],
                   text_bytes_per_s_sequence=n_bytes / med, kernel_ms=sum(ms.values()), kernel_ms_each={k: round(v, 4) for k, v in ms.items()},
                   text_bytes_per_s_k_detail_write=n_bytes / (ms["k_detail_write"] / 1e3) if ms["k_detail_write"] else 0.0,
                   k_gtx_write_ms=round(gtx_ms, 4), gtx_text_bytes=gtx_bytes, text_bytes_per_s_k_gtx_write=gtx_bytes / (gtx_ms / 1e3) if gtx_ms else 0.0,
                   detail_text_host_s=host_s, text_bytes_per_s_host=host_bytes / host_s if host_s else 0.0, sequence_vs_host=host_s / med, equals_host_routine=bool(ok))
        print("| kernel (%s) | ms (all batches, every launch waited for) |\n|---|---|" % label)
        for k, v in ms.items():
            print("| %s | %.3f |" % (k, v))
        print("| k_gtx_write (same records) | %.3f |" % gtx_ms)
        print(json.dumps(out), flush=True)
        assert ok
eng.close()
