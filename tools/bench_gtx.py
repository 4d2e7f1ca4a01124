"""Diagnostics on the GPU box: the engine side of the GTF text of `lr2rmats bam2gtf` (l2r_gtftext_rows with the exon chains of a run,
l2r_gtftext_blocks, l2r_gtftext_lines + l2r_gtftext_out) on the records of a BASELINE workload and on an ONT-like set with long chains.
Not part of the product.
    tools/bench_gtx.py [reads of cfg3 = 10000000] [reads of the ONT-like set = 1000000] [rounds = 3]
(`make -C lr2rmats_amd/csrc gtx-host` first: the host routine is timed in a program of its own.)

Per set the reads are run once with an empty annotation, as the command runs them; their exon chains stay in HBM.  Then, over `rounds`
warm passes (median and spread): the wall time of the whole blocks + lines + out sequence -- the measure kernel, the download of the
lengths, per batch the scan, the write kernel and the download of the text -- and the text bytes per second that makes; from ONE more
pass with L2R_GTX_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel.  Beside them, from the same
run: k_bed_write's device time and text bytes per second on the same records (l2r_bed_lines with L2R_BED_TIMING=1), and gtx_text_host
(csrc/l2r_gtftextplan.hip.h) over the whole set on one core of this host, which is also the check of the text (two byte sums of both).
One JSON line per set."""
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
from tests import gtf_text_cases as gc                              # noqa: E402

n_cfg3 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
n_ont = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
GTX_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "gtx_host")
BATCH, TEXT_MAX = 1 << 20, 1 << 30


def names_of(n):
    """The QNAME table "read%08d\\0" and the ids into it; the same bytes as (name_off, blob) for l2r_bed_lines."""
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10
    rows = np.concatenate([np.tile(np.frombuffer(b"read", np.uint8), (n, 1)), (digits + 48).astype(np.uint8), np.zeros((n, 1), np.uint8)], axis=1)
    return rows.reshape(-1), (np.arange(n, dtype=np.int64) * 13).astype(np.uint32), np.arange(n + 1, dtype=np.int64) * 12, np.ascontiguousarray(rows[:, :12]).reshape(-1)


def sums_of(sums, text, at):
    """The two sums gtx_dump makes of a text of gigabytes, continued over the bytes ``text`` at position ``at``."""
    for a in range(0, len(text), 1 << 26):
        part = text[a:a + (1 << 26)].astype(np.uint64)
        sums[0] += int(part.sum())
        sums[1] += int((part * (1 + (np.arange(at + a, at + a + len(part), dtype=np.uint64) % 251))).sum())


def host_routine(case, tmp):
    """(seconds of gtx_text_host on one core, the sums of its text, its bytes)"""
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "text.bin")
    with open(src, "wb") as fh:
        fh.write(gc.case_file(case, 0, BATCH, TEXT_MAX, sums_only=1))
    r = subprocess.run([GTX_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    secs = float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1))
    raw = open(dst, "rb").read()
    os.remove(src); os.remove(dst)
    sums = np.frombuffer(raw[-16:], "<u8")
    return secs, [int(sums[0]) % (1 << 64), int(sums[1]) % (1 << 64)], int(re.search(r"(\d+) bytes", r.stderr.decode()).group(1))


def one_pass(eng, n, buf, sums=None):
    """blocks + lines + out over the rows that are in place: (bytes, lines, stats behind the last batch, direct tiles, tiles)"""
    n_lines, n_bytes = eng.gtftext_blocks(n)
    first, got, direct, tiles = 0, 0, 0, 0
    while first < n:
        k, text = eng.gtftext_lines(first, BATCH, TEXT_MAX, buf=buf)
        first += k
        if sums is not None:
            sums_of(sums, text, got)
            st = eng.gtftext_stats()
            direct += int(st["tiles_direct"]); tiles += int(st["tiles_lds"] + st["tiles_direct"])
        got += len(text)
    assert got == n_bytes
    return n_bytes, n_lines, eng.gtftext_stats(), direct, tiles


def bed_write(eng, reads, refs, blob12, name_off):
    """(device ms of k_bed_write, bytes of the BED12 text) over the same records, cut as `bam2bed` cuts them"""
    cols = ((reads.flag_rev.astype(np.uint16) << 4), reads.tid.astype(np.int32), reads.pos.astype(np.int32), np.full(reads.n, 60, np.uint8),
            reads.cig_off.astype(np.int64), reads.cig.astype(np.uint32))
    flag, tid, pos, mapq, cig_off, cig = cols
    eng.bed_begin(refs)
    os.environ["L2R_BED_TIMING"] = "1"
    ms, n_bytes, at = 0.0, 0, 0
    for rnd in range(2):                                             # (the first pass warms buffers and code objects)
        ms, n_bytes, at = 0.0, 0, 0
        while at < reads.n:
            k = capi.bed_cut(flag, tid, (cig_off, cig), (name_off, blob12), refs, at, BATCH, TEXT_MAX)
            n_bytes += len(eng.bed_lines(flag[at:at + k], tid[at:at + k], pos[at:at + k], mapq[at:at + k], (cig_off[at:at + k + 1], cig), (name_off[at:at + k + 1], blob12)))
            ms += eng.bed_stats()["k_bed_write"]
            at += k
    del os.environ["L2R_BED_TIMING"]
    return ms, n_bytes


eng = capi.Engine(0)
cfg = workload.CONFIGS["cfg3"]
t0 = time.perf_counter()
anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
sets = [("cfg3", synth.make_reads(anno, n_cfg3, cfg["n_exons"], cfg["seed"] * 1000)),
        ("ONT-like (cfg5's read model)", synth.make_reads(anno, n_ont, 12, 5000, ont=True, micro_exons=3))]
print("inputs made in %.1f s" % (time.perf_counter() - t0), flush=True)
refs = [c.encode() for c in anno.chrom_names]
with tempfile.TemporaryDirectory() as tmp:
    for label, reads in sets:
        n = reads.n
        table, ids, name_off, blob12 = names_of(n)
        eng.set_params(capi.default_params())
        eng.set_outputs(capi.WANT_RESULTS)
        eng.set_annotation([], [], [], [], [0], [], [])
        eng.set_junctions(None)
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        eng.run()
        eng.sync()
        res = eng.download()
        n_exons = int(res.ex_off[-1])
        eng.gtftext_begin(refs, b"lr2rmats", capi.GTX_PLAIN)
        eng.gtftext_rows(reads.tid, reads.rev, None, None, None, table, ids, ids)
        buf = np.zeros(TEXT_MAX + 64, np.uint8)
        one_pass(eng, n, buf)                                        # warm: buffers, code objects
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter(); n_bytes = one_pass(eng, n, buf)[0]; walls.append(time.perf_counter() - t0)
        os.environ["L2R_GTX_TIMING"] = "1"
        sums = [0, 0]
        n_bytes, n_lines, st, direct, tiles = one_pass(eng, n, buf, sums)
        del os.environ["L2R_GTX_TIMING"]
        ms = {k: st[k] for k in ("k_gtx_measure", "k_scan_u32", "k_gtx_write")}
        bed_ms, bed_bytes = bed_write(eng, reads, refs, blob12, name_off)
        case = {"form": 0, "source": b"lr2rmats", "refs": refs, "tid": reads.tid, "rev": reads.rev, "ex_off": res.ex_off, "xs": res.ex_start[:n_exons], "xe": res.ex_end[:n_exons],
                "table": table.tobytes(), "gid": ids, "tids": ids, "gname": ids, "tname": ids, "sel": None, "start": None, "end": None, "cov": None, "m": n}
        host_s, host_sums, host_bytes = host_routine(case, tmp)
        ok = host_sums == [sums[0] % (1 << 64), sums[1] % (1 << 64)] and host_bytes == n_bytes
        walls.sort()
        med = walls[len(walls) // 2]
        out = dict(set=label, blocks=n, exons_per_block=n_exons / max(n, 1), lines=n_lines, text_bytes=n_bytes, rounds=rounds, measure_form=int(st["wave_form"]),
                   batches=int(st["batches"]), tiles=tiles, tiles_direct=direct, sequence_s_median=med, sequence_s_min=walls[0], sequence_s_max=walls[-1],
                   text_bytes_per_s_sequence=n_bytes / med, kernel_ms=sum(ms.values()), kernel_ms_each={k: round(v, 4) for k, v in ms.items()},
                   text_bytes_per_s_k_gtx_write=n_bytes / (ms["k_gtx_write"] / 1e3) if ms["k_gtx_write"] else 0.0,
                   k_bed_write_ms=round(bed_ms, 4), bed_text_bytes=bed_bytes, text_bytes_per_s_k_bed_write=bed_bytes / (bed_ms / 1e3) if bed_ms else 0.0,
                   gtx_text_host_s=host_s, text_bytes_per_s_host=host_bytes / host_s if host_s else 0.0, sequence_vs_host=host_s / med, equals_host_routine=bool(ok))
        print("| kernel (%s) | ms (all batches, every launch waited for) |\n|---|---|" % label)
        for k, v in ms.items():
            print("| %s | %.3f |" % (k, v))
        print("| k_bed_write (same records) | %.3f |" % bed_ms)
        print(json.dumps(out), flush=True)
        assert ok
eng.close()
