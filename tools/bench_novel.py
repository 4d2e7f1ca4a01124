"""Diagnostics on the GPU box: the engine side of the novel list of `lr2rmats update-gtf` (l2r_novel_begin, l2r_novel_add with the results
of a run where they lie in HBM, l2r_novel_finish, the BED text through l2r_novel_lines) on config 3's records and on the
heavy-tailed-isoform workload (cfg3_gencode), classified against their annotation.  Not part of the product.
    tools/bench_novel.py [reads per set = 10000000] [rounds = 5] [sets = cfg3,cfg3_gencode]
(`make -C lr2rmats_amd/csrc novel-host` first: the host routine is timed in a program of its own.)

Per set the reads are run against the annotation with `-l 3` and no junction table -- the pipeline's first call, in which no read is
split -- and the results stay in HBM.  Then, over `rounds` warm passes (median, minimum and maximum): the wall time of the whole begin +
add + finish + text -- the upload of tid, the selection, the merge, the items, their order and compaction, the download of the gene rows,
the counters and the text -- and from ONE more pass with L2R_SORT_TIMING=1 (every launch group bracketed by HIP events and waited for)
the device time per kernel group, with the clusters and the largest cluster, through which k_uniq_merge walks on one wave.  Beside them
novel_host (csrc/l2r_novelplan.hip.h: uniq_host over the offers and the literal backward scans) over the whole set on one core of this
host, `rounds` times in the program of its own -- also the check of the counts and of the text.  One JSON line per set."""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from lr2rmats_amd import capi, synth, workload                      # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
names = sys.argv[3].split(",") if len(sys.argv) > 3 else ["cfg3", "cfg3_gencode"]
NOVEL_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "novel_host")
GROUPS = capi.NOVEL_STAT_NAMES[25:]
OPTS = dict(force_strand=0, ss_dis=0, end_dis=0x7fffffff, frac=0.8)  # the command's defaults


def read_dump(path):
    out = {}
    with open(path, "rb") as fh:
        while True:
            head = fh.read(40)
            if not head:
                return out
            name, typ = head[:24].split(b"\0")[0].decode(), head[24:32].split(b"\0")[0].decode()
            out[name] = np.frombuffer(fh.read(struct.unpack("<q", head[32:])[0] * np.dtype(typ).itemsize), typ)


def host_routine(tid, res, refs, tx_gene, na_gene, tmp, times):
    """(seconds of novel_host on one core, one per run; the counts and the text of the last run)"""
    n, x = len(tid), int(res.ex_off[-1])
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    blob = b"".join(refs)
    off = np.zeros(len(refs) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in refs])
    with open(src, "wb") as fh:
        fh.write(struct.pack("<14q", n, x, len(refs), len(tx_gene), na_gene, 0, 0, OPTS["force_strand"], OPTS["ss_dis"], OPTS["end_dis"],
                             int(np.float32(OPTS["frac"]).view(np.uint32)), len(blob), 0, 0))
        for a in (np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(res.info[:n], np.uint32), np.ascontiguousarray(res.ref_tx[:n], np.int32),
                  np.ascontiguousarray(res.ex_start[:x], np.int32), np.ascontiguousarray(res.ex_end[:x], np.int32), np.ascontiguousarray(res.ex_flag[:x], np.uint8),
                  np.ascontiguousarray(tx_gene, np.uint32), off):
            fh.write(memoryview(a))
        fh.write(blob)
    secs = []
    for _ in range(times):
        r = subprocess.run([NOVEL_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        secs.append(float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1)))
    got = read_dump(dst)
    os.remove(src); os.remove(dst)
    return secs, [int(v) for v in got["counts"]], got["bed"].tobytes()


def one_pass(eng, tid, refs, tx_gene, na_gene):
    t0 = time.perf_counter()
    eng.novel_begin(refs, tx_gene, na_gene, **OPTS)
    eng.novel_add(tid)
    counts = eng.novel_finish()
    text = eng.novel_text()
    return time.perf_counter() - t0, counts, text


eng = capi.Engine(0)
with tempfile.TemporaryDirectory() as tmp:
    for label in names:
        cfg = workload.CONFIGS[label]
        t0 = time.perf_counter()
        anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
        af = anno.in_file_order()
        reads = synth.make_reads(anno, n_reads, cfg["n_exons"], cfg["seed"] * 1000)
        refs = [c.encode() if isinstance(c, str) else bytes(c) for c in anno.chrom_names]
        tx_gene, na_gene = np.ascontiguousarray(af.tx_gene, np.uint32), int(af.n_genes)
        eng.set_outputs(capi.WANT_RESULTS)
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(None)
        eng.set_params(capi.default_params(full_level=3))
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        eng.run()
        eng.sync()
        res = eng.download()
        tid = np.ascontiguousarray(reads.tid, np.int32)
        print("%s: inputs made and classified in %.1f s" % (label, time.perf_counter() - t0), flush=True)
        one_pass(eng, tid, refs, tx_gene, na_gene)                   # warm: buffers, code objects
        walls = sorted(one_pass(eng, tid, refs, tx_gene, na_gene)[0] for _ in range(rounds))
        os.environ["L2R_SORT_TIMING"] = "1"
        _, counts, text = one_pass(eng, tid, refs, tx_gene, na_gene)
        del os.environ["L2R_SORT_TIMING"]
        st = eng.novel_stats()
        assert st["route"] == 0, "the set is not in order: the host routine ran, there are no kernel times"
        host_s, host_counts, host_text = host_routine(tid, res, refs, tx_gene, na_gene, tmp, rounds)
        host_s.sort()
        ok = counts == host_counts and text == host_text
        med, hmed = walls[len(walls) // 2], host_s[len(host_s) // 2]
        line = dict(set=label, reads=int(st["reads"]), offers=int(st["offers"]), known_reads=int(st["known_reads"]), entries=int(st["entries"]), hits=int(st["hits"]),
                    items={k: int(st["items_" + k]) for k in capi.NOVEL_LIST_NAMES}, kept={k: int(st["kept_" + k]) for k in capi.NOVEL_LIST_NAMES}, bed_bytes=len(text),
                    clusters=int(st["clusters"]), largest_cluster=int(st["largest_cluster"]), route=int(st["route"]), copy_form=int(st["wave_form"]), rounds=rounds,
                    sequence_s_median=med, sequence_s_min=walls[0], sequence_s_max=walls[-1], kernel_ms_each={k: round(st[k], 4) for k in GROUPS}, kernel_ms=sum(st[k] for k in GROUPS),
                    novel_host_s_median=hmed, novel_host_s_min=host_s[0], novel_host_s_max=host_s[-1], sequence_vs_host=hmed / med, equals_host_routine=bool(ok))
        print("| kernel group (%s) | ms (every launch group waited for) |\n|---|---|" % label)
        for k in GROUPS:
            print("| %s | %.3f |" % (k, st[k]))
        print(json.dumps(line), flush=True)
        assert ok
eng.close()
