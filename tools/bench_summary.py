"""Diagnostics on the GPU box: the engine side of the read classes of `lr2rmats update-gtf -y` (l2r_summary_begin, l2r_summary_add with the
results of a run where they lie in HBM, l2r_summary_finish) on config 3's records and on the heavy-tailed-isoform workload
(cfg3_gencode), classified against their annotation.  Not part of the product.
    tools/bench_summary.py [reads per set = 10000000] [rounds = 5] [sets = cfg3,cfg3_gencode]
(`make -C lr2rmats_amd/csrc summary-host` first: the host routine is timed in a program of its own.)

Per set the reads are run against the annotation and a junction table (every annotated junction and 60 % of the reads' own, as bench.py's
second option set makes it) with `-s -l 3 -J 1`, the pipeline's option set, so that all four classes are there; the results stay in HBM.
Then, over `rounds` warm passes (median, minimum and maximum): the wall time of the whole begin + add + finish -- the upload of tid, the copies inside HBM, the
kernels, the download of the counters -- and from ONE more pass with L2R_SORT_TIMING=1 (every launch group bracketed by HIP events and
waited for) the device time per kernel group, with the clusters and the largest cluster, through which k_uniq_merge walks on one wave.
Beside them summary_host (csrc/l2r_summaryplan.hip.h: four uniq_host lists) over the whole set on one core of this host, `rounds` times
in the program of its own -- also the check of the eight counts.  One JSON line per set."""
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
SUMMARY_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "summary_host")
GROUPS = capi.SUMMARY_STAT_NAMES[7:]
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


def host_routine(tid, res, tmp, times):
    """(seconds of summary_host on one core, one per run; the counts of the last run)"""
    n, x = len(tid), int(res.ex_off[-1])
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<8q", n, x, OPTS["force_strand"], OPTS["ss_dis"], OPTS["end_dis"], int(np.float32(OPTS["frac"]).view(np.uint32)), 0, 0))
        for a in (np.ascontiguousarray(tid, np.int32), np.ascontiguousarray(res.info[:n], np.uint32), np.ascontiguousarray(res.ex_start[:x], np.int32),
                  np.ascontiguousarray(res.ex_end[:x], np.int32)):
            fh.write(memoryview(a))
    secs = []
    for _ in range(times):
        r = subprocess.run([SUMMARY_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        secs.append(float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1)))
    got = read_dump(dst)
    os.remove(src); os.remove(dst)
    return secs, [int(v) for v in got["counts"]]


def one_pass(eng, tid):
    t0 = time.perf_counter()
    eng.summary_begin(**OPTS)
    eng.summary_add(tid)
    counts = eng.summary_finish()
    return time.perf_counter() - t0, counts


eng = capi.Engine(0)
with tempfile.TemporaryDirectory() as tmp:
    for label in names:
        cfg = workload.CONFIGS[label]
        t0 = time.perf_counter()
        anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
        af = anno.in_file_order()
        reads = synth.make_reads(anno, n_reads, cfg["n_exons"], cfg["seed"] * 1000)
        eng.set_outputs(capi.WANT_RESULTS)
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(None)
        res = eng.classify(reads, capi.default_params(full_level=3))                # the reads' own junctions, for the table
        j = synth.make_junctions_fast(af, res.ex_off, res.ex_start, res.ex_end, reads.tid, cfg["seed"], cover=0.6)
        eng.set_junctions((j.tid, j.don, j.acc, j.uniq, j.multi))
        eng.set_params(capi.default_params(full_level=3, split_trans=1, min_sj_cnt=1))
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        eng.run()
        eng.sync()
        res = eng.download()
        tid = np.ascontiguousarray(reads.tid, np.int32)
        print("%s: inputs made and classified in %.1f s" % (label, time.perf_counter() - t0), flush=True)
        one_pass(eng, tid)                                           # warm: buffers, code objects
        walls = sorted(one_pass(eng, tid)[0] for _ in range(rounds))
        os.environ["L2R_SORT_TIMING"] = "1"
        _, counts = one_pass(eng, tid)
        del os.environ["L2R_SORT_TIMING"]
        st = eng.summary_stats()
        assert st["route"] == 0, "the set is not in order inside a class: the host routine ran, there are no kernel times"
        host_s, host_counts = host_routine(tid, res, tmp, rounds)
        host_s.sort()
        ok = counts == host_counts
        med, hmed = walls[len(walls) // 2], host_s[len(host_s) // 2]
        line = dict(set=label, reads=int(st["reads"]), exons=int(st["exons"]), counts=dict(zip(capi.SUMMARY_COUNT_NAMES, counts[:4])), unique=dict(zip(capi.SUMMARY_COUNT_NAMES, counts[4:])),
                    clusters=int(st["clusters"]), largest_cluster=int(st["largest_cluster"]), route=int(st["route"]), gather_form=int(st["wave_form"]), rounds=rounds,
                    sequence_s_median=med, sequence_s_min=walls[0], sequence_s_max=walls[-1], kernel_ms_each={k: round(st[k], 4) for k in GROUPS}, kernel_ms=sum(st[k] for k in GROUPS),
                    summary_host_s_median=hmed, summary_host_s_min=host_s[0], summary_host_s_max=host_s[-1], sequence_vs_host=hmed / med, equals_host_routine=bool(ok))
        print("| kernel group (%s) | ms (every launch group waited for) |\n|---|---|" % label)
        for k in GROUPS:
            print("| %s | %.3f |" % (k, st[k]))
        print(json.dumps(line), flush=True)
        assert ok
eng.close()
