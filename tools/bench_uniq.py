"""Diagnostics on the GPU box: the engine side of `lr2rmats unique-gtf` (l2r_uniq_merge + l2r_uniq_out) on the exon chains of config 3's
records and on the heavy-tailed-isoform workload (cfg3_gencode).  Not part of the product.
    tools/bench_uniq.py [reads per set = 10000000] [rounds = 5] [sets = cfg3,cfg3_gencode]
(`make -C lr2rmats_amd/csrc uniq-host` first: the host routine is timed in a program of its own.)

Per set the engine first makes the exons of every record (empty annotation, as the command does).  Then, over `rounds` warm calls
(median, minimum and maximum): the wall time of l2r_uniq_merge + l2r_uniq_out on the device route -- upload of the columns, the kernels,
download of the verdicts -- and from ONE more call with L2R_SORT_TIMING=1 (every launch group bracketed by HIP events and waited for) the
device time per kernel group.  Beside them uniq_host (csrc/l2r_uniqplan.hip.h) over the whole set on one core of this host, `rounds`
times in the program of its own (the code path without the device route) -- also the check of every output array.  One JSON line per set."""
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
UNIQ_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "uniq_host")
ARRAYS = ("merged", "uniq_of", "u_src", "u_start", "u_end", "u_cov")
GROUPS = capi.UNIQ_STAT_NAMES[9:]


def read_dump(path):
    out = {}
    with open(path, "rb") as fh:
        while True:
            head = fh.read(40)
            if not head:
                return out
            name, typ = head[:24].split(b"\0")[0].decode(), head[24:32].split(b"\0")[0].decode()
            out[name] = np.frombuffer(fh.read(struct.unpack("<q", head[32:])[0] * np.dtype(typ).itemsize), typ)


def host_routine(cols, tmp, times):
    """(seconds of uniq_host on one core, one per run; the arrays of the last run)"""
    tid, rev, ex_off, xs, xe = cols
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<8q", len(tid), len(xs), 0, 0, 0x7fffffff, int(np.float32(0.8).view(np.uint32)), len(ex_off), 0))
        for a in cols:
            fh.write(memoryview(np.ascontiguousarray(a)))
    secs = []
    for _ in range(times):
        r = subprocess.run([UNIQ_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        secs.append(float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1)))
    got = read_dump(dst)
    os.remove(src); os.remove(dst)
    return secs, got


def call(eng, cols):
    t0 = time.perf_counter()
    out = eng.uniq_merge(*cols)
    return time.perf_counter() - t0, out


eng = capi.Engine(0)
with tempfile.TemporaryDirectory() as tmp:
    for label in names:
        cfg = workload.CONFIGS[label]
        t0 = time.perf_counter()
        anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
        reads = synth.make_reads(anno, n_reads, cfg["n_exons"], cfg["seed"] * 1000)
        z32, z8 = np.zeros(0, np.int32), np.zeros(0, np.uint8)
        eng.set_annotation(z32, z32, z32, z8, np.zeros(1, np.int64), z32, z32)
        eng.set_junctions(None)
        res = eng.classify(reads, capi.default_params())
        cols = (np.ascontiguousarray(reads.tid, np.int32), np.ascontiguousarray(reads.rev, np.uint8), np.ascontiguousarray(res.ex_off, np.int64),
                np.ascontiguousarray(res.ex_start, np.int32), np.ascontiguousarray(res.ex_end, np.int32))
        print("%s: inputs and exons made in %.1f s" % (label, time.perf_counter() - t0), flush=True)
        call(eng, cols)                                              # warm: buffers, code objects
        walls = sorted(call(eng, cols)[0] for _ in range(rounds))
        os.environ["L2R_SORT_TIMING"] = "1"
        _, out = call(eng, cols)
        del os.environ["L2R_SORT_TIMING"]
        st = eng.uniq_stats()
        host_s, host = host_routine(cols, tmp, rounds)
        host_s.sort()
        ok = all(np.array_equal(out[k], host[k]) for k in ARRAYS)
        med, hmed = walls[len(walls) // 2], host_s[len(host_s) // 2]
        line = dict(set=label, transcripts=len(cols[0]), exons=len(cols[3]), unique=int(st["unique"]), clusters=int(st["clusters"]), largest_cluster=int(st["largest_cluster"]),
                    route=int(st["route"]), hits=[int(st[k]) for k in ("hits_identical", "hits_contained", "hits_single")], end_extensions=int(st["end_extensions"]),
                    rounds=rounds, call_s_median=med, call_s_min=walls[0], call_s_max=walls[-1], kernel_ms_each={k: round(st[k], 4) for k in GROUPS},
                    kernel_ms=sum(st[k] for k in GROUPS), uniq_host_s_median=hmed, uniq_host_s_min=host_s[0], uniq_host_s_max=host_s[-1],
                    call_vs_host=hmed / med, slowest_call_vs_fastest_host=host_s[0] / walls[-1], equals_host_routine=bool(ok))
        print("| kernel group (%s) | ms (every launch group waited for) |\n|---|---|" % label)
        for k in GROUPS:
            print("| %s | %.3f |" % (k, st[k]))
        print(json.dumps(line), flush=True)
        assert ok
eng.close()
