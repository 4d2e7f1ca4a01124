"""Diagnostics on the GPU box: the engine side of `lr2rmats sort-gtf` (l2r_gtf_order) on the annotation of a BASELINE workload.  Not part
of the product.   tools/bench_gtf.py [config = cfg3] [rounds = 5]
(`make -C lr2rmats_amd/csrc gtf-host` first: the host routine is timed in a program of its own.)

The annotation of the config is written with synth.Annotation.write_gtf and brought into the order once; then three forms of it are
timed: in order; that file followed by a copy of a tenth of its transcripts (what the pipeline hands the command: an annotation with
update-gtf output appended); whole transcripts shuffled.  Per form, over `rounds` warm calls (median and spread): the wall time of the
whole l2r_gtf_order call -- upload of the text, kernels, the heads to the host and their ranks back, download of three words per kept
line and of the order; then from ONE more call with L2R_SORT_TIMING=1 (every launch bracketed by HIP events and waited for) the device
time per kernel group.  The two line kernels each read every byte of the text once, so their bytes per second are 2 * bytes over their
time, set against the 6.29 TB/s a copy kernel reaches on this device.  Beside them, from the same run:
gtf_order_host (csrc/l2r_gtforder.hip.h) on one core of this host, which is also the check of the rows.  One JSON line per form."""
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
from lr2rmats_amd import capi, hostlib, synth, workload            # noqa: E402

cfg_name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
GTF_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "gtf_host")
COPY_TB_S = 6.29


def host_routine(path, tmp):
    """(seconds of gtf_order_host on one core, its line column)"""
    dst = os.path.join(tmp, "rows.bin")
    r = subprocess.run([GTF_HOST, path, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    secs = float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1))
    raw = open(dst, "rb").read()
    at = raw.index(b"line\0")
    count = struct.unpack_from("<q", raw, at + 32)[0]
    return secs, np.frombuffer(raw, "<u4", count, at + 40)


eng = capi.Engine(0)
with tempfile.TemporaryDirectory() as tmp:
    t0 = time.perf_counter()
    cfg = workload.CONFIGS[cfg_name]
    anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
    raw_path, sorted_path = os.path.join(tmp, "anno.gtf"), os.path.join(tmp, "in_order.gtf")
    anno.write_gtf(raw_path)
    raw = open(raw_path, "rb").read()
    hostlib.gtf_write_rows(raw, *eng.gtf_order(raw), sorted_path)
    in_order = open(sorted_path, "rb").read()
    lines = in_order.split(b"\n")[:-1]
    heads = [k for k, ln in enumerate(lines) if ln.split(b"\t", 3)[2] == b"transcript"] + [len(lines)]
    blocks = [lines[a:b] for a, b in zip(heads, heads[1:])]
    rng = np.random.default_rng(1)
    tenth = [blocks[int(i)] for i in np.sort(rng.permutation(len(blocks))[:len(blocks) // 10])]
    forms = [("in order", in_order),
             ("in order + a copy of a tenth of the transcripts", in_order + b"".join(ln + b"\n" for b in tenth for ln in b)),
             ("transcripts shuffled", b"".join(ln + b"\n" for i in rng.permutation(len(blocks)) for ln in blocks[int(i)]))]
    del raw, lines, blocks, tenth
    print("input: %s, %d bytes, %d transcripts (made in %.1f s)" % (cfg_name, len(in_order), len(heads) - 1, time.perf_counter() - t0), flush=True)
    for form, text in forms:
        eng.gtf_order(text)                                                   # warm: buffers, code objects
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter(); rows = eng.gtf_order(text); walls.append(time.perf_counter() - t0)
        os.environ["L2R_SORT_TIMING"] = "1"
        eng.gtf_order(text)
        tm = eng.gtf_stats()
        del os.environ["L2R_SORT_TIMING"]
        path = os.path.join(tmp, "form.gtf")
        with open(path, "wb") as fh:
            fh.write(text)
        host_s, want = host_routine(path, tmp)
        ok = np.array_equal(rows[2], want)
        walls.sort()
        kern = {k: v for k, v in list(tm.items())[10:16]}
        line_ms = tm["k_gtf_count + k_gtf_starts"]
        line_tb_s = 2 * len(text) / (line_ms / 1e3) / 1e12 if line_ms else 0.0
        out = dict(form=form, config=cfg_name, bytes=len(text), lines=int(tm["lines"]), rows=int(tm["rows"]), transcripts=int(tm["transcripts"]), heads=int(tm["heads"]),
                   rounds=rounds, passes_stage1=int(tm["passes_stage1"]), passes_stage2=int(tm["passes_stage2"]), identity=int(tm["identity"]), route=int(tm["route"]),
                   call_s_median=walls[len(walls) // 2], call_s_min=walls[0], call_s_max=walls[-1], bytes_per_s_call=len(text) / walls[len(walls) // 2],
                   kernel_ms=sum(kern.values()), kernel_ms_each={k: round(v, 4) for k, v in kern.items()},
                   line_kernels_TB_per_s=line_tb_s, line_kernels_share_of_copy=line_tb_s / COPY_TB_S,
                   gtf_order_host_s=host_s, call_vs_host=host_s / walls[len(walls) // 2], equals_host_routine=bool(ok))
        print("| kernel (%s) | ms (one call, every launch waited for) |\n|---|---|" % form)
        for k, v in kern.items():
            print("| %s | %.3f |" % (k, v))
        print(json.dumps(out), flush=True)
        assert ok
eng.close()
