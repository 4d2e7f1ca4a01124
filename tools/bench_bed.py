"""Diagnostics on the GPU box: the engine side of `lr2rmats bam2bed` (l2r_bed_lines + l2r_bed_text_out) on the records of a BASELINE
workload and on an ONT-like set with long CIGARs.  Not part of the product.
    tools/bench_bed.py [reads of cfg3 = 10000000] [reads of the ONT-like set = 1000000] [rounds = 3]
(`make -C lr2rmats_amd/csrc bed-host` first: the host routine is timed in a program of its own.)

The records are cut into batches as the command cuts them (l2r_bed_cut: 1 Mi records, 1 GiB of summed line bounds).  Per set, over
`rounds` warm passes over all batches (median and spread): the wall time of the l2r_bed_lines + l2r_bed_text_out calls -- upload of the
columns, the three kernels, download of the text -- and the text bytes per second that makes; then from ONE more pass with
L2R_BED_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel.  Beside them, from the same run:
bed_lines_host (csrc/l2r_bedplan.hip.h) over the whole set on one core of this host, which is also the check of the text (MD5 of both).
One JSON line per set."""
import hashlib
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

n_cfg3 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
n_ont = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
BED_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "bed_host")
BATCH, TEXT_MAX = 1 << 20, 1 << 30


def columns(reads):
    n = reads.n
    digits = (np.arange(n, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1)) % 10
    blob = np.concatenate([np.tile(np.frombuffer(b"read", np.uint8), (n, 1)), (digits + 48).astype(np.uint8)], axis=1).reshape(-1)
    name_off = np.arange(n + 1, dtype=np.int64) * 12
    return ((reads.flag_rev.astype(np.uint16) << 4), reads.tid.astype(np.int32), reads.pos.astype(np.int32), np.full(n, 60, np.uint8),
            reads.cig_off.astype(np.int64), reads.cig.astype(np.uint32), name_off, blob)


def host_routine(cols, refs, tmp):
    """(seconds of bed_lines_host on one core, MD5 of its text, its bytes)"""
    flag, tid, pos, mapq, cig_off, cig, name_off, blob = cols
    ref_off, ref_blob = capi.pack_names(refs)
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "text.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<8q", len(flag), len(cig), len(refs), 7, 0, BATCH, TEXT_MAX, 0))
        for a in (flag, tid, pos, mapq, cig_off, cig, name_off, blob, ref_off, ref_blob):
            fh.write(memoryview(np.ascontiguousarray(a)))
        fh.write(b"255,0,0")
    r = subprocess.run([BED_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    secs = float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1))
    raw = np.memmap(dst, np.uint8, "r")
    at = 0
    while bytes(raw[at:at + 5]) != b"text\0":                        # the members in front of `text`: rc, bound, cut, lines_rc
        typ = bytes(raw[at + 24:at + 32]).split(b"\0")[0].decode()
        at += 40 + int(np.frombuffer(bytes(raw[at + 32:at + 40]), "<i8")[0]) * np.dtype(typ).itemsize
    count = int(np.frombuffer(bytes(raw[at + 32:at + 40]), "<i8")[0])
    md5 = hashlib.md5(memoryview(raw[at + 40:at + 40 + count])).hexdigest()
    os.remove(src); os.remove(dst)
    return secs, md5, count


def one_pass(eng, cols, cuts, md5=None):
    flag, tid, pos, mapq, cig_off, cig, name_off, blob = cols
    n_bytes, ms = 0, {"k_bed_measure": 0.0, "k_scan_u32": 0.0, "k_bed_write": 0.0}
    forms, direct, tiles = set(), 0, 0
    for a, b in zip(cuts, cuts[1:]):
        text = eng.bed_lines(flag[a:b], tid[a:b], pos[a:b], mapq[a:b], (cig_off[a:b + 1], cig), (name_off[a:b + 1], blob))
        n_bytes += len(text)
        if md5 is not None:
            md5.update(text)
            st = eng.bed_stats()
            for k in ms:
                ms[k] += st[k]
            forms.add(int(st["wave_form"])); direct += int(st["tiles_direct"]); tiles += int(st["tiles_lds"] + st["tiles_direct"])
    return n_bytes, ms, sorted(forms), direct, tiles


eng = capi.Engine(0)
cfg = workload.CONFIGS["cfg3"]
t0 = time.perf_counter()
anno = synth.make_annotation(cfg["anno_exons"], cfg["seed"], mean_tx_exons=cfg["n_exons"] + 1, tx_per_gene=cfg.get("tx_per_gene", 5))
sets = [("cfg3", synth.make_reads(anno, n_cfg3, cfg["n_exons"], cfg["seed"] * 1000)),
        ("ONT-like (cfg5's read model)", synth.make_reads(anno, n_ont, 12, 5000, ont=True, micro_exons=3))]
print("inputs made in %.1f s" % (time.perf_counter() - t0), flush=True)
refs = [c.encode() for c in anno.chrom_names]
eng.bed_begin(refs)
with tempfile.TemporaryDirectory() as tmp:
    for label, reads in sets:
        cols = columns(reads)
        flag, tid, pos, mapq, cig_off, cig, name_off, blob = cols
        cuts = [0]
        while cuts[-1] < reads.n:
            cuts.append(cuts[-1] + capi.bed_cut(flag, tid, (cig_off, cig), (name_off, blob), refs, cuts[-1], BATCH, TEXT_MAX))
        one_pass(eng, cols, cuts)                                    # warm: buffers, code objects
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter(); n_bytes = one_pass(eng, cols, cuts)[0]; walls.append(time.perf_counter() - t0)
        os.environ["L2R_BED_TIMING"] = "1"
        md5 = hashlib.md5()
        n_bytes, ms, forms, direct, tiles = one_pass(eng, cols, cuts, md5)
        del os.environ["L2R_BED_TIMING"]
        host_s, host_md5, host_bytes = host_routine(cols, refs, tmp)
        ok = host_md5 == md5.hexdigest() and host_bytes == n_bytes
        walls.sort()
        med = walls[len(walls) // 2]
        out = dict(set=label, records=reads.n, operations_per_record=len(cig) / max(reads.n, 1), batches=len(cuts) - 1, text_bytes=n_bytes, rounds=rounds,
                   measure_forms=forms, tiles=tiles, tiles_direct=direct, call_s_median=med, call_s_min=walls[0], call_s_max=walls[-1],
                   text_bytes_per_s_call=n_bytes / med, kernel_ms=sum(ms.values()), kernel_ms_each={k: round(v, 4) for k, v in ms.items()},
                   text_bytes_per_s_kernels=n_bytes / (sum(ms.values()) / 1e3) if sum(ms.values()) else 0.0,
                   bed_lines_host_s=host_s, text_bytes_per_s_host=host_bytes / host_s if host_s else 0.0, call_vs_host=host_s / med, equals_host_routine=bool(ok))
        print("| kernel (%s) | ms (all batches, every launch waited for) |\n|---|---|" % label)
        for k, v in ms.items():
            print("| %s | %.3f |" % (k, v))
        print(json.dumps(out), flush=True)
        assert ok
eng.close()
