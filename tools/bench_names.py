"""Diagnostics on the GPU box: the engine side of `lr2rmats sort -n` / `filter -N` / `fusion -N` (l2r_name_order) on the names of a BASELINE
workload.  Not part of the product.   tools/bench_names.py [config = cfg3] [rounds = 5]
(`make -C lr2rmats_amd/csrc name-host` first: the host routine is timed in a program of its own.)

The records of the workload (cfg3: 10 M) get the names read%08d with 1.3 alignments per read (every read one record, three in ten a
second one), the alignments of a read anywhere on the references, in three arrangements: name-grouped; that file in coordinate
order (numpy's stable argsort of the sort keys); fully shuffled.  Per arrangement, over `rounds` warm calls (median and spread): the
wall time of the whole l2r_name_order call -- upload of 8 B of offsets and the name bytes per record, kernels, download of the order;
then from ONE more call with L2R_SORT_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel.
Beside them, from the same run: name_order_host (csrc/l2r_nameorder.hip.h) on one core of this host, which is also the check of the
order, and l2r_sort_order on the same records with its kernel times.  The hash + heads kernels are set against sort's keys kernel +
one scatter pass as bytes per second: the hash reads 8 B of offsets and the name and writes 8 B, the heads kernel reads per row the
index (4 B), a gathered hash (8 B) and -- only where two neighbours have one hash -- two names and their offsets, and writes 4 B;
sort's keys kernel reads 10 B and writes 8 B, a middle scatter pass reads and writes 12 B.  One JSON line per arrangement."""
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
from lr2rmats_amd import capi, workload            # noqa: E402

cfg_name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
NAME_HOST = os.path.join(ROOT, "lr2rmats_amd", "lib", "name_host")
NAME_LEN = 12

t0 = time.perf_counter()
_, reads = workload.make_rank_workload(workload.CONFIGS[cfg_name], 0, 1)
n = int(reads.n)
rng = np.random.default_rng(1)
# the grouped file: read ids 0, 0, 1, 2, 2, 3 ...; the alignments of a read lie anywhere
rid = np.repeat(np.arange(n, dtype=np.int64), 1 + (rng.random(n) < 0.3))[:n]
where = rng.permutation(n)
flag = (np.asarray(reads.flag_rev, np.uint16) << 4).astype(np.uint16)[where]
tid, pos = np.asarray(reads.tid, np.int32)[where], np.asarray(reads.pos, np.int32)[where]
by_coord = np.argsort(capi.sort_keys(flag, tid, pos), kind="stable")
shuffle = rng.permutation(n)
print("input: %s, %d records of %d reads (made in %.1f s)" % (cfg_name, n, int(rid[-1]) + 1, time.perf_counter() - t0), flush=True)


def names_of(ids):
    blob = np.empty((ids.size, NAME_LEN), np.uint8)
    blob[:, :4] = np.frombuffer(b"read", np.uint8)
    v = ids.copy()
    for k in range(NAME_LEN - 1, 3, -1):
        blob[:, k] = 48 + v % 10
        v //= 10
    return np.arange(ids.size + 1, dtype=np.int64) * NAME_LEN, blob.reshape(-1)


def host_routine(off, blob, tmp):
    """(seconds of name_order_host on one core, its order)"""
    src, dst = os.path.join(tmp, "case.bin"), os.path.join(tmp, "order.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<q", off.size - 1)); fh.write(off.tobytes()); fh.write(blob.tobytes())
    r = subprocess.run([NAME_HOST, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
    secs = float(re.search(r"([0-9.]+) s", r.stderr.decode()).group(1))
    raw = open(dst, "rb").read()
    at = raw.index(b"order")
    count = struct.unpack_from("<q", raw, at + 32)[0]
    return secs, np.frombuffer(raw, "<u4", count, at + 40)


eng = capi.Engine(0)
with tempfile.TemporaryDirectory() as tmp:
    for form, perm in (("name-grouped", None), ("coordinate order", by_coord), ("shuffled", shuffle)):
        ids = rid if perm is None else rid[perm]
        f, t, p = (np.ascontiguousarray(x if perm is None else x[perm]) for x in (flag, tid, pos))
        names = names_of(ids)
        eng.name_order(names)                                                 # warm: buffers, code objects
        walls = []
        for _ in range(rounds):
            t0 = time.perf_counter(); order, groups = eng.name_order(names); walls.append(time.perf_counter() - t0)
        os.environ["L2R_SORT_TIMING"] = "1"
        eng.name_order(names)
        tm = eng.name_stats()
        eng.sort_order(f, t, p)
        sm = eng.sort_stats()
        del os.environ["L2R_SORT_TIMING"]
        eng.sort_order(f, t, p)
        t0 = time.perf_counter(); eng.sort_order(f, t, p); sort_call = time.perf_counter() - t0
        host_s, want = host_routine(names[0], names[1], tmp)
        ok = np.array_equal(order, want)
        walls.sort()
        kern = {k: v for k, v in list(tm.items())[6:]}
        sort_passes = int(sm["radix_passes"])
        hash_ms, heads_ms = tm["k_radix_keys<NameHashOf>"], tm["k_name_heads"]
        hash_bytes, heads_bytes = (8 + NAME_LEN + 8) * n, (4 + 8 + 4) * n        # (heads: without the names of equal-hash neighbours)
        line = dict(form=form, config=cfg_name, records=n, groups=groups, rounds=rounds, radix_passes=int(tm["radix_passes"]), identity=int(tm["identity"]),
                    route=int(tm["route"]), mismatches=int(tm["mismatches"]),
                    call_s_median=walls[len(walls) // 2], call_s_min=walls[0], call_s_max=walls[-1], records_per_s_call=n / walls[len(walls) // 2],
                    kernel_ms=sum(kern.values()), kernel_ms_each={k: round(v, 4) for k, v in kern.items()},
                    name_order_host_s=host_s, call_vs_host=host_s / walls[len(walls) // 2],
                    hash_TB_per_s=hash_bytes / (hash_ms / 1e3) / 1e12 if hash_ms else 0.0, heads_TB_per_s=heads_bytes / (heads_ms / 1e3) / 1e12 if heads_ms else 0.0,
                    sort_call_s=sort_call, sort_radix_passes=sort_passes, sort_kernel_ms_each={k: round(v, 4) for k, v in sm.items() if k.startswith("k_")},
                    sort_keys_TB_per_s=18 * n / (sm["k_radix_keys<SortKeyOf>"] / 1e3) / 1e12 if sm["k_radix_keys<SortKeyOf>"] else 0.0,
                    sort_scatter_ms_per_pass=sm["k_radix_scatter<SortRows>"] / sort_passes if sort_passes else 0.0,
                    sort_scatter_TB_per_s=24 * n / (sm["k_radix_scatter<SortRows>"] / sort_passes / 1e3) / 1e12 if sort_passes and sm["k_radix_scatter<SortRows>"] else 0.0,
                    equals_host_routine=bool(ok))
        print("| kernel (%s) | ms (one call, every launch waited for) |\n|---|---|" % form)
        for k, v in kern.items():
            print("| %s | %.3f |" % (k, v))
        print(json.dumps(line), flush=True)
        assert ok
eng.close()
