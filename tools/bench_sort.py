"""Diagnostics on the GPU box: the engine side of `lr2rmats sort` / `filter -S` (l2r_sort_order) on the records of a BASELINE workload.
Not part of the product.   tools/bench_sort.py [config = cfg3] [rounds = 7]

The records of the workload (cfg3: 10 M, coordinate sorted as the generator leaves them) are measured in two forms, shuffled and
already sorted.  Per form, over `rounds` warm calls (median and spread): the wall time of the whole l2r_sort_order call -- upload of
10 B per record, kernels, download of the order, the call ends with a wait for the device; then from ONE more call with
L2R_SORT_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel, the radix passes that ran, the
bytes the algorithm moves per row and scatter pass and what that is per second.  Beside them numpy.argsort(kind="stable") of the same
keys on this host, which is also the check of the order.  One JSON line per form."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lr2rmats_amd import capi, workload            # noqa: E402

cfg_name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7

t0 = time.perf_counter()
_, reads = workload.make_rank_workload(workload.CONFIGS[cfg_name], 0, 1)
n = int(reads.n)
flag = (np.asarray(reads.flag_rev, np.uint16) << 4).astype(np.uint16)
tid, pos = np.ascontiguousarray(reads.tid, np.int32), np.ascontiguousarray(reads.pos, np.int32)
print("input: %s, %d records on %d references (made in %.1f s)" % (cfg_name, n, int(tid.max()) + 1, time.perf_counter() - t0), flush=True)
perm = np.random.default_rng(1).permutation(n)
forms = {"shuffled": (flag[perm], tid[perm], pos[perm]), "sorted": (flag, tid, pos)}

eng = capi.Engine(0)
for form, (f, t, p) in forms.items():
    f, t, p = np.ascontiguousarray(f), np.ascontiguousarray(t), np.ascontiguousarray(p)
    key = capi.sort_keys(f, t, p)
    eng.sort_order(f, t, p)                                               # warm: buffers, code objects
    walls = []
    for _ in range(rounds):
        t0 = time.perf_counter(); order = eng.sort_order(f, t, p); walls.append(time.perf_counter() - t0)
    os.environ["L2R_SORT_TIMING"] = "1"
    eng.sort_order(f, t, p)
    tm = eng.sort_stats()
    del os.environ["L2R_SORT_TIMING"]
    t0 = time.perf_counter()
    want = np.argsort(key, kind="stable")
    numpy_s = time.perf_counter() - t0
    ok = np.array_equal(order, want.astype(np.uint32))
    passes = int(tm["radix_passes"])
    kern = {k: v for k, v in tm.items() if k.startswith("k_")}
    kernel_ms = sum(kern.values())
    # bytes the algorithm has to move: the keys 10 B in + 8 B out per row; per pass 8 B of keys for the tile histograms and 12 B in +
    # 12 B out for the scatter, less the index column the first pass does not read (4 B) and the key column the last does not write (8 B)
    scatter_bytes = (24 * passes - 12) * n if passes else 0
    moved = 18 * n + 8 * passes * n + scatter_bytes
    walls.sort()
    line = dict(form=form, config=cfg_name, records=n, rounds=rounds, radix_passes=passes, in_order=int(tm["in_order"]),
                call_s_median=walls[len(walls) // 2], call_s_min=walls[0], call_s_max=walls[-1], records_per_s_call=n / walls[len(walls) // 2],
                kernel_ms=kernel_ms, kernel_ms_each={k: round(v, 4) for k, v in kern.items()},
                scatter_ms_per_pass=tm["k_radix_scatter<SortRows>"] / passes if passes else 0.0,
                scatter_bytes_per_row_and_pass=scatter_bytes / (passes * n) if passes else 0.0,
                scatter_TB_per_s=(scatter_bytes / (tm["k_radix_scatter<SortRows>"] / 1e3)) / 1e12 if passes and tm["k_radix_scatter<SortRows>"] else 0.0,
                bytes_moved=int(moved), fraction_of_8TBs=(moved / (kernel_ms / 1e3)) / 8e12 if kernel_ms else 0.0,
                numpy_stable_argsort_s=numpy_s, equals_numpy=bool(ok))
    print("| kernel (%s) | ms (one call, every launch waited for) |\n|---|---|" % form)
    for k, v in kern.items():
        print("| %s | %.3f |" % (k, v))
    print(json.dumps(line), flush=True)
    assert ok
eng.close()
