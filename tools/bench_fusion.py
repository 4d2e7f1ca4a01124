"""Diagnostics on the GPU box: device time (HIP events, L2R_FUSION_TIMING=1) of the kernels of `lr2rmats fusion` -- both forms of
k_fusion_seg and k_fusion_select -- on synthetic records at 8 and at 300 operations a record, and beside them k_filter_score /
k_filter_select on the SAME records: the yardstick (same bytes in, same access pattern: one pass over the CIGAR words per record,
one pass over the rows per group).  Prints per kernel the best of the repeats, and the bytes the kernel has to move / that time.
No threshold is set.  Not part of the product.

    tools/bench_fusion.py [records at 8 ops] [records at 300 ops] [repeats]        (default 10 M, 10 M, 5)
"""
import json
import os
import sys

import numpy as np

os.environ["L2R_FUSION_TIMING"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lr2rmats_amd import capi  # noqa: E402

HBM_PEAK = 8.0e12


def make_records(rng, n, ops):
    """n records of `ops` operations each (a leading clip on a third of them), in pieces so that the host arrays stay small."""
    off = np.arange(n + 1, dtype=np.int64) * ops
    cig = np.empty(n * ops, np.uint32)
    step = max(1, (1 << 26) // ops)
    for a in range(0, n, step):
        b = min(n, a + step)
        m = (b - a) * ops
        op = rng.choice(np.array([0, 0, 0, 1, 2, 3, 7, 8], np.uint32), size=m)
        op[::ops][rng.random(b - a) < 0.33] = 4
        cig[a * ops:b * ops] = (rng.integers(1, 200, m, dtype=np.uint32) << 4) | op
    flag = (np.where(rng.random(n) < 0.02, 4, 0) | np.where(rng.random(n) < 0.5, 16, 0)).astype(np.uint16)
    return flag, rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 3_000_000, n).astype(np.int32), off, cig


def best(f, key, repeats, eng):
    t = []
    for _ in range(repeats + 1):                            # the first call is the warm-up
        out = f()
        t.append(eng.fusion_stats()[key])
    return min(t[1:]), out


def main():
    n8 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    n300 = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(10)
    eng = capi.Engine(0)
    report = {}
    for n, ops in ((n8, 8), (n300, 300)):
        flag, tid, pos, off, cig = make_records(rng, n, ops)
        row = {"records": n, "ops_per_record": ops}
        seg_bytes = 4 * n * ops + n * (2 + 4 + 8) + 20 * n              # CIGAR words + flag, pos, cig_off in; five words out
        for wave in ("0", "1"):
            os.environ["L2R_FUSION_WAVE"] = wave
            ms, seg = best(lambda: eng.fusion_segments(flag, pos, off, cig), "k_fusion_seg", repeats, eng)
            row["k_fusion_seg_%s_ms" % ("wave" if wave == "1" else "thread")] = ms
            row["k_fusion_seg_%s_frac_of_8TBs" % ("wave" if wave == "1" else "thread")] = seg_bytes / (ms * 1e-3) / HBM_PEAK if ms else None
        os.environ.pop("L2R_FUSION_WAVE")
        row["k_fusion_seg_bytes"] = seg_bytes
        # the yardstick on the same records
        l_qseq = seg[4]; nm = rng.integers(0, 50, n).astype(np.int32)
        fprm = capi.CFilterParams(0.67, 0.75, 0.98, 0)
        ms, (drop, fscore, intron) = best(lambda: eng.filter_score(flag, tid, pos, l_qseq, nm, off, cig, fprm), "k_filter_score", repeats, eng)
        sc_bytes = 4 * n * ops + n * (2 + 4 + 4 + 4 + 4 + 8) + 9 * n
        row.update(k_filter_score_ms=ms, k_filter_score_bytes=sc_bytes, k_filter_score_frac_of_8TBs=sc_bytes / (ms * 1e-3) / HBM_PEAK if ms else None)
        # groups of 1..6 mapped records
        rows = np.nonzero((flag & 4) == 0)[0]
        gl = rng.integers(1, 7, rows.size); goff = np.concatenate([[0], np.cumsum(gl)]); goff = goff[goff < rows.size]
        goff = np.concatenate([goff, [rows.size]]).astype(np.int64)
        G, R = goff.size - 1, rows.size
        cols = [x[rows] for x in seg[:4]]
        score = rng.integers(0, 1000, R).astype(np.int32); ed = rng.integers(0, 50, R).astype(np.int32)
        rlen = seg[4][rows[goff[:-1]]]
        prm = capi.CFusionParams(0.1, 0.1, 0.99, 100000)
        ms, _ = best(lambda: eng.fusion_select(goff, score, ed, tid[rows], cols[0], cols[1], cols[2], cols[3], rlen, prm), "k_fusion_select", repeats, eng)
        sel_bytes = 8 * G + 28 * R + 4 * G + 16 * G
        row.update(groups=int(G), k_fusion_select_ms=ms, k_fusion_select_bytes=sel_bytes, k_fusion_select_frac_of_8TBs=sel_bytes / (ms * 1e-3) / HBM_PEAK if ms else None)
        ms, _ = best(lambda: eng.filter_select(goff, score, ed, fprm), "k_filter_select", repeats, eng)
        fsel_bytes = 8 * G + 8 * R + 8 * G
        row.update(k_filter_select_ms=ms, k_filter_select_bytes=fsel_bytes, k_filter_select_frac_of_8TBs=fsel_bytes / (ms * 1e-3) / HBM_PEAK if ms else None)
        report["ops_%d" % ops] = row
        del cig
    eng.close()
    print(json.dumps(report, indent=1))


if __name__ == "__main__":
    main()
