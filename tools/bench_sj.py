"""Diagnostics on the GPU box: the engine side of `lr2rmats bam2sj` (l2r_sj_begin / _add / _finish) on synthetic short-read records.
Not part of the product.   tools/bench_sj.py [records = 50_000_000] [rounds = 5] [batch = 8_388_608]

Reports, over `rounds` warm rounds (median and spread): wall time of add + finish with uploads, rows/s; then from ONE more round with
L2R_SJ_TIMING=1 (every launch bracketed by HIP events and waited for) the device time per kernel, the bytes the algorithm moves
divided by the kernel time as a fraction of 8 TB/s, and the radix passes that ran; and the wall time of the numpy restatement
(np.unique + np.bincount, tests/sj_restatement.py) on the same rows on this host -- the only yardstick there is.

A second leg runs the same records through the table of `lr2rmats sjtab` (l2r_sj_begin_tab + l2r_sj_annotate + l2r_sj_filter_rows2 with
STAR's defaults for the distance and the intron-size lists, six columns per row instead of five) and prints a second JSON line
("leg": "sjtab"): the same figures, the device time of every new kernel, the ratio of its scatter passes to the plain leg's (24 / 20 by
the bytes per row), and for the neighbour stage the rows it saw and dropped, the passes of the acceptor order, bytes moved / time per
kernel and the acceptor order's time per row and pass beside k_radix_scatter<SjRows>'s.  The synthetic table has no genome, so every row has motif 0.
L2R_BENCH_SJ_LEGS=plain runs the first leg only."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from lr2rmats_amd import capi                      # noqa: E402
from tests import sj_restatement as sr            # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 23


def make(n, seed=1, n_chrom=24, n_intron=12000, span=100_000_000):
    """Coordinate-sorted records, a third with one or two N between fixed introns (about n_chrom * n_intron junctions), vectorised."""
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.integers(0, n_chrom, n)).astype(np.int32)
    sites = np.sort(rng.integers(1000, span, (n_chrom, 2 * n_intron)), axis=1)
    spliced = rng.random(n) < 0.34
    k = np.where(spliced, rng.integers(1, 3, n), 0)                       # introns per record
    j0 = rng.integers(0, n_intron - 2, n)
    don0, acc0 = sites[tid, 2 * j0], sites[tid, 2 * j0 + 1]
    don1, acc1 = sites[tid, 2 * j0 + 2], sites[tid, 2 * j0 + 3]
    lead = rng.integers(5, 70, n)
    pos = np.where(spliced, don0 - lead, rng.integers(0, span, n)).astype(np.int32)
    n_ops = 1 + 2 * k
    off = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int64)
    cig = np.empty(off[-1], np.uint32)
    m = lambda ln: (np.maximum(ln, 1).astype(np.uint32) << 4)
    s0 = off[:-1]
    cig[s0] = np.where(spliced, m(lead), m(rng.integers(50, 151, n)))
    a = spliced
    cig[s0[a] + 1] = m(acc0[a] - don0[a]) | 3
    cig[s0[a] + 2] = np.where(k[a] == 2, m(don1[a] - acc0[a]), m(rng.integers(5, 70, a.sum())))
    b = k == 2
    cig[s0[b] + 3] = m(acc1[b] - don1[b]) | 3
    cig[s0[b] + 4] = m(rng.integers(5, 70, b.sum()))
    order = np.lexsort((pos, tid))                                        # coordinate sorted
    lens = n_ops[order]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.repeat(off[:-1][order] - new_off[:-1], lens) + np.arange(new_off[-1])
    flag = np.full(n, 3, np.uint16); flag[rng.random(n) < 0.05] = 1; flag[rng.random(n) < 0.02] |= 4
    uniq = (rng.random(n) < 0.8).astype(np.uint8)
    return dict(flag=flag, tid=tid[order], pos=pos[order], uniq=uniq, cig_off=new_off, cig=cig[idx])


def add_all(eng, r):
    for a in range(0, len(r["flag"]), batch):
        b = min(a + batch, len(r["flag"]))
        c0, c1 = r["cig_off"][a], r["cig_off"][b]
        eng.sj_add(r["flag"][a:b], r["tid"][a:b], r["pos"][a:b], r["uniq"][a:b], r["cig_off"][a:b + 1] - c0, r["cig"][c0:c1])


def run(eng, r):
    eng.sj_begin()
    add_all(eng, r)
    return eng.sj_finish()


def run_tab(eng, r, anno):
    """The `sjtab` leg: pair_only as in the plain leg (the same records make the same rows), annotate, default filter with both stages."""
    eng.sj_begin_tab(pair_only=True)
    add_all(eng, r)
    full = eng.sj_finish()
    eng.sj_annotate(*anno)
    return full, eng.sj_filter_rows2(dist_min=capi.SJ_FILTER2_STAR[0], intron_max=capi.SJ_FILTER2_STAR[1])


t0 = time.perf_counter()
r = make(n)
print("input: %d records, %d CIGAR operations (made in %.1f s)" % (n, len(r["cig"]), time.perf_counter() - t0), flush=True)
eng = capi.Engine(0)
run(eng, r)                                                               # warm: buffers, code objects
walls = []
for _ in range(rounds):
    t0 = time.perf_counter(); tab = run(eng, r); walls.append(time.perf_counter() - t0)
st = eng.sj_stats()
os.environ["L2R_SJ_TIMING"] = "1"
run(eng, r)
tm = eng.sj_stats()
del os.environ["L2R_SJ_TIMING"]
rows, out_rows, passes = st["rows_made"], len(tab.tid), int(tm["radix_passes"])
kern = {k: v for k, v in tm.items() if k.startswith("k_")}
kernel_ms = sum(kern.values())
# bytes the algorithm has to move: records in (15 B + 4 B per op), rows out 20 B and in again for hist12 (12 B); per pass 4 B of keys for
# the tile histograms and 20 B in + 20 B out for the scatter; heads 12 B + 4, reduce 28 B (summed over the rounds' rows where there are several)
rows_sorted = rows if st["rounds"] == 1 else None
moved = 15 * n + 4 * len(r["cig"]) + 20 * rows + (12 + passes * 44 + 16 + 28) * rows
t0 = time.perf_counter()
want = sr.table_numpy(*sr.rows_numpy(r["flag"], r["tid"], r["pos"], r["uniq"], r["cig_off"], r["cig"]))
numpy_s = time.perf_counter() - t0
ok = all(np.array_equal(g.astype(np.int64), w) for g, w in zip((tab.tid, tab.don, tab.acc, tab.uniq_c, tab.multi_c), want))
walls.sort()
line = dict(records=n, rows=int(rows), table_rows=out_rows, rounds=rounds, sort_rounds=int(st["rounds"]), radix_passes=passes,
            wall_s_median=walls[len(walls) // 2], wall_s_min=walls[0], wall_s_max=walls[-1], records_per_s=n / walls[len(walls) // 2],
            kernel_ms=kernel_ms, rows_per_s_kernels=rows / (kernel_ms / 1e3) if kernel_ms else 0.0,
            bytes_moved=int(moved), fraction_of_8TBs=(moved / (kernel_ms / 1e3)) / 8e12 if kernel_ms else 0.0,
            numpy_restatement_s=numpy_s, equals_numpy=bool(ok))
print("| kernel | ms (one round, every launch waited for) |\n|---|---|")
for k, v in kern.items():
    print("| %s | %.3f |" % (k, v))
print(json.dumps(line), flush=True)
assert ok
if os.environ.get("L2R_BENCH_SJ_LEGS", "") == "plain":
    sys.exit(0)

# ---- the sjtab leg: the annotation is every second junction of the table as a two-exon transcript, and as many transcripts beside them
from tests import sjtab_restatement as st         # noqa: E402
from tests import sjtab_near_restatement as nr    # noqa: E402
sel = np.arange(len(tab.tid)) % 2 == 0
a_tid = np.concatenate([tab.tid[sel], tab.tid[sel]]).astype(np.int32)
a_don = np.concatenate([tab.don[sel], tab.don[sel] + 7]).astype(np.int64)
a_acc = np.concatenate([tab.acc[sel], tab.acc[sel] + 7]).astype(np.int64)
anno = (a_tid, (2 * np.arange(len(a_tid) + 1)).astype(np.int64), np.stack([a_don - 50, a_acc + 1], axis=1).reshape(-1).astype(np.int32),
        np.stack([a_don - 1, a_acc + 50], axis=1).reshape(-1).astype(np.int32))
run_tab(eng, r, anno)
walls2 = []
for _ in range(rounds):
    t0 = time.perf_counter(); full, kept = run_tab(eng, r, anno); walls2.append(time.perf_counter() - t0)
st2 = eng.sj_stats()
os.environ["L2R_SJ_TIMING"] = "1"
run_tab(eng, r, anno)
tm2 = eng.sj_stats()
del os.environ["L2R_SJ_TIMING"]
kern2 = {k: v for k, v in tm2.items() if k.startswith("k_") or k.startswith("intron sort") or k.startswith("acceptor order")}
kernel_ms2 = sum(kern2.values())
passes2 = int(tm2["radix_passes"])
n_in, n_tab = int(tm2["anno_introns"]), len(full.tid)
# as above with 24 B rows: rows out 24, hist12 12, per pass 4 + 24 + 24, heads 16, reduce 32; the annotation's exons in (8 B) and its introns
# through a sort of their own (counted at 20 B rows and `passes2` passes at most); annotate 12 B + 1 per row; keep 13 B + 4, take 27 B in and out
moved2 = 15 * n + 4 * len(r["cig"]) + 24 * rows + (12 + passes2 * 52 + 16 + 32) * rows + 8 * len(anno[2]) + (20 + 12 + passes2 * 44 + 44) * len(a_tid) + \
    13 * n_tab + 17 * n_tab + 54 * len(kept.tid)
# the neighbour stage over the n1 rows stage 1 left: keys 8 B in + 8 out; per pass of the acceptor order 8 B for the tile histograms and 12 + 12 for
# the scatter; near_acc 4 B index + 8 gathered + 4 out; keep_near 8 + 4 + 2 in, 4 out; its take 27 B in over n1 and out over the kept rows
n1 = len(kept.tid) + int(tm2["rows_dropped_near"])
acc_passes = int(tm2["acc_radix_passes"])
near_bytes = {"k_radix_keys<SjAccKeyOf>": 16 * n1, "acceptor order passes": acc_passes * 32 * n1, "k_sj_near_acc": 16 * n1, "k_sj_keep_near": 18 * n1}
moved2 += sum(near_bytes.values()) + 27 * n1
t0 = time.perf_counter()
want6 = st.table_numpy(*st.rows_numpy(r["flag"], r["tid"], r["pos"], r["uniq"], r["cig_off"], r["cig"], pair_only=True))
numpy_s2 = time.perf_counter() - t0
introns = set(zip(a_tid.tolist(), a_don.tolist(), a_acc.tolist()))
an = st.anno_numpy(introns, want6[0], want6[1], want6[2])
zero = np.zeros(len(an), np.int64)
keep = nr.filter2_numpy([want6[0], want6[1], want6[2], zero, zero, an, want6[3], want6[4], want6[5]], st.DEFAULT_FILTER, nr.STAR_DIST, nr.STAR_INTRON_MAX)["keep"]
ok2 = all(np.array_equal(g.astype(np.int64), w) for g, w in zip((full.tid, full.don, full.acc, full.uniq_c, full.multi_c, full.max_over), want6)) and \
    all(np.array_equal(g.astype(np.int64), w[keep]) for g, w in zip((kept.tid, kept.don, kept.acc, kept.uniq_c, kept.multi_c, kept.max_over), want6)) and \
    np.array_equal(kept.anno, an[keep])
walls2.sort()
line2 = dict(leg="sjtab", records=n, rows=int(st2["rows_made"]), table_rows=n_tab, kept_rows=len(kept.tid), anno_introns=n_in, rounds=rounds,
             radix_passes=passes2, wall_s_median=walls2[len(walls2) // 2], wall_s_min=walls2[0], wall_s_max=walls2[-1],
             records_per_s=n / walls2[len(walls2) // 2], kernel_ms=kernel_ms2, bytes_moved=int(moved2),
             fraction_of_8TBs=(moved2 / (kernel_ms2 / 1e3)) / 8e12 if kernel_ms2 else 0.0,
             scatter_ms=tm2["k_radix_scatter<SjRows>"], scatter_ms_plain=tm["k_radix_scatter<SjRows>"],
             scatter_ratio_to_plain=(tm2["k_radix_scatter<SjRows>"] / passes2) / (tm["k_radix_scatter<SjRows>"] / passes) if passes and passes2 and tm["k_radix_scatter<SjRows>"] else 0.0,
             stage1_rows=n1, rows_dropped_near=int(tm2["rows_dropped_near"]), rows_dropped_long=int(tm2["rows_dropped_long"]), acc_radix_passes=acc_passes,
             near_GBs={k: (b / (tm2[k] / 1e3)) / 1e9 if tm2[k] else 0.0 for k, b in near_bytes.items()},
             acc_order_ps_per_row_pass=tm2["acceptor order passes"] * 1e9 / (n1 * acc_passes) if n1 and acc_passes else 0.0,
             scatter_ps_per_row_pass=tm2["k_radix_scatter<SjRows>"] * 1e9 / (st2["rows_in"] * passes2) if passes2 and st2["rows_in"] else 0.0,
             numpy_restatement_s=numpy_s2, equals_numpy=bool(ok2))
print("| kernel (sjtab leg) | ms (one round, every launch waited for) |\n|---|---|")
for k, v in kern2.items():
    print("| %s | %.3f |" % (k, v))
print(json.dumps(line2))
assert ok2
