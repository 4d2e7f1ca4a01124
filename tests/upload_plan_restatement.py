"""Restatement of the upload's plan (lr2rmats_amd/csrc/l2r_plan.hip.h) in Python: the checker of tests/test_upload_plan_cpu.py, and the
model of the tile cut that tests/test_gpu_tile_split.py tunes its thresholds against.

What l2r_upload_reads decides about a read set before anything is staged, as rules:

* records -- `cig_off` begins at 0, ends at n_cigar and never descends; every record has a reference;
* sorted -- the records are in (tid, pos) order, everything uploaded before them was, and they do not begin in front of its last record;
* sample -- of up to 4096 evenly spaced records, the operations that cut a read into exons (N of at least min_intron, D beyond
  max_delet): `est` exons per read; `many_exon_reads` when more than 0.5 % of the sample have more exons than a slab has rows;
  `wide_cigar` when a record has more than 32 operations on average;
* layouts -- the slab layout for sorted records where it is wanted, with long CIGARs only without `many_exon_reads`; the tile index
  where it is wanted and the CIGARs are short;
* reads per tile -- 256, halved while est * reads * 1.25 exceeds the staged exons (not below 32); without the slab layout also the
  cheapest of 256 / 128 / 64 / 32 by the share of sampled windows whose span the staged directory cannot hold;
* tiles -- runs of that many reads; sorted records: a tile ends with its chromosome, where a read begins 2^17 bases or more behind its
  first read (without the slab layout only after 8 reads), and -- short CIGARs with the slab layout -- where the exon bounds
  (ops + 3) >> 1 of its reads would exceed TILE_POS_CAP;
* slabs -- per tile as many rows of 256 elements as the largest exon bound of its reads that is at most SLAB_ROWS (at least one; long
  CIGARs: SLAB_ROWS); the dense area has a row per operation + 1 of every read (long CIGARs: `exb`, which the engine counts); both
  below 0x7ffffff0 or there is no slab layout;
* index -- with the reader's summaries a tile's statistics are sums, minima and maxima of its records' words; a longest D of 65535
  stands for any length; a read of 255 exons or more, or SLOT_LOC_LIMIT exons in the tile, and the shortest stretch is INT32_MIN
  (the tile is never exact); the tile's last base, clamped to 32 bits, goes into its record;
* super-blocks -- the statistics once more per 1024 tiles, the operation count with the tiles' reads added.

`upload_plan` takes arrays and returns a dict named like the members of UploadPlan.
"""
import numpy as np

from lr2rmats_amd import synth

TILE_READS, TILE_POS_CAP, TILE_SPAN = 256, 2400, 1 << 17        # l2r_slab.hip.h: TILE_THREADS, TILE_POS_CAP, SLAB_TILE_SPAN
LDS_EXON_CAP, SLAB_POS_CAP = 3072, 2536                          # l2r_kernels.hip.h, l2r_slab.hip.h
DIR_CAP, SITE_SHIFT = 384, 9                                     # l2r_kernels.hip.h
SLAB_ROWS, SLAB_STRIDE = 24, 256                                 # l2r_slab.hip.h
SLOT_LOC_LIMIT = 1 << 12                                         # l2r_tile.hip.h
SUP_SHIFT = 10                                                   # l2r_slab.hip.h LB_SUP_SHIFT
LIMIT_31 = 0x7ffffff0
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN = -(1 << 63)
REF_OPS = (0, 2, 3, 7, 8)                                        # M D N = X advance on the reference
EMPTY_STAT = (0, INT32_MAX, 0, INT32_MAX)                        # TileStat: n_ops_n, min_n, max_d, min_seg


class PlanError(Exception):
    pass


def _tile_firsts(reads):
    """The upload's tile cut for coordinate-sorted records with short CIGARs (l2r_upload_reads): runs of up to 256 reads of one
    chromosome that begin less than 2^17 bases apart and whose exon bounds ((ops + 3) >> 1 per read) fit the staged positions."""
    n_ops = np.diff(reads.cig_off)
    firsts, start, pos_sum = [], 0, 0
    for i in range(reads.n):
        need = (int(n_ops[i]) + 3) >> 1
        if i > start and (i - start == TILE_READS or reads.tid[i] != reads.tid[start] or pos_sum + need > TILE_POS_CAP or
                          int(reads.pos[i]) - int(reads.pos[start]) >= TILE_SPAN):
            firsts.append(start)
            start, pos_sum = i, 0
        pos_sum += need
    firsts.append(start)
    return np.array(firsts + [reads.n], np.int64)


def _tile_stats(reads, firsts):
    """TileStat per tile from the records' CIGAR summaries: N operations, the shortest N, the longest D, the shortest inner stretch."""
    s = synth.cigar_summary(reads.cig_off, reads.cig).astype(np.int64)
    n_n, min_n, max_d, min_seg = s[:, 1] & 0xffff, s[:, 1] >> 16, s[:, 2] & 0xffff, s[:, 2] >> 16
    lo = firsts[:-1]
    return (np.add.reduceat(n_n, lo), np.minimum.reduceat(min_n, lo), np.maximum.reduceat(max_d, lo), np.minimum.reduceat(min_seg, lo),
            np.maximum.reduceat(n_n, lo))


def read_key(tid, pos):
    return (int(tid) << 32) | (int(pos) & 0xffffffff)


def check_reads(tid, pos, cig_off, n_cigar):
    """Raises PlanError with the engine's message; returns whether the records are in order among themselves."""
    n = len(tid)
    if n and (cig_off[0] != 0 or cig_off[n] != n_cigar):
        raise PlanError("[l2r_upload_reads] cig_off does not span n_cigar")
    in_order = True
    for i in range(n):
        if tid[i] < 0:
            raise PlanError("[l2r_upload_reads] record %d has no reference (unmapped); the reference aborts on it (bam2gtf.c:100)" % i)
        if cig_off[i + 1] < cig_off[i]:
            raise PlanError("[l2r_upload_reads] cig_off not monotone at %d" % i)
        if i and (tid[i], pos[i]) < (tid[i - 1], pos[i - 1]):
            in_order = False
    return in_order


def exon_sample(cig_off, cig, n, min_intron, max_delet):
    """(est, many_exon_reads)"""
    if n == 0:
        return 1.0, False
    sample = min(n, 4096)
    step = n // sample
    cuts = many = 0
    for s in range(sample):
        i = s * step
        mine = 0
        for w in cig[cig_off[i]:cig_off[i + 1]]:
            op, ln = w & 15, w >> 4
            mine += (op == 3 and ln >= min_intron) or (op == 2 and ln > max_delet)
        cuts += mine
        many += mine + 1 > SLAB_ROWS
    return float(cuts) / float(sample) + 1.0, many * 200 > sample


def reads_per_tile(tid, pos, cig_off, cig, est, in_order, slab_long, slab_layout):
    n = len(tid)
    rpt = TILE_READS
    if n:
        while rpt > 32 and est * rpt * 1.25 > float(SLAB_POS_CAP if slab_long else LDS_EXON_CAP):
            rpt >>= 1
    if not (in_order and n >= 2 * TILE_READS and not slab_layout):
        return rpt
    # sparse input without the slab layout: windows of 256 reads, and for every size the share of them whose first `size` reads span
    # more than the staged directory holds
    n_win = min(n // TILE_READS, 384)
    wstep = (n // TILE_READS) // n_win
    limit = (DIR_CAP - 8) << SITE_SHIFT
    bad = {256: 0, 128: 0, 64: 0, 32: 0}
    for w in range(n_win):
        i0 = w * wstep * TILE_READS
        hi = 0
        for q in range(TILE_READS):
            i = i0 + q
            if i >= n or tid[i] != tid[i0]:
                break
            end = pos[i] + sum(x >> 4 for x in cig[cig_off[i]:cig_off[i + 1]] if (x & 15) in REF_OPS)
            hi = max(hi, end - pos[i0])
            if q + 1 in bad and hi > limit:                     # the first 32 / 64 / 128 / 256 reads: this size and every larger one
                for size in bad:
                    if size >= q + 1:
                        bad[size] += 1
                break
    best, best_rpt = 1e300, rpt
    for size, weight in ((256, 1.0), (128, 1.6), (64, 2.6), (32, 4.5)):
        if size > rpt:
            continue
        f = float(bad[size]) / float(n_win)
        cost = (1.0 - f) * weight + 30.0 * f
        if cost < best - 1e-9:
            best, best_rpt = cost, size
    return best_rpt


def tile_cut(tid, pos, n_ops, rpt, in_order, slab_tiles, slab_layout):
    """First read of every tile, then the closing entries (n; twice for an empty upload)."""
    n = len(tid)
    firsts, start, pos_sum = [], 0, 0
    for i in range(n):
        need = (min(n_ops[i], LIMIT_31) + 3) >> 1 if slab_tiles else 0
        ends = i - start == rpt or (i > start and pos_sum + need > TILE_POS_CAP)
        if in_order and not ends:
            ends = tid[i] != tid[start] or (i > start and pos[i] - pos[start] >= TILE_SPAN and (slab_layout or i - start >= 8))
        if ends:
            firsts.append(start)
            start, pos_sum = i, 0
        pos_sum += need
    if n > start:
        firsts.append(start)
    return firsts + [n] * (2 if not firsts else 1)


def slab_layout_of(firsts, n_tiles, n_ops, wide_cigar, exb):
    """(slab_ok, sbase, slab_total, dense_rows)"""
    sbase, total, dense = [], 0, 0
    for t in range(n_tiles):
        rows = 1
        if wide_cigar:
            rows = SLAB_ROWS
        else:
            for i in range(firsts[t], firsts[t + 1]):
                dense += n_ops[i] + 1
                if (n_ops[i] + 3) >> 1 <= SLAB_ROWS:
                    rows = max(rows, (n_ops[i] + 3) >> 1)
        sbase.append(total)
        total += rows * SLAB_STRIDE
        if total >= LIMIT_31 or dense >= LIMIT_31:
            break
    if wide_cigar:
        dense = exb
    ok = total < LIMIT_31 and dense < LIMIT_31
    return ok, sbase + [total], total, dense


def tile_recs(firsts, n_tiles, sbase, tid, pos):
    """TileRec per tile as eight signed words: r0, n_act, sbase, rows, tid0, lo, last base (summaries only), 0."""
    rec = np.zeros((max(n_tiles, 1), 8), np.int64)
    for t in range(n_tiles):
        r0, n_act = firsts[t], firsts[t + 1] - firsts[t]
        rec[t, :6] = (r0, n_act, sbase[t], (sbase[t + 1] - sbase[t]) >> 8, tid[r0] if n_act else 0, (pos[r0] if n_act else 0) + 1)
    return rec


def summary_index(firsts, n_tiles, pos, summary):
    """(TileStat per tile, last base per tile, N operations per record) from the reader's three words per record."""
    stats, last, nn = [], [], []
    for t in range(n_tiles):
        rows = [(int(summary[i][0]), int(summary[i][1]) & 0xffff, int(summary[i][1]) >> 16, int(summary[i][2]) & 0xffff, int(summary[i][2]) >> 16, pos[i])
                for i in range(firsts[t], firsts[t + 1])]
        nn += [q[1] for q in rows]
        min_seg = min([INT32_MAX] + [q[4] for q in rows])
        if any(q[1] + 1 >= 255 for q in rows) or sum(q[1] + 1 for q in rows) >= SLOT_LOC_LIMIT:
            min_seg = INT32_MIN
        stats.append((sum(q[1] for q in rows), min([INT32_MAX] + [q[2] for q in rows]),
                      max([0] + [INT32_MAX if q[3] == 0xffff else q[3] for q in rows]), min_seg))
        last.append(min(max([INT32_MIN] + [q[5] + q[0] for q in rows]), INT32_MAX))
    return stats, last, nn


def sup_stats(stats, n_act):
    sup = [list(EMPTY_STAT) for _ in range((len(stats) >> SUP_SHIFT) + 1)]
    for t, st in enumerate(stats):
        q = sup[t >> SUP_SHIFT]
        q[0] += st[0] + n_act[t]
        q[1], q[2], q[3] = min(q[1], st[1]), max(q[2], st[2]), min(q[3], st[3])
    return sup


def upload_plan(tid, pos, cig_off, cig, summary=None, min_intron=3, max_delet=50, want_slab=True, want_index=True, stream_sorted=True,
                last_key=INT64_MIN, exb=None):
    tid, pos, cig_off, cig = [int(v) for v in tid], [int(v) for v in pos], [int(v) for v in cig_off], [int(v) for v in cig]
    n, n_cigar = len(tid), len(cig)
    p = {"sorted_here": check_reads(tid, pos, cig_off, n_cigar)}
    p["sorted"] = stream_sorted and (n == 0 or (p["sorted_here"] and read_key(tid[0], pos[0]) >= last_key))
    p["last_key"] = read_key(tid[-1], pos[-1]) if n else last_key
    p["wide_cigar"] = n > 0 and float(n_cigar) / float(n) > 32.0
    p["est"], p["many_exon_reads"] = exon_sample(cig_off, cig, n, min_intron, max_delet)
    slab_wanted = want_slab and p["sorted"]
    p["slab_tiles"] = slab_wanted and not p["wide_cigar"]
    p["slab_long"] = slab_wanted and p["wide_cigar"] and not p["many_exon_reads"]
    p["slab_layout"] = p["slab_tiles"] or p["slab_long"]
    p["make_index"] = want_index and not p["wide_cigar"]
    p["reads_per_tile"] = reads_per_tile(tid, pos, cig_off, cig, p["est"], p["sorted"], p["slab_long"], p["slab_layout"])
    n_ops = [cig_off[i + 1] - cig_off[i] for i in range(n)]
    firsts = tile_cut(tid, pos, n_ops, p["reads_per_tile"], p["sorted"], p["slab_tiles"], p["slab_layout"])
    p["tile_first"] = firsts
    p["n_tiles"] = n_tiles = len(firsts) - (2 if n == 0 else 1)
    p["n_tiles256"] = (n + TILE_READS - 1) // TILE_READS
    p["slab_ok"] = False
    if not p["slab_layout"]:
        return p
    p["slab_ok"], sbase, total, dense = slab_layout_of(firsts, n_tiles, n_ops, p["wide_cigar"], n_cigar + n if exb is None else exb)
    if not p["slab_ok"]:
        return p
    p["sbase"], p["slab_total"], p["dense_rows"] = sbase, total, dense
    rec = tile_recs(firsts, n_tiles, sbase, tid, pos)
    p["off32"] = [v & 0xffffffff for v in cig_off]
    p["have_index"] = n_tiles > 0 and p["make_index"]
    stats, nn = [EMPTY_STAT] * n_tiles, []
    if p["have_index"] and summary is not None:
        stats, last, nn = summary_index(firsts, n_tiles, pos, summary)
        rec[:n_tiles, 6] = last
    p["rec"], p["nn"], p["tile_stat"] = rec.reshape(-1), nn, [v for st in stats for v in st]
    p["sup_stat"] = [v for q in sup_stats(stats, rec[:n_tiles, 1]) for v in q]
    return p
