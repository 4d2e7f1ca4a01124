"""k_tile places a tile's exons with one of two walks (l2r_tile.hip.h): an EXACT tile -- no threshold is borderline in it (tile_exact,
l2r_slab.hip.h) -- takes the walk that knows "a cut is an N operation, every cut keeps"; any other tile, and every tile under
L2R_ABLATE bit 8, takes the general walk.  Both must give what the oracle gives.

The workload has two chromosomes (a tile never spans two, so the mix of tiles does not depend on where the engine cuts them):
chromosome 0 holds no borderline operation at all, on chromosome 1 at least every 20th read and the last one carry one (a D longer than
-t, an N shorter than -i, or an inner exon shorter than -e), so every tile of up to 256 consecutive reads there is inexact.  Both hold
single-exon reads, reads whose first or last exon is shorter than -e, and one read of more than 24 operations among short ones."""
import numpy as np
import pytest

from lr2rmats_amd import capi, synth

MIN_EXON, MIN_INTRON, MAX_DELET = 3, 3, 50          # the defaults (-e, -i, -t)
M, I, D, N = synth.CIG_M, synth.CIG_I, synth.CIG_D, synth.CIG_N
EVERY = 20


def _op(length, op):
    return (int(length) << 4) | op


def _chain_ops(ex):
    """M N M N ... M of an exon chain [(start, end), ...] (1-based, closed)."""
    ops = []
    for k, (s, e) in enumerate(ex):
        if k:
            ops.append(_op(s - ex[k - 1][1] - 1, N))
        ops.append(_op(e - s + 1, M))
    return ops


def _borderline(ops, kind):
    """The read's operations with one borderline stretch behind its first M."""
    extra = {0: [_op(MAX_DELET + 10, D), _op(5, M)],                                   # a D that cuts
             1: [_op(MIN_INTRON - 1, N), _op(7, M)],                                   # an N that is no intron
             2: [_op(200, N), _op(MIN_EXON - 1, M), _op(200, N), _op(30, M)]}[kind]      # an inner exon that is dropped
    return ops[:1] + extra + ops[1:]


def _read_stats(ops):
    """tile_exact's three statistics for one read: its shortest N, its longest D, the shortest stretch of reference bases between two N."""
    min_n, max_d, min_seg = 1 << 30, 0, 1 << 30
    seg, seen_n = 0, False
    for c in ops:
        op, ln = c & 15, c >> 4
        if op == N:
            min_n = min(min_n, ln)
            if seen_n:
                min_seg = min(min_seg, seg)
            seen_n, seg = True, 0
        else:
            if op == D:
                max_d = max(max_d, ln)
            if op in (0, 2, 3, 7, 8):
                seg += ln
    return min_n, max_d, min_seg


def _is_borderline(ops):
    min_n, max_d, min_seg = _read_stats(ops)
    return not (min_n >= MIN_INTRON and max_d <= MAX_DELET and min_seg >= MIN_EXON)


def _workload():
    rng = np.random.default_rng(7007)
    anno = synth.make_annotation(300, 11, nchr=2)              # six genes, three per chromosome: a tile's reads begin close together
    af = anno.in_file_order()
    rows = []                                                  # (tid, pos, rev, exon chain, shape)
    for i in range(5000):
        t = int(rng.integers(af.n_tx))
        a, b = int(af.tx_ex_off[t]), int(af.tx_ex_off[t + 1])
        ex = [(int(af.ex_start[k]), int(af.ex_end[k])) for k in range(a, b)]
        lo = int(rng.integers(0, len(ex)))
        ex = ex[lo:lo + int(rng.integers(1, 9))]
        shape = i % 11
        if shape == 0:
            ex = ex[:1]                                        # single exon
        elif shape == 1 and len(ex) > 1:
            ex[0] = (ex[0][1] - (MIN_EXON - 2), ex[0][1])      # first exon shorter than -e: kept whatever its length
        elif shape == 2 and len(ex) > 1:
            ex[-1] = (ex[-1][0], ex[-1][0] + (MIN_EXON - 2))   # ... and the last one
        rows.append((int(af.tx_tid[t]), ex[0][0] - 1, int(af.tx_rev[t]), ex, shape))
    rows.sort(key=lambda r: (r[0], r[1]))
    n_a = sum(1 for r in rows if r[0] == 0)
    tid, pos, rev, cig, off = [], [], [], [], [0]
    long_at = {n_a // 2, n_a + (len(rows) - n_a) // 2 + 3}     # one long read per chromosome (not a borderline one)
    for i, (t, p, rv, ex, shape) in enumerate(rows):
        ops = _chain_ops(ex)
        if shape == 3:                                         # short indels well clear of -t
            ops = [_op((ops[0] >> 4) - 20, M), _op(4, D), _op(10, M), _op(2, I), _op(6, M)] + ops[1:]
        if i in long_at:                                       # more than 24 operations: its tail is walked from memory
            head = []
            for _ in range(14):
                head += [_op(3, M), _op(1, I), _op(2, D)]
            ops = head + ops                                   # (its first exon grows by the head's 70 bases)
        j = i - n_a
        if t == 1 and i not in long_at and (j % EVERY == 0 or i == len(rows) - 1):
            ops = _borderline(ops, (j // EVERY) % 3)
        tid.append(t); pos.append(p); rev.append(rv); cig += ops; off.append(len(cig))
    reads = synth.Reads(af.chrom_names, np.array(tid, np.int32), np.array(pos, np.int32), np.array(rev, np.uint8),
                        np.array(rev, np.uint8), np.zeros(len(tid), np.uint8), np.array(off, np.int64), np.array(cig, np.uint32))
    return af, reads, n_a


def _classify(af, reads):
    eng = capi.Engine(0)
    try:
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_params(capi.default_params(full_level=3, min_exon=MIN_EXON, min_intron=MIN_INTRON, max_delet=MAX_DELET))
        eng.set_outputs(1)
        eng.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
        eng.run(); eng.sync()
        return eng.download(), (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()
    finally:
        eng.close()


@pytest.mark.gpu
def test_exact_walk_general_walk_and_oracle_agree(monkeypatch):
    from oracle import pyoracle as po
    af, reads, n_a = _workload()
    # what the test rests on: chromosome 0 has no borderline read, every stretch of chromosome 1 that can be a tile has one
    ops_of = lambda i: [int(c) for c in reads.cig[int(reads.cig_off[i]):int(reads.cig_off[i + 1])]]
    bl = np.array([_is_borderline(ops_of(i)) for i in range(reads.n)])
    assert n_a > 1000 and reads.n - n_a > 1000
    assert (reads.tid[:n_a] == 0).all() and (reads.tid[n_a:] == 1).all()
    assert not bl[:n_a].any()
    at = np.nonzero(bl[n_a:])[0]
    assert at[0] == 0 and at[-1] == reads.n - n_a - 1 and np.diff(at).max() <= 50
    n_ops = np.diff(reads.cig_off)
    for lo, hi in ((0, n_a), (n_a, reads.n)):
        assert (n_ops[lo:hi] == 1).any() and (n_ops[lo:hi] > 24).sum() == 1
        first_m = reads.cig[reads.cig_off[lo:hi]] >> 4
        assert ((first_m < MIN_EXON) & (n_ops[lo:hi] > 1)).any()
        last_m = reads.cig[reads.cig_off[lo + 1:hi + 1] - 1] >> 4
        assert ((last_m < MIN_EXON) & (n_ops[lo:hi] > 1)).any()

    monkeypatch.setenv("L2R_PIPELINE", "tile")
    monkeypatch.delenv("L2R_ABLATE", raising=False)
    got, kernel = _classify(af, reads)
    assert kernel.startswith("k_tile"), kernel
    monkeypatch.setenv("L2R_ABLATE", "256")                    # every tile counts and takes the general walk
    gen, kernel_g = _classify(af, reads)
    assert kernel_g.startswith("k_tile"), kernel_g
    want = po.classify_soa(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig, af.tx_tid, af.tx_start, af.tx_end, af.tx_rev,
                           af.tx_ex_off, af.ex_start, af.ex_end,
                           params=po.default_params(full_level=3, min_exon=MIN_EXON, min_intron=MIN_INTRON, max_delet=MAX_DELET))
    for name, res in (("exact walk", got), ("general walk", gen)):
        assert np.array_equal(res.ex_off, want.ex_off), name
        assert np.array_equal(res.ex_start, want.ex_start), name
        assert np.array_equal(res.ex_end, want.ex_end), name
        assert np.array_equal(res.ex_flag, want.ex_flag), name
        assert np.array_equal(res.info & 0x7f, want.info & 0x7f), name
        assert np.array_equal(res.ref_tx, want.ref_tx), name
    for f in ("ex_off", "ex_start", "ex_end", "ex_flag", "info", "ref_tx"):
        assert np.array_equal(getattr(got, f), getattr(gen, f)), f
