"""Hand-built cases of `update-gtf -j` junction support (src/update_gtf.c:589-627, 698-709), as data.

The engine answers "is this novel junction supported" by searches where the reference scans from a sequential cursor (k_tile's staged
path and its table-in-HBM path in l2r_tile.hip.h, k_validate_sj / junction_supported / sj_first_row in l2r_kernels.hip.h).  The seeded
junction tables of the other tests hold rows that are a read's junction or unrelated to it; the tables here hold what those never do:
rows near a junction but not on it, two rows inside one tolerance, rows inside a short intron, rows in front of the tile that pin the
cursor, a cursor row at the read's end, 447 / 448 / 449 rows in a tile's span, buckets of 16 and 17 rows.

A case is Case(name, txs, rows, table, params, expect, family, meta):

    txs, rows   what test_gpu_edges._anno / _reads take
    table       [(tid, don, acc, uniq, multi)], sorted
    params      keyword arguments of default_params (split_trans is the test's)
    expect      {read index: "pass" | ("fail", [exon indices with the unreliable flag]) | "q7" | "not_checked"}, stated by the
                construction: q7 = checked, not passed, no exon flagged
    meta        what the case is for: m / have_prev (family A), cells (family C), front_row (the table row in front of the span)

tests/test_sj_support_cpu.py validates every case on the CPU (restatement == oracle == expect, and the case reaches what it is for);
tests/test_gpu_sj_support.py runs them on every route of the engine.

Every locus is one shape.  A transcript first exon / one pool exon / last exon; a read keeps the first exon (it may begin later) and
the last exon and carries novel exons between them: it is full at -l 3, has known sites, is not known -- a candidate -- and every one
of its junctions is novel.  With one middle exon (N0, n1) the junctions are J1 = (A1 + 1, N0 - 1), the same for every read, and
J2 = (n1 + 1, Z0 - 1): the donor is the read's own, the acceptor the same for every read.  Isoform-rich loci (family F) add isoforms
made of the first exon, pool exons and the last exon: the pool lies in front of N0, so no isoform has a read's junction.

-d -1: l2r_set_params takes it (it checks nothing; the engine then classifies with its generic kernel, and a junction lookup would scan
the table literally).  The case `D_dis_minus_1` pins what the reference gives: no site is within a negative tolerance, so no read has a
known site and none reaches the junction check.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name txs rows table params expect family meta")

SITE_SHIFT = 9                           # 512-bp buckets of the donor directory (l2r_kernels.hip.h)
SLAB_KEY_CAP = 168                       # l2r_slab.hip.h
SJ_STAGE = 2 * SLAB_KEY_CAP * 16 // 12   # l2r_tile.hip.h: junction rows k_tile stages per tile (448)
TILE_POS_CAP = 2400                      # l2r_slab.hip.h: exon positions of a tile
S = SJ_STAGE
M_OP, N_OP = 0, 3

A_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 1000)
C_DIS = (0, 1, 2, 7, 64)
BALLOT_ROWS = (31, 32, 63, 64, 255, 256, S - 1)      # staged entries whose count bit has to decide a read (family A)


def staged_entries(table, tid, tile_lo, tile_last, dis):
    """How many entries k_tile counts for a tile (l2r_tile.hip.h, the comment above rlo / rhi): the rows of the chromosome whose donor
    lies in the 512-bp buckets (tile_lo - dis) >> 9 .. (tile_last + dis) >> 9, plus one for the row in front."""
    b_lo, b_hi = max(tile_lo - max(dis, 0), 0) >> SITE_SHIFT, max(tile_last + max(dis, 0), 0) >> SITE_SHIFT
    return sum(1 for t, don, _a, _u, _m in table if t == tid and b_lo <= (max(don, 0) >> SITE_SHIFT) <= b_hi) + 1


def chain(exons):
    """(0-based position, CIGAR) of a read made of the given exons (1-based, closed); an exon may begin right behind its predecessor
    (an N of no length)."""
    ops = []
    for k, (s, e) in enumerate(exons):
        if k:
            ops.append((s - exons[k - 1][1] - 1, N_OP))
        ops.append((e - s + 1, M_OP))
    return exons[0][0] - 1, ops


class Locus:
    """first exon (A0, A1), twelve pool exons, novel exons from N0 on, last exon (Z0, Z1)."""

    def __init__(self, reach, lo_b=20, tid=1):
        self.tid = tid
        self.A0 = lo_b * 512 + 100
        self.A1 = self.A0 + 199
        self.pool = [(self.A1 + 60 + 100 * k, self.A1 + 99 + 100 * k) for k in range(12)]
        self.N0 = self.A1 + 1301
        self.Z0 = self.N0 + reach + 200
        self.Z1 = self.Z0 + 149
        self.J1 = (self.A1 + 1, self.N0 - 1)
        self.acc = self.Z0 - 1                                   # the acceptor of every read's last junction

    def txs(self, n_iso=1):
        out, seen = [(self.tid, 0, [(self.A0, self.A1), self.pool[3], (self.Z0, self.Z1)])], {(3,)}
        rng = np.random.default_rng(1000 + n_iso)
        while len(out) < n_iso:
            keep = tuple(sorted(int(k) for k in rng.choice(12, size=int(rng.integers(2, 9)), replace=False)))
            if keep not in seen:
                seen.add(keep)
                out.append((self.tid, len(out) & 1, [(self.A0, self.A1)] + [self.pool[k] for k in keep] + [(self.Z0, self.Z1)]))
        return out

    def read(self, s, *middle):
        """the read that begins s bases into the first exon and has the given middle exons"""
        return (self.tid, *chain([(self.A0 + s, self.A1)] + list(middle) + [(self.Z0, self.Z1)]))

    def read_to(self, s, n1):
        """... with one middle exon (N0, n1): J2 = (n1 + 1, Z0 - 1)"""
        return self.read(s, (self.N0, n1))

    def row(self, don, acc, uniq=1, multi=0):
        return (self.tid, don, acc, uniq, multi)


def _rows(reads):
    return [(t, p, 0, ops) for t, p, ops in reads]


def _case(name, family, txs, reads, table, params, expect, unsorted=False, **meta):
    rows = _rows(reads)
    if not unsorted:
        assert rows == sorted(rows, key=lambda r: (r[0], r[1])), name
    table = sorted(table)
    assert len(set(r[:3] for r in table)) == len(table), name           # (one row per junction, as a reduced table has)
    prm = dict(full_level=3)
    prm.update(params)
    return Case(name, txs, rows, table, prm, dict(expect), family, dict(meta, unsorted=unsorted))


# ---- A: rows in the tile's span ---------------------------------------------------------------------------------------------------

def case_a(m, have_prev, n_iso=1, prefix="A"):
    """m staged entries (the span's rows + 1) at -d 1 -J 2.  Entry 1 is J1's row; behind it, four bases apart, one donor per slot:
         hi      the read's junction with the count                                        -> pass
         low     the read's junction, one read short                                       -> fail
         pair    the junction one read short, then the same donor one base on with the count -> pass by the second row
         near    a row with the count two bases off the acceptor                           -> fail
         filler  a row between two reads' donors, with the count, on nobody's junction
    laid so that the count bits of entries 31 (second of a pair), 32 (low, between two rows with the count), 63, 64, 255, 256, S - 1
    each decide a read.  Every read begins in one 512-bp bucket and ends at one base, so every tile of the case has the same span
    however the engine cuts the tiles."""
    dis, J = 1, 2
    n = m - 1
    L = Locus(4 * (n + 6))
    D0 = L.N0 + 50
    span, reads, expect = [], [], {}
    front = L.row((20 - 3) * 512 + 7, L.A0 + 35, J) if have_prev else (L.tid - 1, 500, 900, J, 0)
    behind = L.row(((L.Z1 + dis) >> SITE_SHIFT) * 512 + 3 * 512 + 5, L.Z1 + 3000, J)

    def add(read, what):
        expect[len(reads)] = what
        reads.append(read)

    if n == 0:
        # no row in the span: the row in front (acceptor at A0 + 35) is the cursor row of the reads that begin in front of that base --
        # their junctions find nothing --, the others' cursor row lies behind them.  Nothing can pass: a pass needs a row in the span.
        for s in (0, 20, 34, 35, 50):
            add(L.read_to(s, D0 - 1), ("fail", [0, 1]) if have_prev and s < 35 else "q7")
    elif n == 1:
        # one row: a read whose only junction it is passes, a read with two junctions has neither supported
        span.append(L.row(L.A1 + 1, L.acc, J))
        for s in (0, 40):
            add(L.read(s), "pass")
            add(L.read_to(s, D0 - 1), ("fail", [0, 1]))
    else:
        span.append(L.row(*L.J1, J))
        hi_at, lo_at = {31, 63, 255, S - 1}, {32, 64, 256}
        cycle = ("hi", "filler", "low", "pair", "filler", "near", "hi", "filler")
        slot = 0
        todo = []                                                           # (donor, outcome) in donor order
        while len(span) < n:
            nxt, left, d = len(span) + 1, n - len(span), D0 + 4 * slot
            if left >= 2 and nxt + 1 in hi_at:
                kind = "pair"
            elif nxt in lo_at:
                kind = "low"
            elif nxt in hi_at or nxt - 1 in lo_at or nxt + 1 in lo_at:
                kind = "hi"
            elif nxt + 2 in hi_at:
                kind = "filler"
            else:
                kind = cycle[slot % len(cycle)] if len(todo) < 270 else "filler"
                if kind == "pair" and (left < 2 or nxt + 1 in lo_at or nxt + 2 in hi_at):
                    kind = "hi"
            slot += 1
            if kind == "hi":
                span.append(L.row(d, L.acc, J)); todo.append((d, "pass"))
            elif kind == "low":
                span.append(L.row(d, L.acc, J - 1, 5)); todo.append((d, ("fail", [1])))
            elif kind == "pair":
                span += [L.row(d, L.acc, J - 1), L.row(d, L.acc + 1, J)]; todo.append((d, "pass"))
            elif kind == "near":
                span.append(L.row(d, L.acc - 2, J)); todo.append((d, ("fail", [1])))
            else:
                span.append(L.row(d + 2, L.acc - 40 - slot % 5, J))
        for i, (d, what) in enumerate(todo):                                # (starts 0 .. 67: both sides of the front row's acceptor)
            add(L.read_to(i * 68 // len(todo), d - 1), what)
    table = [front] + span + [behind]
    got_m = staged_entries(table, L.tid, L.A0, L.Z1, dis)
    assert got_m == m, (m, got_m)
    assert (L.A0 - dis) >> SITE_SHIFT == (L.A0 + 70 - dis) >> SITE_SHIFT
    return _case("%s_m%d_%s%s" % (prefix, m, "prev" if have_prev else "noprev", "" if n_iso == 1 else "_iso%d" % n_iso), prefix[0],
                 L.txs(n_iso), reads, table, dict(ss_dis=dis, min_sj_cnt=J), expect, m=m, have_prev=have_prev,
                 front_row=sorted(table).index(front) if have_prev else None, tile=(L.tid, L.A0, L.Z1, dis))


# ---- B: cursor row and Q7 -------------------------------------------------------------------------------------------------------------

def cases_b(n_iso=1, prefix="B"):
    out = []
    L = Locus(600)
    n1 = L.N0 + 100
    j2 = (n1 + 1, L.acc)
    e = L.Z1
    sup = [L.row(*L.J1), L.row(*j2)]
    far = L.row(e + 5000, e + 6000)

    def mk(name, reads, table, expect, locus=L):
        out.append(_case("%s_%s%s" % (prefix, name, "" if n_iso == 1 else "_iso%d" % n_iso), prefix[0], locus.txs(n_iso), reads, table,
                         dict(ss_dis=0, min_sj_cnt=1), expect))

    # a row whose acceptor is the read's first base is in front of it (:613 `acc <= start`), one base further it is the cursor row
    mk("acc_eq_start", [L.read_to(10, n1), L.read_to(11, n1)], [L.row(L.A0 - 300, L.A0 + 11), far], {0: ("fail", [0, 1]), 1: "q7"})
    mk("acc_eq_start_supported", [L.read_to(10, n1), L.read_to(11, n1)], [L.row(L.A0 - 300, L.A0 + 11), far] + sup, {0: "pass", 1: "pass"})
    # the cursor row's donor against the read's last base (:615 `don >= end`)
    for k, what in ((-1, ("fail", [0, 1])), (0, "q7"), (1, "q7")):
        mk("cursor_don_end%+d" % k, [L.read_to(5, n1)], [L.row(e + k, e + 400)], {0: what})
    mk("all_rows_in_front", [L.read_to(5, n1)], [L.row(L.A0 - 400, L.A0 - 300), L.row(L.A0 - 200, L.A0 + 2), L.row(L.A0 - 50, L.A0 + 5)], {0: "q7"})
    mk("earlier_chromosome_only", [L.read_to(5, n1)], [(0,) + r[1:] for r in sup], {0: "q7"})
    mk("later_chromosome_only", [L.read_to(5, n1)], [(2,) + r[1:] for r in sup], {0: "q7"})
    L3 = Locus(600, tid=2)
    mk("reads_behind_the_last_table_chromosome", [L3.read_to(5, n1)], [(0,) + r[1:] for r in sup] + sup, {0: "q7"}, locus=L3)
    mk("rows_without_chromosome_first", [L.read_to(5, n1), L.read_to(6, n1 + 40)], [(-1, 100, 200, 1, 0), (-1,) + sup[0][1:]] + sup,
       {0: "pass", 1: ("fail", [1])})
    # one row far in front of the tile with its acceptor behind it: the cursor row of every read
    long_row = L.row(L.A0 - 6000, e + 6000, 0, 0)
    mk("long_row_in_front", [L.read_to(5, n1), L.read_to(6, n1 + 40)], [long_row] + sup, {0: "pass", 1: ("fail", [1])})
    mk("long_row_in_front_alone", [L.read_to(5, n1)], [long_row], {0: ("fail", [0, 1])})
    # the span's only row lies in front of the read, the cursor row behind every staged row
    mk("cursor_behind_the_staged_rows", [L.read_to(5, n1)], [L.row(L.A0 - 50, L.A0 + 3), L.row((e >> SITE_SHIFT) * 512 + 4 * 512, e + 9000)], {0: "q7"})
    return out


# ---- C: tolerance -----------------------------------------------------------------------------------------------------------------

def _offsets(dis):
    return sorted({-dis - 1, -dis, 0, dis, dis + 1})


def case_c_cells(dis, n_iso=1, prefix="C"):
    """one read per (donor offset, acceptor offset): its last junction's only row lies that far off"""
    offs = _offsets(dis)
    step = 2 * dis + 6
    L = Locus(100 + step * len(offs) ** 2 + 2 * dis)
    reads, table, expect, cells = [], [L.row(*L.J1)], {}, {}
    for c, (dx, dy) in enumerate((dx, dy) for dx in offs for dy in offs):
        d = L.N0 + 100 + c * step
        cells[(dx, dy)] = c
        reads.append(L.read_to(c // 4, d - 1))
        table.append(L.row(d + dx, L.acc + dy))
        expect[c] = "pass" if abs(dx) <= dis and abs(dy) <= dis else ("fail", [1])
    return _case("%s_cells_d%d%s" % (prefix, dis, "" if n_iso == 1 else "_iso%d" % n_iso), prefix[0], L.txs(n_iso), reads, table,
                 dict(ss_dis=dis, min_sj_cnt=1), expect, cells=cells, offsets=offs)


def cases_c_rest():
    out = []
    # two rows inside one junction's tolerance, the count on the later one; uniq short and uniq + multi reaching -J
    for multi in (0, 1):
        L = Locus(400)
        d = [L.N0 + 100 + 20 * k for k in range(3)]
        table = [L.row(*L.J1, 3), L.row(d[0], L.acc, 2, 0), L.row(d[0] + 1, L.acc, 3, 0), L.row(d[1], L.acc, 2, 1),
                 L.row(d[2], L.acc, 2, 0), L.row(d[2] + 1, L.acc, 1, 2)]
        out.append(_case("C_two_rows_multi%d" % multi, "C", L.txs(), [L.read_to(k, d[k] - 1) for k in range(3)], table,
                         dict(ss_dis=2, min_sj_cnt=3, use_multi=multi), {0: "pass", 1: "pass" if multi else ("fail", [1]), 2: "pass" if multi else ("fail", [1])}))
    # an intron of 3 bases at -d 7 -i 1: a row inside the tolerance whose donor is at the junction's acceptor ends the reference's scan
    # (:594 `don >= end`) -- unsupported; with a matching row in front of that one the scan never gets there
    L = Locus(900)
    xa, xb = L.N0 + 100, L.N0 + 400
    reads = [L.read(0, (L.N0, xa), (xa + 4, xa + 60)), L.read(1, (L.N0, xb), (xb + 4, xb + 60))]
    table = [L.row(*L.J1), L.row(xa + 3, xa + 3), L.row(xa + 61, L.acc), L.row(xb + 2, xb + 3), L.row(xb + 3, xb + 3), L.row(xb + 61, L.acc)]
    out.append(_case("C_short_intron", "C", L.txs(), reads, table, dict(ss_dis=7, min_sj_cnt=1, min_intron=1), {0: ("fail", [1]), 1: "pass"}))
    # donors at 511, 512, 513 modulo 512 at -d 2.  Residues 512 and 513: the lower bound don - dis (510, 511) lies in the bucket in front of
    # the donor's, so the row at don - 2 is the last row of that bucket.  Residue 511: don - dis (509) is in the donor's own bucket and
    # don + dis (513) in the one behind, so the row at don + 2 is found by walking over the bucket's end.  Each residue with a row at
    # -2, at +2 and at -3 (outside).
    L = Locus(16 * 512)
    reads, table, expect = [], [L.row(*L.J1)], {}
    b0 = (L.N0 >> SITE_SHIFT) + 1
    for i, (res, off) in enumerate((res, off) for res in (511, 512, 513) for off in (-2, 2, -3)):
        d = (b0 + i) * 512 + res
        reads.append(L.read_to(i, d - 1))
        table.append(L.row(d + off, L.acc))
        expect[i] = "pass" if abs(off) <= 2 else ("fail", [1])
    out.append(_case("C_bucket_edges", "C", L.txs(), reads, table, dict(ss_dis=2, min_sj_cnt=1), expect))
    # buckets of exactly 16 and 17 rows (sj_first_row walks up to 16 rows and searches beyond), the matching row first, last, absent
    L = Locus(16 * 512)
    reads, table, expect, buckets = [], [L.row(*L.J1)], {}, {}
    for i, (size, where) in enumerate((size, where) for size in (16, 17) for where in ("first", "last", "absent")):
        b = b0 + 2 * i
        d = b * 512 + 200
        reads.append(L.read_to(i, d - 1))
        others = size - (where != "absent")
        if where == "first":
            rows = [L.row(d, L.acc)] + [L.row(d, L.acc + 3 + k) if k % 2 else L.row(d + 5 + k, L.acc) for k in range(others)]
        elif where == "last":
            rows = [L.row(d, L.acc - 3 - k) if k % 2 else L.row(d - 5 - k, L.acc) for k in range(others)] + [L.row(d, L.acc)]
        else:
            rows = [L.row(d, L.acc - 3 - k) if k % 2 else L.row(d - 5 - k, L.acc) for k in range(others // 2)]
            rows += [L.row(d, L.acc + 3 + k) if k % 2 else L.row(d + 5 + k, L.acc) for k in range(others - others // 2)]
        assert len(rows) == size and all(r[1] >> SITE_SHIFT == b for r in rows)
        table += rows
        buckets[b] = size
        expect[i] = ("fail", [1]) if where == "absent" else "pass"
    out.append(_case("C_buckets_of_16_and_17", "C", L.txs(), reads, table, dict(ss_dis=0, min_sj_cnt=1), expect, buckets=buckets))
    return out


# ---- D: the literal-scan conditions ---------------------------------------------------------------------------------------------------

def cases_d():
    out = []
    # -i 0 and an N of no length: the junction's acceptor lies one base in front of its donor.  A row on the junction itself has its donor
    # behind the acceptor and ends the scan; at -d 2 a row two bases in front of the donor is inside the tolerance and in front of the acceptor.
    L = Locus(900)
    xa, xb = L.N0 + 100, L.N0 + 400
    reads = [L.read(0, (L.N0, xa), (xa + 1, xa + 60)), L.read(1, (L.N0, xb), (xb + 1, xb + 60))]
    table = [L.row(*L.J1), L.row(xa - 1, xa), L.row(xa + 61, L.acc), L.row(xb + 1, xb), L.row(xb + 61, L.acc)]
    out.append(_case("D_zero_length_intron", "D", L.txs(), reads, table, dict(ss_dis=2, min_sj_cnt=1, min_intron=0), {0: "pass", 1: ("fail", [1])}))
    # -d -1: no annotation site is within the tolerance of a read's, so no read has a known site: none reaches the junction check
    L = Locus(400)
    d = L.N0 + 100
    out.append(_case("D_dis_minus_1", "D", L.txs(), [L.read_to(0, d - 1), L.read_to(1, d + 19)], [L.row(*L.J1), L.row(d, L.acc)],
                     dict(ss_dis=-1, min_sj_cnt=1), {0: "not_checked", 1: "not_checked"}))
    return out


# ---- E: junctions behind exon 64 ------------------------------------------------------------------------------------------------------

def case_e(n_iso=1, prefix="E", copies=1):
    """A transcript of 100 exons and 20 reads of 99: each skips exon 62, 63, 64, 65 or 98 and ends the exon in front of the gap 3, 6, 9 or
    12 bases early (a donor of its own): one novel junction, at the read's exon 61, 62, 63 (the last one k_tile keeps as a bit), 64 (the
    first one of its tail loop) or 97.  -J 2 with --use-multi: 3 -> a row with two unique reads, 9 -> one unique and one multi read (pass);
    6 -> no row, 12 -> a row with one read (fail).

    An upload of such reads alone has 197 CIGAR operations per read: beyond 32 on average the upload plan (l2r_plan.hip.h, wide_cigar)
    makes no tile index and the engine takes its classic kernels whatever pipeline is asked for -- k_tile would never see the reads.  So
    140 reads of three consecutive inner exons (5 operations; not full at -l 3: not checked) follow the long ones in the same upload:
    29 operations per read on average, 160 reads, and the first tile -- the 20 long reads and the first 100 short ones, cut by the plan
    at TILE_POS_CAP -- has 2280 exons.  copies = 4 has no short reads and is for the classic kernels: 80 reads, 7920 exons -- more than
    the SJ_MAP_CAP = 6144 positions k_validate_sj maps for a block of 256 reads (l2r_kernels.hip.h): the reads behind them take its
    per-read loop.

    Isoform-rich loci: 40 isoforms that skip one to three exons each (one junction of their own per isoform: 100 START and 138 END
    entries, inside what k_tile's WIDE instance stages); 70 isoforms of the first exon, four consecutive inner exons and the last exon
    around the whole transcript in the middle of the file order (no inner key has members 64 apart: 102 START entries, below
    k_tile_chunk's TC_ST_CAP = 128)."""
    tid, base = 1, 20 * 512 + 100
    ex = [(base + 200 * k, base + 200 * k + 59) for k in range(100)]
    if n_iso <= 63:
        txs = [(tid, 0, list(ex))]
        for t in range(1, n_iso):
            a = 2 + t
            txs.append((tid, t & 1, ex[:a + 1] + ex[a + 2 + t % 3:]))
    else:
        txs = [(tid, t & 1, [ex[0]] + ex[1 + t:5 + t] + [ex[99]]) for t in range(1, n_iso)]
        txs.insert(n_iso // 2, (tid, 0, list(ex)))
    reads, table, expect = [], [], {}
    for i, (v, skip) in enumerate((v, skip) for _ in range(copies) for v in (3, 6, 9, 12) for skip in (62, 63, 64, 65, 98)):
        c = list(ex)
        c[skip - 1] = (c[skip - 1][0], c[skip - 1][1] - v)
        del c[skip]
        c[0] = (c[0][0] + i // copies, c[0][1])
        reads.append((tid, *chain(c)))
        don, acc = ex[skip - 1][1] - v + 1, ex[skip + 1][0] - 1
        if v != 6 and i < 20:
            table.append((tid, don, acc) + {3: (2, 0), 9: (1, 1), 12: (1, 0)}[v])
        expect[i] = "pass" if v in (3, 9) else ("fail", [skip - 1])
    if copies == 1:
        for j in range(140):
            k = 1 + j * 96 // 140
            expect[len(reads)] = "not_checked"
            reads.append((tid, *chain(ex[k:k + 3])))
        n_ops = sum(len(r[2]) for r in reads)
        assert n_ops <= 32 * len(reads)                                  # (the upload keeps its tile index)
        assert 20 * 99 + 100 * 3 <= TILE_POS_CAP
    return _case("%s_behind_exon_64%s%s" % (prefix, "" if n_iso == 1 else "_iso%d" % n_iso, "" if copies == 1 else "_x%d" % copies), prefix[0], txs, reads, table,
                 dict(ss_dis=0, min_sj_cnt=2, use_multi=1), expect, long_reads=20 * copies)


# ---- G: the cursor never goes back ----------------------------------------------------------------------------------------------------

def cases_g():
    """Unsorted input: read 0 and read 2 at a locus 40 buckets behind read 1's.  Read 0 moves the cursor over the rows of read 1's
    junctions (their acceptors lie in front of read 0): read 1's cursor row is then the first row of the later locus, behind it -- q7.
    With a row that begins inside read 1's last exon and ends behind read 0's first base the cursor stops there instead: read 1's
    junctions are looked up from a row whose donor lies behind their acceptors -- both unsupported."""
    out = []
    La, Lb = Locus(600), Locus(600, lo_b=60)
    na, nb = La.N0 + 100, Lb.N0 + 100
    # (the annotation cursor moves forward too: the earlier locus's transcript reaches behind the later locus, so read 1 still meets it;
    #  its last exon is then an inner exon of the transcript, so the reads are full at -l 5 only)
    ta = La.txs()[0]
    txs = [(ta[0], ta[1], ta[2] + [(Lb.Z1 + 1000, Lb.Z1 + 1100)])] + Lb.txs()
    reads = [Lb.read_to(5, nb), La.read_to(5, na), Lb.read_to(6, nb)]
    sup = [La.row(*La.J1), La.row(na + 1, La.acc), Lb.row(*Lb.J1), Lb.row(nb + 1, Lb.acc)]
    out.append(_case("G_cursor_past_the_earlier_locus", "G", txs, reads, sup, dict(ss_dis=0, min_sj_cnt=1, full_level=5), {0: "pass", 1: "q7", 2: "pass"}, unsorted=True))
    out.append(_case("G_cursor_on_a_row_inside_the_earlier_read", "G", txs, reads, sup + [La.row(La.Z1 - 10, Lb.A0 + 500, 0, 0)],
                     dict(ss_dis=0, min_sj_cnt=1, full_level=5), {0: "pass", 1: ("fail", [0, 1]), 2: "pass"}, unsorted=True))
    return out


# ---- the list -------------------------------------------------------------------------------------------------------------------------

def build_cases():
    out = [case_a(m, prev) for m in A_SIZES for prev in (True, False)]
    out += cases_b()
    out += [case_c_cells(dis) for dis in C_DIS]
    out += cases_c_rest()
    out += cases_d()
    out += [case_e(), case_e(copies=4)]
    for n_iso in (40, 70):                                  # F: k_tile's WIDE instance; k_tile_chunk, then k_validate_sj
        out += [case_a(S, True, n_iso, "FA"), case_a(S + 1, True, n_iso, "FA")]
        out += [c for c in cases_b(n_iso, "FB") if "long_row_in_front_iso" in c.name or "acc_eq_start_iso" in c.name]
        out += [case_c_cells(7, n_iso, "FC"), case_e(n_iso, "FE")]
    out += cases_g()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# what the families enumerate: A 12 sizes x 2; B 13; C 5 tolerances + 5; D 2; E 1; F 2 loci x (2 + 2 + 1 + 1); G 2
N_ENUMERATED = len(A_SIZES) * 2 + 13 + len(C_DIS) + 5 + 2 + 1 + 2 * 6 + 2
CASES = build_cases()
