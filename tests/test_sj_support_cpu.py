"""CPU: the cases of tests/sj_support_cases.py before a GPU sees them.  For every case the literal restatement of the reference's junction
check (tests/sj_support_restatement.py), the oracle run with the table and the outcome the case states by hand agree, and the case reaches
what it is for (family A: the entry count, a pass, a fail, a read whose cursor row is the row in front; family C: one read per cell)."""
import pytest

from tests import sj_support_cases as sc
from tests import sj_support_restatement as rs
from tests import util
from tests.test_gpu_edges import _anno, _reads

CASES = sc.CASES


def test_the_list_is_complete():
    assert len(CASES) >= sc.N_ENUMERATED, (len(CASES), sc.N_ENUMERATED)
    fam = {c.family for c in CASES}
    assert fam == set("ABCDEFG"), fam
    a = {(c.meta["m"], c.meta["have_prev"]) for c in CASES if c.family == "A"}
    assert a == {(m, p) for m in sc.A_SIZES for p in (True, False)}
    assert {c.params["ss_dis"] for c in CASES if c.family == "C" and "cells" in c.meta} == set(sc.C_DIS)
    f = [c.name for c in CASES if c.family == "F"]
    for n_iso in (40, 70):
        for head in ("FA_m%d_" % sc.S, "FA_m%d_" % (sc.S + 1), "FB_", "FC_", "FE_"):
            assert any(n.startswith(head) and n.endswith("_iso%d" % n_iso) for n in f), (head, n_iso)
    for c in CASES:
        assert len(c.rows) <= 300 and all(r[1] < (1 << 17) for r in c.rows), c.name
        assert c.table == sorted(c.table), c.name


def evaluate(oracle, case):
    """(reads, restatement per read, oracle result with the table)"""
    af, reads = _anno(case.txs), _reads(case.rows)
    prm = {k: v for k, v in case.params.items()}
    base = util.oracle_run(oracle, af, reads, oracle.default_params(**prm))
    sj = tuple([r[k] for r in case.table] for k in range(5))
    want = util.oracle_run(oracle, af, reads, oracle.default_params(**prm), sj)
    mine = rs.junction_support(reads.tid, base, case.table, prm.get("ss_dis", 0), prm.get("min_sj_cnt", 1), prm.get("use_multi", 0))
    return reads, base, mine, want


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_restatement_oracle_and_hand_agree(oracle, case):
    reads, base, mine, want = evaluate(oracle, case)
    assert sorted(case.expect) == list(range(reads.n)), "every read has a stated outcome"
    for r in range(reads.n):                                 # a read is a candidate (full, not known, known site) unless the case says it is not checked
        assert ((int(base.info[r]) & 7) == 6) == (case.expect[r] != "not_checked"), (r, int(base.info[r]) & 7)
    outcomes = []
    for r in range(reads.n):
        bits, unrel, _row = mine[r]
        lo, hi = int(want.ex_off[r]), int(want.ex_off[r + 1])
        assert bits == int(want.info[r]) & 0x70, (r, bits, int(want.info[r]))
        assert unrel == [1 if f & rs.EXF_UNREL_JUNC else 0 for f in want.ex_flag[lo:hi].tolist()], r
        got = rs.outcome(bits, unrel)
        want_r = case.expect[r]
        assert got == (want_r if isinstance(want_r, str) else (want_r[0], list(want_r[1]))), (r, got, want_r)
        outcomes.append(got if isinstance(got, str) else got[0])
    # ---- reach
    if case.family == "A" or case.name.startswith("FA_"):
        m, have_prev = case.meta["m"], case.meta["have_prev"]
        assert sc.staged_entries(case.table, *case.meta["tile"]) == m
        tid, lo, last, dis = case.meta["tile"]
        for t, pos, _rev, ops in case.rows:                  # one span for every tile, however the reads are cut into tiles
            end = pos + sum(l for l, op in ops)
            assert t == tid and (pos + 1 - dis) >> 9 == (lo - dis) >> 9 and end == last
        # (a pass needs a supporting row inside the span: m = 1 is the row in front alone, and without that row no cursor row lies in
        #  front of a read's end either)
        assert "pass" in outcomes or m == 1
        assert "fail" in outcomes or (m == 1 and not have_prev)
        if have_prev:
            front = case.meta["front_row"]
            rows_used = [row for _b, _u, row in mine]
            assert front in rows_used and any(row is not None and row != front for row in rows_used) or m == 1 and front in rows_used
        # the count bits of the named entries decide a read: the entry is the row a read's last junction is looked up at, its bit differs
        # from both neighbours' (the successor's where the span has one)
        first = case.meta["front_row"] if have_prev else 0          # table index of staged entry 0
        for k in sc.BALLOT_ROWS:
            if k <= m - 1 and m > 3:
                row = case.table[first + k]
                ok = lambda q: q[3] >= case.params["min_sj_cnt"]
                deciders = [r for r in range(reads.n) if abs(_last_junction(want, r)[0] - row[1]) <= dis and abs(_last_junction(want, r)[1] - row[2]) <= dis]
                assert len(deciders) == 1, (k, row)
                assert ok(row) != ok(case.table[first + k - 1]), (k, row)
                if k < m - 1:
                    assert ok(row) != ok(case.table[first + k + 1]), (k, row)
                assert (outcomes[deciders[0]] == "pass") == ok(row), (k, row)
    if "cells" in case.meta:
        dis, cells = case.params["ss_dis"], case.meta["cells"]
        offs = case.meta["offsets"]
        assert sorted(cells) == sorted((dx, dy) for dx in offs for dy in offs) and sorted(cells.values()) == list(range(reads.n))
        j1 = case.table[0]
        for (dx, dy), r in cells.items():                      # the read's last junction has exactly one row near it: the cell's
            don, acc = _last_junction(want, r)
            near = [q for q in case.table if q != j1 and abs(q[1] - don) <= dis + 1 and abs(q[2] - acc) <= dis + 1]
            assert near == [(q[0], don + dx, acc + dy, q[3], q[4]) for q in near] and len(near) == 1, (dx, dy, near)
        assert "pass" in outcomes and "fail" in outcomes


def _last_junction(res, r):
    hi = int(res.ex_off[r + 1])
    return int(res.ex_end[hi - 2]) + 1, int(res.ex_start[hi - 1]) - 1


def test_the_cursor_only_moves_forward():
    """the restatement on a table by itself: a later read in front of an earlier one finds its rows behind the cursor"""
    table = [(0, 101, 199, 1, 0), (0, 1101, 1199, 1, 0)]

    class Base:
        ex_off = [0, 2, 4]
        ex_start, ex_end = [1000, 1200, 50, 200], [1100, 1300, 100, 300]
        ex_flag = [8, 0, 8, 0]
        info = [6, 6]
    got = rs.junction_support([0, 0], Base, table)
    assert [rs.outcome(b, u) for b, u, _ in got] == ["pass", "q7"]
    Base.ex_start, Base.ex_end = [50, 200, 1000, 1200], [100, 300, 1100, 1300]
    got = rs.junction_support([0, 0], Base, table)
    assert [rs.outcome(b, u) for b, u, _ in got] == ["pass", "pass"]
