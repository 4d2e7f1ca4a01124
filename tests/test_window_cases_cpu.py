"""CPU: the cases of tests/window_cases.py before a GPU sees them.  For every case the model of the tile descriptor (window_cases.describe)
says that the locus sits where the case claims -- the window's size, the START / END slices, the bucket count, the transcript that ends
the window scan, the exons of a tile -- and the oracle's result has what the case relies on: reads that are known through the edge member
alone, through the first and the last entry of a slice, in the last bucket; and reads of all three classes (known, known sites only,
neither).  A later change to a builder cannot move a case off its cap without failing here."""
import numpy as np
import pytest

from tests import util
from tests import window_cases as wc
from tests.test_gpu_edges import _anno, _reads


def _oracle(oracle, case, **kw):
    prm = dict(full_level=3, **case.params)
    prm.update(kw)
    return util.oracle_run(oracle, _anno(case.txs), _reads(case.rows), oracle.default_params(**prm))


def _classes(want, rows=None):
    info = want.info if rows is None else want.info[rows]
    known = (info & 1) != 0
    return known, ((info & 2) != 0) & ~known, (info & 3) == 0


def _all_three(want):
    known, site, neither = _classes(want)
    assert known.sum() >= 20 and site.sum() >= 20 and neither.sum() >= 20, (known.sum(), site.sum(), neither.sum())


def _full_and_not(want):
    """(-l 3: some reads have the full-length evidence, some do not)"""
    full = (want.info & 4) != 0
    assert full.sum() >= 20 and (~full).sum() >= 20, (full.sum(), (~full).sum())


def _one_descriptor(case, **kw):
    """The case's promise: every tile has the same window and the same slices.  Returns the tiles."""
    tiles = wc.describe(case.txs, case.rows, dis=case.params.get("ss_dis", 0), **kw)
    assert len(tiles) >= 4 and tiles[-1].last - tiles[-1].first < 256 and 700 <= len(case.rows) <= 900, len(tiles)
    t0 = tiles[0]
    for t in tiles:
        assert (t.cursor, t.members, t.scanned) == (t0.cursor, t0.members, t0.scanned)
        assert (t.tlo >> 9, t.thi >> 9) == (wc.LO_B, wc.HI_B)
        if not case.params.get("ss_dis"):
            assert (t.nbk, t.st, t.en) == (t0.nbk, t0.st, t0.en)
    return tiles


def _single_part_keys(case):
    dic = wc.Dictionaries(case.txs)
    assert len(dic.st) == len(set(dic.st)) and len(dic.en) == len(set(dic.en))        # word 1 of l2r_debug_counters is 0
    return dic


def _shape(case):
    """short CIGARs in coordinate order: the slab and the tile pipeline take the reads"""
    assert [r[:2] for r in case.rows] == sorted(r[:2] for r in case.rows)
    assert sum(len(r[3]) for r in case.rows) <= 32 * len(case.rows)
    assert {r[2] for r in case.rows} == {0, 1} and len(case.txs) < 4200


@pytest.mark.parametrize("name", wc.names("window") + wc.names("dis"))
def test_window_size(oracle, name):
    case = wc.case("dis" if name.startswith("dis_") else "window", name)
    m = case.meta
    _shape(case)
    tiles = _one_descriptor(case)
    members = tiles[0].members
    assert len(members) == m["n_win"] and tiles[0].scanned is not None
    assert (members[-1] - members[0] + 1 == len(members)) == (not m["gapped"])       # TD_CONTIG
    _single_part_keys(case)
    for t in tiles:
        assert len(t.st) <= wc.SLAB_KEY_CAP and len(t.en) <= wc.SLAB_KEY_CAP and t.nbk <= wc.DIR_CAP
    want = _oracle(oracle, case)
    _all_three(want)
    if m["n_iso"]:
        _full_and_not(want)
    kinds, last = m["kinds"], members[-1]
    n_ex = np.diff(want.ex_off)
    if case.family == "dis":
        return
    if m["shorts"] == 0:
        k1, k2 = np.array(kinds[1]), np.array(sorted(set(kinds[2]) - set(m.get("between", ()))))
        assert ((want.info[k1] & 1) != 0).all() and (want.ref_tx[k1] == members[0]).all()
        if m["edge"] != "single":                                  # the last member's chain: known through it and nobody else
            assert ((want.info[k2] & 1) != 0).all() and (want.ref_tx[k2] == last).all()
        assert ((want.info & 1) != 0)[want.ref_tx == last].sum() >= 50
    if m["edge"] == "single":                                      # reads of one exon over it on both sides of single_exon_ovlp_frac
        k6 = np.array(kinds[6])
        hit = ((want.info[k6] & 1) != 0) & (want.ref_tx[k6] == last)
        assert len(case.txs[last][2]) == 1 and (n_ex[k6] == 1).all() and hit.sum() >= 20 and (~hit).sum() >= 20
    if m["edge"] == "loose":
        ex = case.txs[last][2]
        assert any(ex[k + 1][0] <= ex[k][0] for k in range(len(ex) - 1))
        assert all(all(ex[k + 1][0] > ex[k][0] for k in range(len(ex) - 1)) for _t, _r, ex in case.txs[:last])
    if m["edge"] == "twin":
        # the last member has two donors within 2 * dis of each other; the reads between them have X's donor strictly between the two, and
        # those within the tolerance of both are not known through the member -- they are as soon as the second donor is out of reach
        dis, (d0, d1), rows = case.params["ss_dis"], m["twin"], np.array(m["between"])
        donors = {e for s, e in case.txs[last][2][:-1]}
        assert dis > 0 and 0 < d1 - d0 <= 2 * dis and {d0, d1} <= donors and len(rows) >= 40
        read_donor = np.array([[int(e) for e in want.ex_end[want.ex_off[i]:want.ex_off[i + 1] - 1] if d0 < e < d1] for i in rows])
        assert read_donor.shape == (len(rows), 1)
        both = (read_donor[:, 0] - d0 <= dis) & (d1 - read_donor[:, 0] <= dis)
        assert both.sum() >= 15 and ((want.info[rows[both]] & 3) == 2).all() and ((want.info[rows[~both]] & 1) != 0).all()
        far = wc.window_case(m["n_win"], edge="twin", dis=dis, twin_gap=2 * dis + 1)
        assert far.rows == case.rows and len(wc.describe(far.txs, far.rows, dis=dis)[0].members) == m["n_win"]
        moved = _oracle(oracle, far)
        assert ((moved.info[rows] & 1) != 0).all() and (moved.ref_tx[rows] == last).all()
        rest = np.setdiff1d(np.arange(len(case.rows)), rows[both])
        assert np.array_equal(moved.info[rest], want.info[rest]) and np.array_equal(moved.ref_tx[rest], want.ref_tx[rest])
    if m["shorts"]:
        # the early reads' sweep begins at member 0, the late reads' at member `shorts`: behind every short transcript
        first = {t.first for t in tiles}
        late = [i for i, r in enumerate(case.rows) if r[1] + 1 > wc.EARLY]
        assert len(late) == 60 and not first & set(late)
        for i, r in enumerate(case.rows):
            cur = wc.window(case.txs, 0, r[1] + 1, r[1] + wc.ref_len(r[3]))[0]
            assert cur == (m["shorts"] if i in late else 0), (i, cur)
        if m["n_iso"]:
            assert m["shorts"] == len(members) - 1 and (want.ref_tx[late] == last).sum() >= 20 and ((want.info[late] & 1) != 0).sum() >= 20
        else:
            assert m["shorts"] == len(members) and ((want.info[late] & 3) == 0).all()


@pytest.mark.parametrize("name", wc.names("slice"))
def test_slices(oracle, name):
    case = wc.case("slice", name)
    m = case.meta
    _shape(case)
    tiles = _one_descriptor(case)
    t = tiles[0]
    assert len(t.members) == m["members"]
    got = (len(t.st), len(t.en))
    assert got[0 if m["which"] == "st" else 1] == m["target"] and got[1 if m["which"] == "st" else 0] < m["cap"], got
    _single_part_keys(case)
    assert (t.st[0], t.en[0]) == m["first_keys"] and (t.st[-1], t.en[-1]) == m["last_keys"]
    want = _oracle(oracle, case)
    _all_three(want)
    _full_and_not(want)
    # known reads through the first and the last entry of both slices: the verbatim copies of the first and of the last family's isoform
    for kind, tx, keys in ((1, m["first_tx"], m["first_keys"]), (2, m["last_tx"], m["last_keys"])):
        n = 0
        for i in m["kinds"][kind]:
            lo, hi = int(want.ex_off[i]), int(want.ex_off[i + 1])
            ex = list(zip(want.ex_start[lo:hi].tolist(), want.ex_end[lo:hi].tolist()))
            assert int(want.info[i]) & 1 and int(want.ref_tx[i]) == tx
            junctions = [(0, ex[k][1], ex[k + 1][0]) for k in range(len(ex) - 1)]
            n += keys[0][1:] in ex and keys[1] in junctions
        assert n >= 10, (kind, n)


@pytest.mark.parametrize("name", wc.names("span"))
def test_bucket_span(oracle, name):
    case = wc.case("span", name)
    m, dis = case.meta, case.params["ss_dis"]
    _shape(case)
    tiles = wc.describe(case.txs, case.rows, dis=dis)
    want = _oracle(oracle, case)
    _all_three(want)
    assert len(tiles) == 4
    wide = 0
    for t in tiles:
        far = [i for i in m["far"] if t.first <= i < t.last]
        assert far and (t.tlo >> 9) == wc.LO_B and t.thi - t.tlo < (1 << 18) - 1
        assert (m["far_exon"][0] >> 9) == (m["far_exon"][1] >> 9) == wc.LO_B + m["nbk"] - 1
        if "last_base" in name:
            assert t.thi == m["far_exon"][1] and (t.thi + 1) % 512 == 0
        assert t.nbk in (m["nbk"], m["nbk"] + 1)
        wide += t.nbk > m["nbk"]
        # a known read whose last exon is the far one, an entry of the slice's last bucket
        hit = [i for i in far if int(want.info[i]) & 1 and int(want.ref_tx[i]) in m["far_tx"] and int(want.ex_start[want.ex_off[i + 1] - 1]) == m["far_exon"][0]]
        assert hit and t.st[-1] == (0,) + m["far_exon"]
    expect = {"span_384_first_base_d1": 1, "span_384_last_base_d1": 4}.get(name, 0)
    assert wide == expect and (tiles[0].tlo == wc.B0) == ("first_base" in name)


@pytest.mark.parametrize("name", wc.names("scan"))
def test_window_scan(oracle, name):
    case = wc.case("scan", name)
    _shape(case)
    tiles = _one_descriptor(case)
    assert tiles[0].cursor == 0 and tiles[0].scanned == case.meta["scanned"] and len(tiles[0].members) == case.meta["n_win"]
    assert tiles[0].members[0] == 0 and tiles[0].members[1] > 4000
    _all_three(_oracle(oracle, case))


@pytest.mark.parametrize("name", wc.names("positions"))
def test_staged_positions(oracle, name):
    case = wc.case("positions", name)
    _shape(case)
    cut, p = wc.tiles_of(case.rows)
    assert cut == [(0, 256), (256, 512), (512, 712)] and p["slab_tiles"] and p["reads_per_tile"] == 256
    want = _oracle(oracle, case)
    n_ex = np.diff(want.ex_off)
    assert [int(n_ex[a:b].sum()) for a, b in cut] == [case.meta["total"], wc.TILE_POS_CAP - 1, 700]
    _all_three(want)
    empty = [i for i in range(len(case.rows)) if (want.ex_end[want.ex_off[i]:want.ex_off[i + 1]] < want.ex_start[want.ex_off[i]:want.ex_off[i + 1]]).any()]
    assert empty == list(range(512))                              # (the reads with an empty exon: the first two tiles)
    want1 = _oracle(oracle, case, min_exon=1)
    assert int(np.diff(want1.ex_off)[:512].max()) == 2


@pytest.mark.parametrize("name", wc.names("rows"))
def test_rows_and_the_exon_count_byte(oracle, name):
    case = wc.case("rows", name)
    _shape(case)
    cut, p = wc.tiles_of(case.rows)
    assert p["slab_tiles"] and not p["many_exon_reads"] and not p["wide_cigar"] and p["reads_per_tile"] == 256 and len(cut) == 4
    want = _oracle(oracle, case)
    _all_three(want)
    n_ex = np.diff(want.ex_off)
    longs = np.nonzero(n_ex > 3)[0]
    assert n_ex[longs].tolist() == list(case.meta["counts"])
    for t, ((a, b), i) in enumerate(zip(cut, longs.tolist())):
        assert a < i < b - 1                                       # one per tile, between neighbours of three exons
        if case.meta["long_tx"]:                                   # known through the transcript it copies, down to its last exon
            tx = case.meta["long_tx"][t]
            assert int(want.info[i]) & 1 and int(want.ref_tx[i]) == tx
            last = case.txs[tx][2][-1]
            assert (int(want.ex_start[want.ex_off[i + 1] - 1]), int(want.ex_end[want.ex_off[i + 1] - 1])) == last
    tiles = wc.describe(case.txs, case.rows)
    one_window = all(len(t.st) <= wc.SLAB_KEY_CAP and len(t.en) <= wc.SLAB_KEY_CAP and len(t.members) <= wc.WIN_TX for t in tiles)
    assert one_window == (name != "rows_count_byte")              # (253 annotated exons and more in a tile's span: reason 3)
