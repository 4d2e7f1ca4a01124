"""GPU: the front of k_tile (l2r_tile.hip.h) -- the slot record asked for in front of every early return, the dictionary slices, directory
words and window vector loaded unconditionally with clamped indices (load_dict_slices, l2r_window.hip.h; load_tw_vec, l2r_slab.hip.h) --
on the tile pipeline, against the oracle, bit exact in all six result arrays.

A clamped load goes wrong where a slice ends: at the first and the last entry of a dictionary, at the last directory word, in a slice
of no or one entry, at the caps; a hoisted load where a workgroup leaves: behind the last tile, or at a tile of another instance.  The
cases are the smallest inputs that put a tile there, and the model of tests/window_cases.py says on the CPU that they do:

    ends      one annotation, one locus per case (each a tile of its own, run alone and all together):
              first    reads on the first transcript of the first chromosome: both slices begin at entry 0
              void     reads on that chromosome far from any transcript: both slices empty, a window of no member
              one_one  reads on the first exon of a two-exon transcript whose exons lie far apart: one START and one END entry
              st_only  reads on its last exon: one START entry, no END entry, a window of one member
              last     reads on the last transcript of the last annotated chromosome: the last entries of both dictionaries, and
                       the buckets of the last directory words
              no_anno  reads on a chromosome the annotation lacks: no bucket
              (no tile has END entries without START entries: the exon that ends at an END key reaches into the tile's first bucket or
               begins in it, and is an entry of the START slice either way)
    caps      slices of 167 / 168 entries, 383 / 384 buckets (the second directory word of a thread, thread + 256 <= nbk), windows of
              31 / 32 members (tw_vec_used at its edges; 0 and 1 member: void, one_one above) -- the builders of tests/window_cases.py
    slots     uploads of 1, 255, 256, 257 reads (inactive slots, a second tile of one read); one tile with reads of 1, 3, 4, 5, 8, 9, 23,
              24, 25 and 40 CIGAR operations (the vectors' edges, the tail loop behind SLAB_HEAD = 24) whose last read -- the one
              whose CIGAR ends the `cig` array -- has 1, 4, 5 or 25 of them
    exits     an inexact tile (a borderline -e), tiles of the WIDE instance and of k_tile_chunk beside exact ones in one upload: every
              instance leaves for the tiles that are not its own; the same results with the split, the WIDE instance and
              k_tile_chunk switched off

Routes: k_tile's EXACT instance; its general instance (L2R_TILE_SPLIT=0); -d 2 (the DIS instances); the accepted list wanted (the ACC
instances); the WIDE instance (the 40-isoform locus of `exits`).  l2r_debug_counters says where a case landed: word 3 tiles, 27 tiles
of the EXACT instance, 28 entries of the rest list, 12 tiles of the 64-bit masks, 26 tiles k_tile_chunk took.  k_tile_chunk has a front
of its own, which did not change.  Every case is a few hundred reads."""
import ctypes as C

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import util
from tests import upload_plan_restatement as plan
from tests import window_cases as wc
from tests.test_gpu_edges import _anno, _chain, _reads

pytestmark = pytest.mark.gpu

CLEARED = ("L2R_TILE_SPLIT", "L2R_ABLATE", "L2R_LAUNCH_ALL", "L2R_SIDE", "L2R_CHECK", "L2R_WIDE_DIRECT", "L2R_CHUNK_DIRECT", "L2R_TILE_ANYWAY", "L2R_STAMPS")
OFF = ("L2R_TILE_SPLIT", "L2R_WIDE_DIRECT", "L2R_CHUNK_DIRECT")
M, N_, S_ = 0, 3, 4
# route -> (outputs, ss_dis, switches set to 0)
ROUTES = {"exact": (1, 0, ()), "general": (1, 0, ("L2R_TILE_SPLIT",)), "dis": (1, 2, ()), "acc": (3, 0, ())}


@pytest.fixture(autouse=True)
def tile_pipeline(monkeypatch):
    monkeypatch.setenv("L2R_PIPELINE", "tile")
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)


def b(k):
    return k << wc.SITE_SHIFT


def _words(eng):
    cnt = (C.c_longlong * 29)()
    eng.lib.l2r_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert eng.lib.l2r_debug_counters(eng.ctx, cnt, 29) == 0
    return list(cnt)


def _same(got, want, outputs):
    """the six result arrays (without the accepted list nobody owes the ACCEPTED bit of `info`)"""
    if outputs & 2:
        util.assert_same_result(got, want, 0, 0)
        return
    for f in ("ex_off", "ex_start", "ex_end", "ex_flag", "ref_tx"):
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f))
    np.testing.assert_array_equal(got.info & 0x7f, want.info & 0x7f)
    np.testing.assert_array_equal(got.info >> 8, np.diff(want.ex_off).astype(np.uint32))


def _accepted_is_the_results(eng, got):
    acc = eng.download_accepted()
    idx = np.nonzero((got.info & 128) != 0)[0]
    lens = (got.info[idx] >> 8).astype(np.int64)
    g = synth._ragged_gather_index(got.ex_off[idx], lens)
    np.testing.assert_array_equal(acc.read_index, idx)
    np.testing.assert_array_equal(np.diff(acc.ex_off), lens)
    np.testing.assert_array_equal(acc.ex_start, got.ex_start[g])
    np.testing.assert_array_equal(acc.ex_end, got.ex_end[g])
    np.testing.assert_array_equal(acc.ex_flag, got.ex_flag[g])


def _classify(monkeypatch, af, reads, prm, outputs=1, off=(), runs=1):
    """[(result, counter words)] of `runs` runs of one upload, and the kernel behind the tile stage"""
    with monkeypatch.context() as m:
        for k in off:
            m.setenv(k, "0")
        eng = capi.Engine(0)                                     # (l2r_create reads the switches)
    try:
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(None)
        eng.set_outputs(outputs)
        out = [(eng.classify(reads, capi.default_params(**prm)), _words(eng))]
        for _ in range(runs - 1):
            eng.run(); eng.sync()
            out.append((eng.download(), _words(eng)))
        if outputs & 2:
            _accepted_is_the_results(eng, out[-1][0])
        kernel = (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()
    finally:
        eng.close()
    assert kernel.startswith("k_tile"), kernel
    return out


_wanted = {}


def _want(oracle, key, af, reads, prm):
    """the oracle's result, computed once per input and parameter set and never changed"""
    key = (key, tuple(sorted(prm.items())))
    if key not in _wanted:
        _wanted[key] = util.oracle_run(oracle, af, reads, oracle.default_params(**prm))
    return _wanted[key]


def _route(oracle, monkeypatch, key, af, reads, route, all_exact=True, **extra):
    """One route of one input: bit exact, and landed where the route says.  Returns the counter words."""
    outputs, dis, off = ROUTES[route]
    prm = dict(full_level=3, ss_dis=dis, **extra)
    want = _want(oracle, key, af, reads, prm)
    (got, w), = _classify(monkeypatch, af, reads, prm, outputs, off)
    print(key, route, "words", w)
    _same(got, want, outputs)
    assert w[3] >= 1 and w[13] == 0, w
    if route == "general":
        assert (w[27], w[28]) == (0, 0), w
    else:
        assert w[27] + w[28] == w[3], w
        if all_exact:                                            # (-d widens a tile's span: at a cap some tiles may leave the mask path)
            assert w[27] >= 1 if route == "dis" else w[27] == w[3], w
    return w


# ---- ends: the slices at the ends of their arrays, empty slices, slices of one entry, no bucket

FAR_A, FAR_B = 3000, 4000
ENDS_TXS = [
    (0, 0, [(b(2) + 101, b(2) + 200), (b(3) + 101, b(3) + 200), (b(4) + 101, b(4) + 200)]),
    (0, 1, [(b(FAR_A) + 101, b(FAR_A) + 200), (b(FAR_B) + 101, b(FAR_B) + 300)]),
    (1, 0, [(b(10) + 101, b(10) + 200), (b(11) + 101, b(11) + 200)]),
    (1, 1, [(b(600) + 101, b(600) + 200), (b(601) + 101, b(601) + 200), (b(602) + 101, b(602) + 200)]),
]
NOVEL = lambda k: [(b(k) + 101, b(k) + 200), (b(k) + 301, b(k) + 400)]         # two exons in bucket k


def _locus_rows(tid, iso, n, seed):
    """n reads over the exons `iso`: verbatim (whole, or from the second exon on), the last exon shortened, a donor moved, an exon
    skipped, a single exon, a later start"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ex = [list(x) for x in iso]
        kind = i % 6
        if kind == 0 and len(ex) > 2 and i % 12:
            del ex[0]                                            # (from an acceptor on: a known read)
        elif kind == 1:
            ex[-1][1] -= 1 + int(rng.integers(0, 30))
        elif kind == 2 and len(ex) > 1:
            ex[0][1] -= 5
        elif kind == 3 and len(ex) > 2:
            del ex[1]
        elif kind == 4:
            ex = [[ex[0][0], ex[0][1] - int(rng.integers(0, 30))]]
        elif kind == 5:
            ex[0][0] += 1 + int(rng.integers(0, 30))
        pos0, ops = _chain([tuple(x) for x in ex])
        rows.append((tid, pos0, i & 1, ops))
    return sorted(rows, key=lambda r: r[1])


ENDS_LOCI = {
    "first": (0, ENDS_TXS[0][2]), "void": (0, NOVEL(1000)), "one_one": (0, NOVEL(FAR_A)),
    "st_only": (0, [(b(FAR_B) + 101, b(FAR_B) + 180), (b(FAR_B) + 221, b(FAR_B) + 300)]),
    "last": (1, ENDS_TXS[3][2]), "no_anno": (2, NOVEL(5)),
}
# (START entries, END entries, window members) of the locus's tile
ENDS_MODEL = {"first": (3, 2, 1), "void": (0, 0, 0), "one_one": (1, 1, 1), "st_only": (1, 0, 1), "last": (3, 2, 1)}


def _ends_rows(name, n=60):
    order = list(ENDS_LOCI)
    loci = order if name == "all" else [name]
    rows = []
    for q in loci:
        tid, iso = ENDS_LOCI[q]
        rows += _locus_rows(tid, iso, n, 17 + order.index(q))
    return sorted(rows, key=lambda r: (r[0], r[1]))


def _check_ends_model(name, rows):
    """the model's word on where the locus's tile sits: its slices, where they begin and end in the dictionaries, its window"""
    if name in ("no_anno", "all"):
        return
    (t,) = wc.describe(ENDS_TXS, rows)
    dic = wc.Dictionaries(ENDS_TXS)
    assert (len(t.st), len(t.en), len(t.members)) == ENDS_MODEL[name], (name, t)
    if name == "first":
        assert t.st == dic.st[:3] and t.en == dic.en[:2]
    if name == "last":
        assert t.st == dic.st[-3:] and t.en == dic.en[-2:]
        assert (t.thi >> wc.SITE_SHIFT) == dic.nb[1] - 1          # the tile's last bucket is the chromosome's last: the directory's last words


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(ENDS_LOCI) + ["all"])
def test_slices_at_the_ends_of_their_arrays(oracle, monkeypatch, name, route):
    rows = _ends_rows(name)
    _check_ends_model(name, rows)
    # (a tile without a window member or on a chromosome without buckets may be either instance's: the words must add up)
    w = _route(oracle, monkeypatch, "ends_" + name, _anno(ENDS_TXS), _reads(rows), route, all_exact=name not in ("void", "no_anno", "all"))
    assert w[3] == (len(ENDS_LOCI) if name == "all" else 1), w


# ---- caps: full slices, the last staged bucket, the window vectors

CAPS = [("slice", "st_167_m24"), ("slice", "st_168_m24"), ("slice", "en_167_m32"), ("slice", "en_168_m32"),
        ("span", "span_383"), ("span", "span_384"), ("window", "win_31_contig"), ("window", "win_32_contig")]
_caps = {}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("family,name", CAPS)
def test_slices_buckets_and_windows_at_their_caps(oracle, monkeypatch, family, name, route):
    if name not in _caps:
        case = wc.case(family, name)
        _caps[name] = (case, _anno(case.txs), _reads(case.rows))
    case, af, reads = _caps[name]
    t = wc.describe(case.txs, case.rows)[0]
    want_sizes = {"st_167_m24": (167, None), "st_168_m24": (168, None), "en_167_m32": (None, 167), "en_168_m32": (None, 168)}.get(name)
    if want_sizes:
        assert (want_sizes[0] in (None, len(t.st))) and (want_sizes[1] in (None, len(t.en))), (len(t.st), len(t.en))
    if family == "span":
        assert t.nbk == case.meta["nbk"]
    if family == "window":
        assert len(t.members) == case.meta["n_win"]
    # -d 2 makes a span of 383 / 384 buckets two wider: beyond the cap such a tile is not on the mask path at all
    w = _route(oracle, monkeypatch, name, af, reads, route, all_exact=not (family == "span" and route == "dis"))
    if route != "dis":
        assert w[4] == w[3] and w[12] == 0, w
        if family == "slice":
            assert (w[24], w[25]) == (len(t.st), len(t.en)), w


# ---- slots: inactive slots, a second tile of one read, CIGAR lengths at the vectors' edges, the end of the `cig` array

@pytest.mark.parametrize("route", ["exact", "general"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_uploads_around_one_tile(oracle, monkeypatch, n, route):
    rows = _locus_rows(0, ENDS_TXS[0][2], n, 5)
    tiles, _ = wc.tiles_of(rows)
    assert len(tiles) == (2 if n == 257 else 1) and tiles[-1][1] - tiles[-1][0] == (1 if n == 257 else n)
    w = _route(oracle, monkeypatch, "upload_%d" % n, _anno(ENDS_TXS), _reads(rows), route)
    assert w[3] == len(tiles), w


CIG_OPS = (1, 3, 4, 5, 8, 9, 23, 24, 25, 40)


def _read_of(n_ops, start):
    """A read of exactly n_ops CIGAR operations from base `start`: exons of 40 bases, introns of 60; an even count begins with a soft clip"""
    k = (n_ops + 1) // 2
    pos0, ops = _chain([(start + 100 * j, start + 100 * j + 39) for j in range(k)])
    if n_ops % 2 == 0:
        ops = [(5, S_)] + ops
    assert len(ops) == n_ops
    return pos0, ops


def _cigar_rows(last_ops):
    rows = []
    for i in range(60):
        pos0, ops = _read_of(CIG_OPS[i % len(CIG_OPS)], b(2) + 101 + (i % 7))
        rows.append((0, pos0, i & 1, ops))
    rows += _locus_rows(0, ENDS_TXS[0][2], 30, 9)                  # ordinary reads of the locus between them
    rows.sort(key=lambda r: r[1])
    pos0, ops = _read_of(last_ops, max(r[1] for r in rows) + 10)   # the upload's last read: its CIGAR ends the array
    return rows + [(0, pos0, 0, ops)]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("last_ops", [1, 4, 5, 25])
def test_cigar_lengths_at_the_vector_edges(oracle, monkeypatch, last_ops, route):
    rows = _cigar_rows(last_ops)
    reads = _reads(rows)
    assert len(wc.tiles_of(rows)[0]) == 1 and reads.cig_off[-1] == len(reads.cig) and len(rows[-1][3]) == last_ops
    assert sorted(set(len(r[3]) for r in rows[:-1]) & set(CIG_OPS)) == sorted(CIG_OPS)
    assert len(reads.cig) <= 32 * len(rows)                      # (an upload of long CIGARs is not the tile path's)
    w = _route(oracle, monkeypatch, "cigars_%d" % last_ops, _anno(ENDS_TXS), reads, route)
    assert w[3] == 1, w


# ---- exits: every instance leaves for the tiles that are not its own

MIN_EXON = 25
N_PLAIN = 6


def _exits_case():
    """chromosome 1: a 40-isoform locus (the WIDE instance's); chromosome 2: a locus of 64 window members (k_tile_chunk's); chromosome 3:
    six loci of ordinary reads (more than half of the upload's tiles: else its later runs are the slab pipeline's), in the second one
    a read with an inner exon shorter than -e (its tile counts: the general instance's)"""
    wide, chunk = wc.window_case(40, n_reads=300), wc.window_case(64, n_reads=300)
    iso = [(b(20) + 101, b(20) + 200), (b(21) + 101, b(21) + 200), (b(22) + 101, b(22) + 200)]
    shift = lambda ex, k: [(s + b(k), e + b(k)) for s, e in ex]
    txs = list(wide.txs) + [(1 if t >= 0 else t, r, ex) for t, r, ex in chunk.txs] + [(2, k & 1, shift(iso, 1000 * k)) for k in range(N_PLAIN)]
    rows = list(wide.rows) + [(1, p, r, ops) for _t, p, r, ops in chunk.rows]
    for k in range(N_PLAIN):
        rows += _locus_rows(2, shift(iso, 1000 * k), 80, 40 + k)
    short = shift(iso, 1000)
    short[1] = (short[1][0], short[1][0] + MIN_EXON - 6)          # an inner exon of MIN_EXON - 5 bases
    pos0, ops = _chain(short)
    rows.append((2, pos0, 0, ops))
    rows.sort(key=lambda r: (r[0], r[1]))
    return txs, rows


def test_every_instance_leaves_for_the_tiles_of_the_others(oracle, monkeypatch):
    txs, rows = _exits_case()
    af, reads = _anno(txs), _reads(rows)
    firsts = plan._tile_firsts(reads)
    n_tiles = len(firsts) - 1
    _, min_n, max_d, min_seg, _ = plan._tile_stats(reads, firsts)
    exact = (min_n >= 3) & (max_d <= 50) & (min_seg >= MIN_EXON)                   # tile_exact, l2r_slab.hip.h
    plain = reads.tid[firsts[:-1]] == 2
    assert int((~exact).sum()) == 1 and bool(plain[~exact].all()) and int((plain & exact).sum()) == N_PLAIN - 1, (exact, plain)
    prm = dict(full_level=3, min_exon=MIN_EXON)
    want = _want(oracle, "exits", af, reads, prm)
    on = _classify(monkeypatch, af, reads, prm, 1, (), runs=2)
    off = _classify(monkeypatch, af, reads, prm, 1, OFF, runs=2)
    for k in (0, 1):
        (got_on, w_on), (got_off, w_off) = on[k], off[k]
        print("exits run", k, "words on", w_on, "off", w_off)
        _same(got_on, want, 1)
        _same(got_off, want, 1)
        for f in ("ex_off", "ex_start", "ex_end", "ex_flag", "info", "ref_tx"):
            assert np.array_equal(getattr(got_on, f), getattr(got_off, f)), (k, f)
        assert w_on[3] == n_tiles == w_off[3] and w_on[13] == 0 and w_off[13] == 0
        assert (w_off[27], w_off[28], w_off[26]) == (0, 0, 0), w_off
    # the steady run: the exact tiles of the 32-bit masks are the EXACT instance's; the inexact one, the 64-bit-mask tiles (the WIDE
    # instance takes them) and the chunked tiles (k_tile_chunk takes them) are on the rest list, where the general instance leaves the last two kinds
    w = on[1][1]
    n_wide, n_chunk = int((reads.tid[firsts[:-1]] == 0).sum()), int((reads.tid[firsts[:-1]] == 1).sum())
    assert (w[27], w[28]) == (N_PLAIN - 1, n_tiles - (N_PLAIN - 1)), w
    assert 2 * (n_wide + n_chunk) <= n_tiles
    assert w[12] == n_wide and w[26] >= 1 and w[23] == n_chunk, (w, n_wide, n_chunk)
