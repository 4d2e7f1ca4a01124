"""GPU: the one-window kernels at the edges of their descriptor caps -- against the oracle, bit exact, on every kernel pipeline.

k_classify_fast, k_probe_slab, k_probe_slab_wide and k_tile's EXACT, general and WIDE instances classify a tile from ONE window and trust
its descriptor (make_descriptor, l2r_window.hip.h; k_pass_a).  Every case of tests/window_cases.py lands a locus on one side of a cap of
that descriptor -- tests/test_window_cases_cpu.py has proved on the CPU that it does -- and l2r_debug_counters proves where the engine
put it: word 3 = all tiles, word 4 + k = tiles with reason k (0: on the 32-bit masks), 12 = tiles of the 64-bit-mask kernel, 23 = tiles
of the chunked kernels, 24 / 25 = the largest START / END slice, 27 / 28 = tiles of k_tile's EXACT instance / of the rest list.

    window        31 / 32 | 33 .. 62 / 63 | 64 members: 32-bit masks | 64-bit masks | reason 4 (classic: reason 4 from 33 on)
    slices        167 / 168 | 169 START or END entries (classic 223 / 224 | 225): staged | reason 3
    buckets       383 / 384 | 385: staged | reason 2
    window scan   the transcript behind the span is the 4096th | 4097th one scanned: found | reason 5
    -d            64 | 65: mask kernels | reason 7
    positions     2399 / 2400 | 2401 exons of a tile (k_tile), 2535 / 2536 | 2537 (k_probe_slab): staged | written directly
    rows          23 / 24 | 25 / 26 exons of a read (a slab column), 253 / 254 | 255 / 256 (the tile is never exact)

On the tile pipeline a case also runs with the switch that hands its tiles to the other kernel that can take them: L2R_TILE_SPLIT=0
(k_tile's general instance instead of EXACT), L2R_WIDE_DIRECT=0 (k_probe_slab_wide instead of the WIDE instance), L2R_CHUNK_DIRECT=0
(k_probe_slab_chunked instead of k_tile_chunk)."""
import ctypes as C

import numpy as np
import pytest

from lr2rmats_amd import capi
from tests import util
from tests import window_cases as wc
from tests.test_gpu_edges import _anno, _reads, _run, pipeline  # noqa: F401  (pipeline: autouse fixture)

pytestmark = pytest.mark.gpu

CLEARED = ("L2R_TILE_SPLIT", "L2R_ABLATE", "L2R_LAUNCH_ALL", "L2R_SIDE", "L2R_CHECK", "L2R_WIDE_DIRECT", "L2R_CHUNK_DIRECT", "L2R_TILE_ANYWAY")
SWITCH = {"fast": "L2R_TILE_SPLIT", "wide": "L2R_WIDE_DIRECT", "chunked": "L2R_CHUNK_DIRECT"}


@pytest.fixture(autouse=True)
def switches(pipeline, monkeypatch):
    """(the pipeline is the fixture's; every other switch of the engine is off unless a route sets it)"""
    for k in CLEARED:
        monkeypatch.delenv(k, raising=False)


_arrays, _wanted = {}, {}        # per case: (case, annotation, reads); per (case, level, parameters): (parameters, the oracle's result)


def _case(oracle, family, name, level=3, **kw):
    """(case, annotation, reads, parameters, the oracle's result) -- computed once per parameter set, never changed"""
    if name not in _arrays:
        case = wc.case(family, name)
        _arrays[name] = (case, _anno(case.txs), _reads(case.rows))
    case, af, reads = _arrays[name]
    key = (name, level, tuple(sorted(kw.items())))
    if key not in _wanted:
        prm = dict(case.params, full_level=level, **kw)
        _wanted[key] = (prm, util.oracle_run(oracle, af, reads, oracle.default_params(**prm)))
    return _arrays[name] + _wanted[key]


def _routes(pipeline, kind):
    """[(switch or None)] for a case whose tiles are `kind` (fast: 32-bit masks, wide: 64-bit masks, chunked)"""
    return [None, SWITCH[kind]] if pipeline == "tile" else [None]


def _go(oracle, family, name, pipeline, monkeypatch, kind, land, levels=None, **kw):
    case = wc.case(family, name)
    for level in levels or case.levels:
        case, af, reads, prm, want = _case(oracle, family, name, level, **kw)
        for switch in _routes(pipeline, kind):
            if switch:
                monkeypatch.setenv(switch, "0")
            w = []
            _run(oracle, af, reads, words=w, want=want, n_words=29, **prm)
            print(name, pipeline, "level", level, switch or "-", "words", w)
            assert w[3] >= 1 and w[13] == 0, w
            land(w, switch, want)
            if switch:
                monkeypatch.delenv(switch)


def _exact_instance(w, pipeline, switch, all_of_them):
    """words 27 / 28: k_tile's EXACT instance took every tile / none (none, and no rest list, with L2R_TILE_SPLIT=0)"""
    if pipeline == "tile":
        assert w[27] == (w[3] if all_of_them and switch != "L2R_TILE_SPLIT" else 0), w
        if switch == "L2R_TILE_SPLIT":
            assert w[28] == 0, w


# ---- 1: the window's size

@pytest.mark.parametrize("name", wc.names("window"))
def test_window_size(oracle, name, pipeline, monkeypatch):
    case = wc.case("window", name)
    n, m = case.meta["n_win"], case.meta
    classic = pipeline == "classic"
    kind = "fast" if n <= wc.WIN_TX else "wide" if n <= wc.WIDE_MEMBERS else "chunked"

    def land(w, switch, want):
        assert w[1] == 0, w
        if n <= wc.WIN_TX:
            assert w[4] == w[3] and w[12] == 0, w
        elif classic:
            assert w[8] == w[3], w
        elif n <= wc.WIDE_MEMBERS:
            assert w[12] == w[3], w
        else:
            assert w[8] == w[3] == w[23], w
        _exact_instance(w, pipeline, switch, n <= wc.WIN_TX)
        if n <= (wc.WIN_TX if classic else wc.WIDE_MEMBERS):
            # a member without TX_COMPACT: the reads of several exons that reach it are the generic kernel's, and nobody else is
            multi = int((np.diff(want.ex_off) > 1).sum())
            if m["edge"] == "twin":
                # a read donor within the tolerance of both of the member's twin donors: the reads between them, and nobody else
                assert 1 <= w[0] <= len(m["between"]), (w, len(m["between"]))
            else:
                assert w[0] == (multi if m["edge"] == "loose" else 0), (w, multi)
    _go(oracle, "window", name, pipeline, monkeypatch, kind, land)


# ---- 2: the dictionary slices

def _land_slice(case, pipeline):
    m = case.meta
    cap = wc.KEY_CAP if pipeline == "classic" else wc.SLAB_KEY_CAP
    t = wc.describe(case.txs, case.rows)[0]
    st, en = len(t.st), len(t.en)
    inside = st <= cap and en <= cap
    wide = m["members"] > wc.WIN_TX

    def land(w, switch, want):
        assert (w[24], w[25]) == (st, en) and w[1] == 0, (w, st, en)
        if pipeline == "classic":
            if wide:
                assert w[8] == w[3], w
            elif inside:
                assert w[4] == w[3] and w[0] == 0, w
            else:
                assert w[7] == w[3] and w[0] == len(case.rows), w             # the generic kernel has every read
        elif inside:
            assert (w[12] == w[3] if wide else w[4] == w[3] and w[12] == 0) and w[0] == 0, w
        else:
            assert w[7] == w[3] == w[23], w                                   # every tile goes to the chunked kernels
        _exact_instance(w, pipeline, switch, inside and not wide)
    return land, ("chunked" if not inside else "wide" if wide else "fast"), inside


@pytest.mark.parametrize("name", wc.names("slice"))
def test_slices(oracle, name, pipeline, monkeypatch):
    case = wc.case("slice", name)
    land, kind, _ = _land_slice(case, pipeline)
    _go(oracle, "slice", name, pipeline, monkeypatch, kind, land)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", [n for n in wc.names("slice") if "_%d_" % wc.SLAB_KEY_CAP in n])
def test_full_slices_with_a_junction_table(oracle, name, split, pipeline):
    """k_tile stages the rows of a -j table over the dead dictionary slices: a full slice and staged rows in one tile (the other pipelines
    check the junctions in a kernel of their own)"""
    case, af, reads, _prm, base = _case(oracle, "slice", name)
    _j, sj = util.junction_table(af, reads, base, 7, cover=0.7)
    w = []
    got, want = _run(oracle, af, reads, sj=sj, words=w, n_words=29, full_level=3, split_trans=split, min_sj_cnt=1)
    t = wc.describe(case.txs, case.rows)[0]
    print(name, pipeline, "split", split, "words", w)
    assert (w[24], w[25]) == (len(t.st), len(t.en)) and w[7] == 0 and w[13] == 0, w
    # the tiles stayed where the slices are staged whole: the 32-bit masks (24 / 32 members), the 64-bit masks (40; classic: reason 4)
    if case.meta["members"] <= wc.WIN_TX:
        assert w[4] == w[3] and w[12] == 0 and w[0] == 0, w
    elif pipeline == "classic":
        assert w[8] == w[3], w
    else:
        assert w[12] == w[3] and w[23] == 0 and w[0] == 0, w
    if pipeline == "tile":                                        # k_tile itself took them, tile by tile
        assert (eng_kernel := _tile_kernel(oracle, af, reads, sj, split)).startswith("k_tile"), eng_kernel
        assert w[27] == (w[3] if case.meta["members"] <= wc.WIN_TX else 0), w
    assert ((want.info & 7) == 6).sum() > 20 and len(sj[0]) > 10          # (reads the junction check looks at)


def _tile_kernel(oracle, af, reads, sj, split):
    """the kernel behind the tile stage of a run with these inputs (l2r_stage_kernel)"""
    eng = capi.Engine(0)
    try:
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(sj)
        eng.classify(reads, capi.default_params(full_level=3, split_trans=split, min_sj_cnt=1))
        eng.lib.l2r_stage_kernel.restype = C.c_char_p
        eng.lib.l2r_stage_kernel.argtypes = [C.c_void_p, C.c_int]
        return (eng.lib.l2r_stage_kernel(eng.ctx, 1) or b"").decode()
    finally:
        eng.close()


# ---- 3: the bucket span

@pytest.mark.parametrize("name", wc.names("span"))
def test_bucket_span(oracle, name, pipeline, monkeypatch):
    case = wc.case("span", name)
    # (the classic upload chooses its reads per tile by a sample of the tiles' spans: the model cuts the tiles as that pipeline does)
    tiles = wc.describe(case.txs, case.rows, dis=case.params["ss_dis"], slab=pipeline != "classic")
    over = sum(t.nbk > wc.DIR_CAP for t in tiles)
    assert all(any(t.first <= i < t.last for i in case.meta["far"]) for t in tiles)

    def land(w, switch, want):
        assert w[3] == len(tiles) and w[6] == over and w[4] == w[3] - over, (w, over)
        if not over:
            assert w[0] == 0, w
        elif over == len(tiles):
            assert w[0] == len(case.rows), w
    _go(oracle, "span", name, pipeline, monkeypatch, "fast", land)


# ---- 4: the window scan

@pytest.mark.parametrize("name", wc.names("scan"))
def test_window_scan(oracle, name, pipeline, monkeypatch):
    case = wc.case("scan", name)
    found = case.meta["scanned"] <= wc.WIN_SCAN

    def land(w, switch, want):
        assert (w[4], w[9]) == ((w[3], 0) if found else (0, w[3])), w
        assert w[0] == (0 if found else len(case.rows)), w
        _exact_instance(w, pipeline, switch, found)
    _go(oracle, "scan", name, pipeline, monkeypatch, "fast", land)


# ---- 5: -d

@pytest.mark.parametrize("name", wc.names("dis"))
def test_splice_distance(oracle, name, pipeline, monkeypatch):
    case = wc.case("dis", name)
    masks = case.params["ss_dis"] <= wc.DIS_MASK_MAX

    def land(w, switch, want):
        assert w[11] == (0 if masks else w[3]), w
        if not masks:
            assert w[0] == len(case.rows), w
    _go(oracle, "dis", name, pipeline, monkeypatch, "fast", land)


# ---- 6: the staged positions

@pytest.mark.parametrize("name", wc.names("positions"))
def test_staged_positions(oracle, name, pipeline, monkeypatch):
    """The exon total of a tile reaches the caps only through empty inner exons (-e 0, N operations back to back), and a read with an empty
    exon is the generic kernel's on every pipeline whatever its tile holds (`sane`, k_classify_fast; the slab kernels likewise): word 0
    counts those reads -- the 512 of the first two tiles -- at or below the cap, and nobody else above it, where the reads behind the
    staged positions are written directly: they are the same reads.  What the cap can break is the write-out of the staged positions:
    the comparison with the oracle.  With -e 1 the same input has two exons per read and nothing for the generic kernel."""
    case = wc.case("positions", name)
    cap = {"tile": wc.TILE_POS_CAP, "slab": wc.SLAB_POS_CAP}.get(pipeline)

    def land(w, switch, want):
        s, e = want.ex_start, want.ex_end
        empty = int(np.add.reduceat((e < s).astype(np.int64), want.ex_off[:-1]).astype(bool).sum())
        assert empty == 512 and w[4] == w[3] == 3, (w, empty)
        if cap and case.meta["total"] <= cap:
            assert w[0] == empty, w
        else:
            assert w[0] <= 512, w                                 # (at most the reads of the tiles that hold such reads)
    _go(oracle, "positions", name, pipeline, monkeypatch, "fast", land)

    def land1(w, switch, want):
        assert w[0] == 0 and int(np.diff(want.ex_off)[:512].max()) == 2, w
    _go(oracle, "positions", name, pipeline, monkeypatch, "fast", land1, min_exon=1)


# ---- 7: the rows of a slab column, the exon-count byte

def _words(eng):
    cnt = (C.c_longlong * 29)()
    eng.lib.l2r_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    assert eng.lib.l2r_debug_counters(eng.ctx, cnt, 29) == 0
    return list(cnt)


@pytest.mark.parametrize("name", wc.names("rows"))
def test_rows_and_the_exon_count_byte(oracle, name, pipeline, monkeypatch):
    """On the tile pipeline words 27 / 28 say who took the tiles: the first run of an upload marks tiles for k_tile's EXACT instance only
    when no tile is inexact, the second run knows the rest list's length.  A tile with a read of 255 exons or more is inexact under every
    threshold and never the EXACT instance's; where the long reads copy annotated transcripts of 253 exons and more the tiles' START
    slices are beyond SLAB_KEY_CAP, and every tile is on the rest list from the first run on."""
    case, af, reads, prm, want = _case(oracle, "rows", name)
    w = []
    _run(oracle, af, reads, words=w, want=want, n_words=29, **prm)
    print(name, pipeline, "words", w)
    tiles = wc.describe(case.txs, case.rows)
    n_ex = np.diff(want.ex_off)
    if pipeline == "slab" and name != "rows_count_byte":
        # a read whose exon bound (ops + 3) / 2 is beyond SLAB_ROWS has no slab column: a dense outlier, the generic kernel's -- and nobody else is
        outliers = sum((len(r[3]) + 3) >> 1 > wc.SLAB_ROWS for r in case.rows)
        assert outliers == sum(n >= wc.SLAB_ROWS for n in case.meta["counts"]) and w[4] == w[3] == len(tiles) and w[0] == outliers, (w, outliers)
    if pipeline != "tile":
        return
    never = sum(int(n_ex[t.first:t.last].max()) >= wc.NEVER_EXACT for t in tiles)
    one_window = all(len(t.st) <= wc.SLAB_KEY_CAP and len(t.en) <= wc.SLAB_KEY_CAP for t in tiles)
    eng = capi.Engine(0)
    try:
        eng.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
        eng.set_junctions(None)
        util.assert_same_result(eng.classify(reads, capi.default_params(**prm)), want, 0, 0)
        first = _words(eng)
        eng.run(); eng.sync()
        util.assert_same_result(eng.download(), want, 0, 0)
        second = _words(eng)
    finally:
        eng.close()
    print(name, "first run", first, "second run", second)
    assert first[3] == len(tiles) and first[13] == 0 and second[13] == 0
    if not one_window:
        assert (first[27], first[28], first[7]) == (0, first[3], first[3]), first
        assert (second[27], second[7], second[23]) == (0, second[3], second[3]), second     # no tile on the 32-bit masks: none for the EXACT instance
    else:
        long_ = int((n_ex >= wc.NEVER_EXACT).sum())               # (a read's exon count is a byte on the mask path: these are the generic kernel's)
        assert first[4] == first[3] and first[0] == long_ and second[0] == long_, (first, second, long_)
        assert (first[27], first[28]) == ((first[3], 0) if never == 0 else (0, never)), (first, never)
        assert (second[27], second[28]) == (second[3] - never, never), (second, never)
