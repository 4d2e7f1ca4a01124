"""The read lists of `update-gtf -a / -k / -v / -u` on the GPU: l2r_gtftext_anno / _reads / _list / _list_out (k_rl_count, k_scan_u32,
k_rl_take, k_rl_measure in both forms) and l2r_gtftext_lines behind a list (k_rl_write on the LDS and on the direct path) against
tests/read_list_restatement.py: the selection alone, the text of every case of tests/test_read_lists_cpu.py, the tile geometry, the
batch cut, the routes, and the results of a run where they lie.  Every case asserts the route and an intact guard (L2R_CHECK=1)."""
import os

import numpy as np
import pytest

from lr2rmats_amd import capi, synth
from tests import read_list_cases as rc
from tests import read_list_restatement as rr
from tests import util

pytestmark = pytest.mark.gpu

TILE = capi.header_define("L2R_GTX_TILE")
LDS = capi.header_define("L2R_GTX_LDS_BYTES")
SCAN_TILE = 16384                                       # elements of one round of k_scan_u32 (1024 lanes x SCAN_PER_THREAD)


@pytest.fixture(scope="module")
def eng():
    os.environ["L2R_CHECK"] = "1"                       # (read when the context is made: the guard behind the text is filled and looked at)
    try:
        e = capi.Engine(0)
    finally:
        del os.environ["L2R_CHECK"]
    yield e
    e.close()


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at %d: %r / %r" % (len(got), len(want), k, got[max(0, k - 60):k + 60], want[max(0, k - 60):k + 60])


def check(e, case, lists=rr.LISTS, max_blocks=1 << 20, max_bytes=1 << 30, route=0, given=False):
    """The engine's selection and text of a case's lists against the restatement; route and guard.  The stats per list."""
    if not given:
        rc.engine_reads(e, case)
    out = {}
    for lst in lists:
        want_sel, want = rr.select(case, lst), rr.texts(case, lst)          # (raises where a block lies outside the domain)
        sel, text, (m, n_lines, n_bytes), st = rc.engine_list(e, lst, max_blocks, max_bytes)
        assert sel == want_sel, lst
        assert text == b"".join(want), (lst, first_difference(text, b"".join(want)))
        assert (m, n_lines, n_bytes) == (len(want), sum(t.count(b"\n") for t in want), sum(len(t) for t in want))
        assert st["blocks"] == m and st["route"] == route and st["guard_intact"] == 1
        assert st["piece_blocks"] == sum(1 for b in want_sel if b[3] >= 0)
        out[lst] = st
    return out


def head(case, n):
    x = int(case["ex_off"][n])
    c = dict(case)
    for k in ("tid", "qname", "info", "ref_tx"):
        c[k] = case[k][:n]
    if case.get("tid_name") is not None:
        c["tid_name"] = case["tid_name"][:n]
    c["ex_off"] = case["ex_off"][:n + 1]
    for k in ("xs", "xe", "f"):
        c[k] = case[k][:x]
    return c


@pytest.fixture(scope="module")
def mixed():
    """3 x TILE + 17 reads of every class, made once."""
    rng = np.random.default_rng(7)
    return rc.make_case(70, rng.choice([1, 2, 2, 3, 4, 6, 9, 14, 25, 70], 3 * TILE + 17), flags="pieces")


# ---------------------------------------------------------------------------------------------------- the selection alone

def selection(e, case, lst):
    m, _, _ = e.gtftext_list(lst)
    cols = e.gtftext_list_out(m)
    return list(zip(*[c.tolist() for c in cols])) if m else []


@pytest.fixture(scope="module")
def many():
    """One count beyond k_scan_u32's tile plus 17: short reads, classes alternating, pieces 0, 1 or 2."""
    n = SCAN_TILE + 17
    rows = [[rc.NJ, 0, 0], [0], [rc.NJ, 0, rc.UJ, rc.NJ, 0], [0, 0]]
    return rc.flag_case(90, [rows[i % 4] for i in range(n)], info=(rc.NOVEL_FAIL, rc.KNOWN, rc.NOVEL_FAIL, rc.UNRECOG, rc.NOVEL_PASS), name_len=(1, 3))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, SCAN_TILE + 17])
def test_selection_at_read_counts(eng, many, n):
    case = head(many, n)
    rc.engine_reads(eng, case)
    for lst in rr.LISTS:
        assert selection(eng, case, lst) == rr.select(case, lst), lst
        assert eng.gtftext_stats()["piece_blocks"] == sum(1 for b in rr.select(case, lst) if b[3] >= 0)


def test_selection_by_class_and_piece_count(eng):
    rows = {0: [rc.NJ, rc.NJ, 0], 1: [rc.NJ, 0, 0], 2: [rc.NJ, rc.UJ, rc.NJ, 0, 0], 11: [rc.NJ, rc.UJ] * 10 + [rc.NJ, 0, 0]}
    for k, r in rows.items():
        assert len(rr.pieces(r)) == k
    cases = [rc.flag_case(91, [rows[k] for k in (0, 1, 2, 11, 11, 0, 2, 1) * 9])]                                       # pieces per read: 0, 1, 2, 11
    cases += [rc.flag_case(92, [rows[2]] * 70, info=c) for c in (rc.KNOWN, rc.UNRECOG, rc.NOVEL_PASS, rc.NOVEL_FAIL, 0x03)]     # all of one class: the other lists are empty
    cases.append(rc.flag_case(93, [rows[1], rows[11]] * 40, info=(rc.NOVEL_FAIL, rc.KNOWN, rc.UNRECOG)))                  # alternating
    cases.append(rc.flag_case(94, [[0]] * 40 + [[rc.NJ, 0, rc.UJ] * 100] + [[0, 0]] * 40, info=rc.NOVEL_FAIL))            # a split candidate of 300 exons among short reads
    for case in cases:
        for has_sj, split in ((True, True), (True, False), (False, True)):
            case["has_sj"], case["split"] = has_sj, split
            rc.engine_reads(eng, case)
            for lst in rr.LISTS:
                assert selection(eng, case, lst) == rr.select(case, lst), (lst, has_sj, split)
    assert len(rr.pieces(cases[-1]["f"][40:340].tolist())) == 100


# ---------------------------------------------------------------------------------------------------- the text

def test_every_cpu_case_in_both_forms(eng, monkeypatch):
    cases = rc.class_cases() + rc.piece_cases() + rc.name_cases()
    for form in (0, 1):
        monkeypatch.setenv("L2R_GTX_WAVE", str(form))
        for case in cases:
            for st in check(eng, case).values():
                assert st["blocks"] == 0 or st["wave_form"] == form


def test_the_form_follows_the_exons_per_read(eng):
    assert check(eng, rc.make_case(5, [32, 33, 31], info=rc.KNOWN), [rr.ALL])[rr.ALL]["wave_form"] == 0
    assert check(eng, rc.make_case(5, [32, 33, 32], info=rc.KNOWN), [rr.ALL])[rr.ALL]["wave_form"] == 1


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 300, 2000])
def test_exons_per_read_in_both_forms(eng, monkeypatch, k):
    case = rc.make_case(100 + k, [k] * 5, info=(rc.KNOWN, rc.NOVEL_FAIL, rc.NOVEL_PASS), flags="pieces")
    for form in (0, 1):
        monkeypatch.setenv("L2R_GTX_WAVE", str(form))
        check(eng, case, [rr.ALL, rr.NOVEL])


# ---------------------------------------------------------------------------------------------------- tile geometry

@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_block_counts_around_the_tile(eng, mixed, n):
    st = check(eng, head(mixed, n), [rr.ALL])[rr.ALL]
    assert st["tiles_lds"] + st["tiles_direct"] == (n + TILE - 1) // TILE and st["batches"] == 1


def tile_case(ref0_len, exons=6, behind=3):
    """The novel list: TILE - 1 whole reads and one piece in the first tile, none of them on reference 0 -- so reference 0's name stands
    once in the tile, on the piece's transcript line, and its length moves the tile's bytes one by one -- and ``behind`` reads behind."""
    n = TILE + behind
    case = rc.make_case(41, [exons] * n, info=rc.NOVEL_PASS, flags=0, refs=(b"c" * ref0_len, b"chr2"), name_len=(6, 6), gene_len=(3, 3))
    case["tid"][:] = 1
    case["info"][5] = (case["info"][5] & ~np.uint32(0xf7)) | np.uint32(rc.NOVEL_FAIL)
    off = int(case["ex_off"][5])
    case["f"][off:off + exons] = [rc.NJ] + [0] * (exons - 1)
    sel = rr.select(case, rr.NOVEL)
    assert len(sel) == n and [b[3] for b in sel] == [0 if i == 5 else -1 for i in range(n)]
    return case


def tile_text_case(target):
    base = sum(len(t) for t in rr.texts(tile_case(1), rr.NOVEL)[:TILE])
    assert 0 <= target - base < 60000, (base, target)
    case = tile_case(1 + target - base)
    assert sum(len(t) for t in rr.texts(case, rr.NOVEL)[:TILE]) == target
    return case


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_text_at_the_lds_edge(eng, delta):
    st = check(eng, tile_text_case(LDS + delta), [rr.NOVEL])[rr.NOVEL]
    assert (st["tiles_lds"], st["tiles_direct"]) == ((2, 0) if delta <= 0 else (1, 1))


def test_tile_offsets_take_every_residue(eng):
    """The stream-out of k_rl_write (text_stream_out) with the second tile's span beginning at every offset modulo 16."""
    seen = set()
    for r in range(16):
        case = tile_case(40 + r, exons=3, behind=TILE + 1)
        seen.add(sum(len(t) for t in rr.texts(case, rr.NOVEL)[:TILE]) % 16)
        st = check(eng, case, [rr.NOVEL])[rr.NOVEL]
        assert (st["tiles_lds"], st["tiles_direct"], st["batches"]) == (3, 0, 1)
    assert seen == set(range(16))


def test_oversized_tiles_take_the_direct_path(eng, monkeypatch):
    case = rc.make_case(43, [2000] * 3 + [1] * (TILE - 3) + [2] * 5, info=(rc.NOVEL_FAIL, rc.NOVEL_PASS), flags="pieces", name_len=(60, 80))
    for form in (0, 1):
        monkeypatch.setenv("L2R_GTX_WAVE", str(form))
        st = check(eng, case, [rr.ALL])[rr.ALL]
        assert (st["tiles_lds"], st["tiles_direct"]) == (1, 1)
        check(eng, case, [rr.NOVEL], given=True)


@pytest.mark.parametrize("refs", [(b"R" * 200, b"c"), (b"c", b"R" * 200)])
def test_tiles_made_of_pieces_only(eng, refs):
    """The transcript line of a piece longer than its exon lines (a long reference 0), and shorter."""
    case = rc.flag_case(44, [[rc.NJ, 0, rc.UJ, rc.NJ, 0, 0]] * (2 * TILE + 5), refs=refs)
    case["tid"][:] = 1
    texts = rr.texts(case, rr.NOVEL)
    assert len(texts) == 2 * (2 * TILE + 5)
    lines = texts[0].split(b"\n")
    assert (len(lines[0]) > len(lines[1])) == (len(refs[0]) > len(refs[1]))
    check(eng, case, [rr.NOVEL])


# ---------------------------------------------------------------------------------------------------- batches, routes, errors

def test_batch_invariance(eng, mixed):
    small = head(mixed, 40)
    for lst in (rr.ALL, rr.NOVEL):
        m = len(rr.select(mixed, lst))
        assert check(eng, small, [lst], max_blocks=1)[lst]["batches"] == len(rr.select(small, lst))
        assert check(eng, mixed, [lst], max_blocks=3)[lst]["batches"] == (m + 2) // 3
        assert check(eng, mixed, [lst], max_blocks=TILE + 1)[lst]["batches"] == (m + TILE) // (TILE + 1)
        assert check(eng, small, [lst], max_bytes=1)[lst]["batches"] == len(rr.select(small, lst))      # down to one block each
        assert check(eng, mixed, [lst], max_bytes=3000)[lst]["batches"] > m // 20


def test_lines_takes_what_the_cut_says(eng, mixed):
    case = head(mixed, 50)
    want = rr.texts(case, rr.ALL)
    lens = [len(t) for t in want]
    rc.engine_reads(eng, case)
    assert eng.gtftext_list(rr.ALL)[0] == 50
    for first, mb, mby in ((0, 7, 1 << 30), (10, 1 << 20, sum(lens[10:13])), (10, 1 << 20, sum(lens[10:13]) - 1), (10, 1 << 20, sum(lens[10:13]) + 1), (49, 5, 1)):
        k, text = eng.gtftext_lines(first, mb, mby)
        assert k == rr.cut(lens, first, mb, mby) and text == b"".join(want[first:first + k])
        st = eng.gtftext_stats()
        assert st["lines"] == text.count(b"\n") and st["bytes"] == len(text) and st["route"] == 0 and st["guard_intact"] == 1
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(50)
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(0, 0)


def test_out_needs_room(eng, mixed):
    case = head(mixed, 9)
    want = rr.text(case, rr.ALL)
    rc.engine_reads(eng, case)
    eng.gtftext_list(rr.ALL)
    with pytest.raises(capi.L2RError):
        eng.gtftext_lines(0, cap=len(want) - 1)
    buf = np.full(len(want) + 8, 0x55, np.uint8)
    assert eng.lib.l2r_gtftext_out(eng.ctx, buf.ctypes.data, len(want) - 1) != 0 and (buf == 0x55).all()     # too little room: nothing is written
    eng._chk(eng.lib.l2r_gtftext_out(eng.ctx, buf.ctypes.data, len(want)))
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0x55).all()


def expect_error(e, case, lst, block, kind):
    rc.engine_reads(e, case)
    with pytest.raises(capi.L2RError) as err:
        e.gtftext_list(lst)
    assert "rc=-1:" in str(err.value) and "block %d:" % block in str(err.value) and rr.KIND_TEXT[kind] in str(err.value), (kind, block, str(err.value))
    for call in (lambda: e.gtftext_lines(0), lambda: e.gtftext_list_out(1)):        # nothing was written and nothing can be fetched
        with pytest.raises(capi.L2RError) as err:
            call()
        assert "rc=-1:" not in str(err.value)
    for other in rc.sound_lists(case, lst, block):                                   # ... and the lists without the bad read are sound
        check(e, case, [other], given=True)


def test_every_domain_error(eng, monkeypatch):
    for wave in (0, 1):
        monkeypatch.setenv("L2R_GTX_WAVE", str(wave))
        for case, lst, block, kind in rc.error_cases():
            expect_error(eng, case, lst, block, kind)


def test_order_of_calls(mixed):
    case = head(mixed, 3)
    e = capi.Engine(0)
    anno = lambda: e.gtftext_anno(case["anno"], case["tx_gid"], case["tx_gname"])
    reads = lambda: e.gtftext_reads(case["tid"], case["names"], case["qname"], None, rc.result_of(case), True, True)
    calls = [anno, reads, lambda: e.gtftext_list(rr.ALL), lambda: e.gtftext_list_out(3), lambda: e.gtftext_lines(0)]
    for call in calls:
        with pytest.raises(capi.L2RError) as err:
            call()
        assert "rc=-1:" not in str(err.value)
    e.gtftext_begin(case["refs"], case["src"], capi.GTX_PLAIN)
    with pytest.raises(capi.L2RError) as err:                # the lists are blocks of form READ
        anno()
    assert "form READ" in str(err.value)
    e.gtftext_begin(case["refs"], case["src"], capi.GTX_READ)
    for call in calls[1:]:
        with pytest.raises(capi.L2RError):
            call()
    anno()
    for call in calls[2:]:
        with pytest.raises(capi.L2RError):
            call()
    reads()
    with pytest.raises(capi.L2RError):
        calls[4]()
    with pytest.raises(capi.L2RError):                       # no list 4
        e.gtftext_list(4)
    assert e.gtftext_list(rr.ALL)[0] == 3 and e.gtftext_lines(0)[0] == 3
    with pytest.raises(capi.L2RError):                       # l2r_gtftext_blocks wants l2r_gtftext_rows
        e.gtftext_blocks(m=1)
    with pytest.raises(capi.L2RError):                       # results that do not fit the reads: an argument error ...
        e.gtftext_reads(case["tid"][:2], case["names"], case["qname"][:2], None, rc.result_of(case), n=2)
    with pytest.raises(capi.L2RError):                       # ... which leaves no reads behind
        calls[2]()
    e.close()


def test_route_host_gives_the_same_bytes_and_errors(eng, monkeypatch, mixed):
    monkeypatch.setenv("L2R_GTX_ROUTE", "host")
    check(eng, mixed, route=1)
    check(eng, head(mixed, 40), [rr.ALL, rr.NOVEL], max_blocks=3, route=1)
    for case in rc.piece_cases()[:3] + rc.name_cases()[-3:]:
        check(eng, case, route=1)
    for case, lst, block, kind in rc.error_cases():
        rc.engine_reads(eng, case)
        with pytest.raises(capi.L2RError) as e:
            eng.gtftext_list(lst)
        assert "rc=-1:" in str(e.value) and "block %d:" % block in str(e.value) and rr.KIND_TEXT[kind] in str(e.value)


def test_the_plain_blocks_still_work_behind_a_list(eng, mixed):
    """l2r_gtftext_rows / _blocks behind the lists: l2r_gtftext_lines goes back to k_gtx_write."""
    from tests import gtf_text_cases as gc
    from tests import gtf_text_restatement as gr
    check(eng, head(mixed, 20), [rr.NOVEL])
    case = gc.make_case(3, [1, 4, 2, 9, 1, 3], gr.READ)
    text, _, _, st = gc.engine_text(eng, case)
    assert text == gr.text(case) and st["route"] == 0 and st["piece_blocks"] == 0


# ---------------------------------------------------------------------------------------------------- the results of a run

SEED = 61           # chosen on the CPU with the oracle: its results alone meet the preconditions asserted below


@pytest.fixture(scope="module")
def run_set(oracle):
    anno = synth.make_annotation(3000, SEED, nchr=3)
    af, reads = anno.in_file_order(), synth.make_reads(anno, 700, 6, SEED)
    base = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=3))
    _, sj = util.junction_table(af, reads, base, SEED, cover=0.6)
    op = oracle.default_params(full_level=3, split_trans=1, min_sj_cnt=1)
    return af, reads, sj, op, util.oracle_run(oracle, af, reads, op, sj)


def run_reads(e, af, reads, sj, prm, want=capi.WANT_RESULTS):
    e.set_params(prm)
    e.set_outputs(want)
    e.set_annotation(af.tx_tid, af.tx_start, af.tx_end, af.tx_rev, af.tx_ex_off, af.ex_start, af.ex_end)
    e.set_junctions(sj)
    e.upload_reads(reads.tid, reads.pos, reads.rev, reads.cig_off, reads.cig)
    e.run()
    e.sync()


def run_case(af, reads, res):
    n, x = reads.n, int(res.ex_off[-1])
    names, qname = rr.pack_table([reads.qname(i).encode() for i in range(n)])
    anno, ids = rr.pack_table([af.gene_id(int(g)).encode() for g in af.tx_gene] + [af.gene_name(int(g)).encode() for g in af.tx_gene])
    info = np.asarray(res.info[:n], np.uint32)
    if not (info >> 8).any():                                # (the oracle's info carries no exon count)
        info = (info & np.uint32(0x7f)) | (np.diff(res.ex_off).astype(np.uint32) << 8)
    return {"refs": [c.encode() for c in reads.chrom_names], "src": b"lr2rmats", "tid": reads.tid, "names": names, "qname": np.asarray(qname, np.uint32), "tid_name": None,
            "anno": anno, "tx_gid": np.asarray(ids[:af.n_tx], np.uint32), "tx_gname": np.asarray(ids[af.n_tx:], np.uint32), "ex_off": res.ex_off, "xs": res.ex_start[:x],
            "xe": res.ex_end[:x], "f": res.ex_flag[:x], "info": info, "ref_tx": res.ref_tx[:n], "has_sj": True, "split": True}


def test_the_results_of_a_run_where_they_lie(eng, monkeypatch, run_set):
    af, reads, sj, op, oracle_res = run_set
    ref = run_case(af, reads, oracle_res)                     # the reference alone meets the preconditions
    sel = {lst: rr.select(ref, lst) for lst in rr.LISTS}
    pieces = [b for b in sel[rr.NOVEL] if b[3] >= 0]
    assert all(len(s) > 0 for s in sel.values()) and pieces and any(int(ref["info"][b[0]]) & rc.REV for b in pieces) and (ref["ref_tx"] < 0).any()
    run_reads(eng, af, reads, sj, util.to_engine_params(capi, op))
    case = run_case(af, reads, eng.download())
    want = {lst: rr.text(case, lst) for lst in rr.LISTS}
    assert want == {lst: rr.text(ref, lst) for lst in rr.LISTS}
    for wave in (None, 0, 1):
        if wave is not None:
            monkeypatch.setenv("L2R_GTX_WAVE", str(wave))
        eng.gtftext_begin(case["refs"], case["src"], capi.GTX_READ)
        eng.gtftext_anno(case["anno"], case["tx_gid"], case["tx_gname"])
        eng.gtftext_reads(reads.tid, case["names"], case["qname"], None, None, True, True)
        for st in check(eng, case, given=True, max_blocks=TILE + 1).values():
            assert wave is None or st["wave_form"] == wave
    monkeypatch.delenv("L2R_GTX_WAVE")
    check(eng, case)                                          # the same reads uploaded from l2r_download's arrays
    monkeypatch.setenv("L2R_GTX_ROUTE", "host")               # the host route fetches the results itself
    eng.gtftext_reads(reads.tid, case["names"], case["qname"], None, None, True, True)
    check(eng, case, given=True, route=1)
    monkeypatch.delenv("L2R_GTX_ROUTE")
    n = reads.n
    for bad_n in (n - 1, n + 1):                              # n differing from the run's reads
        with pytest.raises(capi.L2RError) as e:
            eng.gtftext_reads(reads.tid[:bad_n] if bad_n < n else np.append(reads.tid, 0), case["names"], case["qname"][:bad_n] if bad_n < n else np.append(case["qname"], 0))
        assert "the last run had %d reads" % n in str(e.value) and "rc=-1:" not in str(e.value)


def test_results_need_a_run_that_kept_them(run_set, mixed):
    af, reads, sj, op, _ = run_set
    case = head(mixed, 3)
    e = capi.Engine(0)
    e.gtftext_begin(case["refs"], case["src"], capi.GTX_READ)
    e.gtftext_anno(case["anno"], case["tx_gid"], case["tx_gname"])
    with pytest.raises(capi.L2RError) as err:                 # no run at all
        e.gtftext_reads(case["tid"], case["names"], case["qname"])
    assert "no completed run" in str(err.value) and "rc=-1:" not in str(err.value)
    run_reads(e, af, reads, sj, util.to_engine_params(capi, op), want=capi.WANT_ACCEPTED)
    names, qname = rr.pack_table([reads.qname(i).encode() for i in range(reads.n)])
    with pytest.raises(capi.L2RError) as err:
        e.gtftext_reads(reads.tid, names, np.asarray(qname, np.uint32))
    assert "kept no results" in str(err.value) and "rc=-1:" not in str(err.value)
    e.close()


# ---------------------------------------------------------------------------------------------------- the command

import filecmp
import re

from lr2rmats_amd import hostlib

HAND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_lists")
CONFIGS = {"default": {}, "host": {"L2R_GTX_ROUTE": "host"}, "off": {"L2R_GTX_ROUTE": "off"}, "small": {"L2R_GTX_BATCH": 3, "L2R_GTX_TEXT_MAX": 400},
           "shards": {"L2R_CHUNK_READS": None}, "threaded": {"L2R_THREADS": 3, "L2R_TAIL_PART_READS": 50}}
ROUTE = {"default": "route device", "host": "route host", "off": "route off", "small": "route device", "shards": "route device", "threaded": "route device"}
OUTS = ("gtf", "detail", "summary", "bed", "known", "novel", "unrec", "all")
LINE = re.compile(r"\[update_gtf\] read lists: route (device|host|off|mixed), all (\d+), known (\d+), novel (\d+) \((\d+) pieces\), unrecognised (\d+) blocks, (\d+) bytes, (\d+) batches$")


def every_way(tmp_path, make_args, n_reads, pieces=None):
    """One command in the six configurations: identical files and stdout; the timing line names the route and counts the blocks.
    make_args(outs) -> (argv, the files it writes).  Returns the default configuration's files."""
    got = {}
    for tag, env in CONFIGS.items():
        env = dict(env, L2R_TIMING=1)
        if tag == "shards":
            env["L2R_CHUNK_READS"] = max(1, n_reads // 3 - 1)                                  # at least three engine shards
        d = tmp_path / tag
        d.mkdir()
        argv, files = make_args({k: str(d / k) for k in OUTS})
        r = hostlib.run_cli(argv, env=env)
        assert r.returncode == 0, (tag, r.stderr.decode()[-1500:])
        lines = [ln for ln in r.stderr.decode().splitlines() if "read lists: route" in ln]
        assert len(lines) == 1 and ROUTE[tag] in lines[0] and LINE.match(lines[0]), (tag, lines)
        assert "detail text: route" not in lines[0] and "gtf text: route" not in lines[0]
        m = LINE.match(lines[0])
        if tag != "off":
            assert int(m.group(2)) == n_reads and (pieces is None or int(m.group(5)) == pieces), (tag, lines[0])
        if tag == "small" and n_reads > 3:
            assert int(m.group(8)) >= n_reads // 3
        got[tag] = (files, r.stdout)
    for tag in CONFIGS:
        assert got[tag][1] == got["default"][1], tag
        for a, b in zip(got[tag][0], got["default"][0]):
            assert filecmp.cmp(a, b, shallow=False), (tag, a)
    d = tmp_path / "plain"
    d.mkdir()
    argv, files = make_args({k: str(d / k) for k in OUTS})
    r = hostlib.run_cli(argv)                                                                  # without L2R_TIMING nothing new is on stderr
    assert r.returncode == 0 and r.stdout == got["default"][1] and b"read lists" not in r.stderr
    for a, b in zip(files, got["default"][0]):
        assert filecmp.cmp(a, b, shallow=False), a
    return got["default"][0]


@pytest.fixture(scope="module")
def cli_files(oracle, run_set, tmp_path_factory):
    af, reads, sj, op, want = run_set
    d = tmp_path_factory.mktemp("lists")
    anno = synth.make_annotation(3000, SEED, nchr=3)
    base = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=3))
    j, _ = util.junction_table(af, reads, base, SEED, cover=0.6)
    sam, bam, gtf, tab = str(d / "r.sam"), str(d / "r.bam"), str(d / "a.gtf"), str(d / "sj.tab")
    reads.write_sam(sam)
    synth.write_bam(reads, bam)
    anno.write_gtf(gtf)
    j.write(tab)
    case = run_case(af, reads, want)
    return {"sam": sam, "bam": bam, "gtf": gtf, "tab": tab, "n": reads.n, "case": case}


def all_outputs(o, extra, aln, gtf):
    return (["update-gtf"] + extra + ["-A", o["detail"], "-y", o["summary"], "-E", o["bed"], "-k", o["known"], "-v", o["novel"], "-u", o["unrec"], "-a", o["all"],
                                      "-o", o["gtf"], aln, gtf], [o[k] for k in OUTS])


@pytest.mark.parametrize("src", ["sam", "bam"])
def test_cli_synthetic_set(tmp_path, cli_files, src):
    case = cli_files["case"]
    pieces = sum(1 for b in rr.select(case, rr.NOVEL) if b[3] >= 0)
    assert pieces > 0
    files = every_way(tmp_path, lambda o: all_outputs(o, ["-s", "-l", "3", "-J", "1", "-j", cli_files["tab"]], cli_files[src], cli_files["gtf"]), cli_files["n"], pieces)
    for k, lst in (("all", rr.ALL), ("known", rr.KNOWN), ("novel", rr.NOVEL), ("unrec", rr.UNRECOG)):      # ... and they are the restatement over the oracle's results
        got, want = open(files[OUTS.index(k)], "rb").read(), rr.text(case, lst)
        assert got == want, (k, first_difference(got, want))


@pytest.mark.parametrize("name", ["upd", "split"])
def test_cli_hand_cases_equal_the_goldens(tmp_path, name):
    from tests.test_hand_known_answers import CASES
    cmd, inp, _, _ = CASES[name]
    n = sum(1 for ln in open(os.path.join(HAND, inp)) if not ln.startswith("@"))
    files = every_way(tmp_path, lambda o: all_outputs(o, list(cmd)[1:], os.path.join(HAND, inp), os.path.join(HAND, "anno.gtf")), n, 2 if name == "split" else 0)
    for k, g in (("all", "all"), ("known", "known"), ("novel", "novel"), ("unrec", "unrecog")):
        assert filecmp.cmp(files[OUTS.index(k)], os.path.join(GOLDEN, "%s.%s.gtf" % (name, g)), shallow=False), (name, k)


def test_cli_gtf_input_mode(tmp_path):
    """`-m g`: transcript_id and transcript_name differ (tid_name is given)."""
    from tests.test_hand_known_answers import CASES
    cmd, inp, anno, _ = CASES["mg"]
    n = sum(1 for _ in open(os.path.join(HAND, "mg.detail.txt"))) - 1          # (a read-like transcript may come without a transcript line)
    files = every_way(tmp_path, lambda o: all_outputs(o, list(cmd)[1:], os.path.join(HAND, inp), os.path.join(HAND, anno)), n)
    assert os.path.getsize(files[OUTS.index("all")]) > 0
