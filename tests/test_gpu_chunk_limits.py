"""GPU: k_tile_chunk's staging caps at their edges -- against the oracle, bit exact, on every kernel pipeline.

k_tile_chunk (l2r_tchunk.hip.h) stages a tile's dictionary slices and its window under fixed caps; tile_chunk_direct (l2r_slab.hip.h)
and the kernel itself decline what does not fit.  Each case below lands a locus exactly on one side of a cap and proves where it
landed: a model of the host dictionary builder (build_dict, l2r_engine.hip) says how many START / END entries a tile's slices hold,
and l2r_debug_counters says what the engine staged (words 24 / 25) and which tiles k_tile_chunk took (26) or declined (14).

    END slice       511 / 512 / 513 entries (TC_EN_CAP = 512: entry number en_nk is the "no entry" slot, 9 bits)
    START slice     126 / 127 / 128 / 129 entries (TC_ST_CAP = 128)
    parts of a key  1, 2 (tc_half's round of six reads), 3, 4 (its loop), 15 / 16 (TC_R_OVER: the read goes to the generic kernel)
    key-1 runs      0 .. 4 entries with the same key 1 in front of a read's missing pair, the run at the very start of the slice
    chunks          64 / 65 stretches with members (TC_CHUNKS)
    stretches       256 / 257 stretches up to the one that ends the sweeps (TC_TRIPS)

On the tile pipeline every case also runs with L2R_CHUNK_DIRECT=0: k_probe_slab_chunked then takes the same tiles.
"""
import bisect

import numpy as np
import pytest

from tests import util
from tests.test_gpu_edges import _anno, _chain, _reads, _run, pipeline  # noqa: F401  (pipeline: autouse fixture)
from tests.window_cases import _dictionaries, _parts  # noqa: F401  (the dictionary model, shared with the one-window cases)

pytestmark = pytest.mark.gpu

SITE_SHIFT = 9
TC_ST_CAP, TC_EN_CAP, TC_CHUNKS, TC_TRIPS, MEMBERS = 128, 512, 64, 256, 63      # (l2r_slab.hip.h, l2r_tchunk.hip.h)
LO_B, HI_B = 200, 262          # every read begins in bucket LO_B and ends in bucket HI_B: all tiles share one span, one slice


# ---- the model: build_dict (l2r_engine.hip) and the slice bounds of make_descriptor (l2r_window.hip.h)

def _model(txs, rows, tid=0):
    """(st_nk, en_nk, END entries of the slice) of the tiles of `rows`, which all share one span."""
    st, en, nb = _dictionaries(txs)
    starts = {(r[1] + 1) >> SITE_SHIFT for r in rows}
    ends = {(r[1] + sum(l for l, op in r[-1] if op in (0, 2, 3))) >> SITE_SHIFT for r in rows}
    assert starts == {LO_B} and ends == {HI_B}, (starts, ends)             # (the construction's promise: one span for every tile)
    lo, hi = min(LO_B, nb[tid] - 1), min(HI_B, nb[tid] - 1)

    def dir_(ent, b):                           # entries in front of bucket b of chromosome tid
        return bisect.bisect_left([(t, k1 >> SITE_SHIFT) for t, k1, _ in ent], (tid, b))
    # START from the reach-back directory: the first entry whose exon reaches into bucket lo from an earlier bucket
    rdir = dir_(st, lo)
    for i, (t, k1, k2) in enumerate(st):
        if t == tid and (k1 >> SITE_SHIFT) < lo <= min(k2 >> SITE_SHIFT, nb[tid] - 1) and (i == 0 or st[i - 1] != st[i]):
            rdir = min(rdir, i)
    e0, e1 = dir_(en, lo), dir_(en, hi + 1)
    return dir_(st, hi + 1) - rdir, e1 - e0, en[e0:e1]


# ---- the loci

def _first(b):
    return (LO_B * 512 + 60 + 5 * b, LO_B * 512 + 260 + 5 * b)


def _last(b):
    return (HI_B * 512 + 60 + 5 * b, HI_B * 512 + 260 + 5 * b)


def _inner(b, i, n_blocks):
    k = i * n_blocks + b
    return (103_000 + 120 * k, 103_050 + 120 * k)


def _gap(g):
    """A single-exon transcript over the whole locus: a window member that enters no dictionary."""
    return (0, g & 1, [(LO_B * 512 + 300 + g % 150, HI_B * 512 + 300 + g % 150)])


def _locus(pools, en_target=None, seed=0, extra=None):
    """Blocks of transcripts; block b is made of its own exons: first exon F_b (bucket LO_B), pools[b] inner exons, last exon L_b
    (bucket HI_B).  No site is shared between blocks, and a block holds fewer than 64 transcripts, so every key has one part.  Per block:
    core isoforms F_b + inner exons + L_b (the reads copy them; the first one is F_b, last inner exon, L_b: the block's largest
    junction), one transcript through all inner exons, and -- en_target -- chains of inner exons whose junctions nobody else has, until
    the END slice holds en_target entries.  Behind each block single-exon transcripts up to 64 in all (window members, no entries: a
    chunk of k_probe_slab_chunked meets at most two blocks' entries).  extra[b]: more transcripts of block b.
    Returns (transcripts in file order, the cores of each block)."""
    rng = np.random.default_rng(seed)
    nbk = len(pools)
    blocks, cores, used = [], [], []
    for b, P in enumerate(pools):
        inner = [_inner(b, i, nbk) for i in range(P)]
        cs = [[_first(b), inner[-1], _last(b)]]
        for _ in range(5):
            cs.append([_first(b)] + [inner[i] for i in sorted(rng.choice(P - 1, size=int(rng.integers(3, 6)), replace=False))] + [_last(b)])
        txs = [list(c) for c in cs] + [list(inner)] + [list(t) for t in (extra or {}).get(b, [])]
        blocks.append(txs)
        cores.append(cs)
        used.append({(t[k][1], t[k + 1][0]) for t in txs for k in range(len(t) - 1)})
    if en_target is not None:
        rest = en_target - sum(len(u) for u in used)
        assert rest >= 0, rest
        for b, P in enumerate(pools):
            inner = [_inner(b, i, nbk) for i in range(P)]
            r = rest // nbk + (1 if b < rest % nbk else 0)
            todo = [(i, i + d) for d in range(1, P) for i in range(P - d)]
            while r > 0:
                i, j = next(q for q in todo if (inner[q[0]][1], inner[q[1]][0]) not in used[b])
                chain = [i, j]
                used[b].add((inner[i][1], inner[j][0])); r -= 1
                while r > 0 and len(chain) < 6:
                    k = next((k for k in range(chain[-1] + 1, P) if (inner[chain[-1]][1], inner[k][0]) not in used[b]), None)
                    if k is None:
                        break
                    used[b].add((inner[chain[-1]][1], inner[k][0])); r -= 1
                    chain.append(k)
                blocks[b].append([inner[x] for x in chain])
    out, g = [], 0
    for b, txs in enumerate(blocks):
        assert len(txs) < 64, len(txs)
        out += [(0, (b + t) & 1, ex) for t, ex in enumerate(txs)]
        for _ in range(64 - len(txs)):
            out.append(_gap(g)); g += 1
    return out, cores


def _locus_rows(cores, n, seed):
    """Reads over the cores: whole isoforms with their outer ends moved inwards, all of whose sites are novel (donor entry 0 of the END
    slice -- F_0's end -- is the first core donor), with a novel donor inside, with a skipped exon."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cs = cores[i % len(cores)]
        ex = [list(x) for x in cs[int(rng.integers(len(cs)))]]
        ex[0][0] += int(rng.integers(0, 40))
        ex[-1][1] -= int(rng.integers(0, 40))
        kind = (i // len(cores)) % 4
        if kind == 1:
            ex[0][1] += 4
            for q in ex[1:-1]:
                q[0] += 4; q[1] += 4
            ex[-1][0] += 4
        elif kind == 2 and len(ex) > 3:
            ex[1][1] -= 5
        elif kind == 3 and len(ex) > 3:
            del ex[1]
        rows.append((0, *_chain([tuple(x) for x in ex])))
    return rows


def _check(oracle, txs, rows, pipeline, monkeypatch, levels=(1, 3, 5), route=None):
    """Runs the case at every level (on the tile pipeline with and without k_tile_chunk, against one oracle result per level),
    checks the model against the staged slices, calls route(words, direct) on the tile pipeline."""
    rows = sorted(((r[0], r[1], i & 1, r[2]) for i, r in enumerate(rows)), key=lambda r: (r[0], r[1]))
    st, en, _ = _model(txs, rows)
    af, reads = _anno(txs), _reads(rows)
    wants = []
    for level in levels:
        want = util.oracle_run(oracle, af, reads, oracle.default_params(full_level=level))
        for direct in ((1, 0) if pipeline == "tile" else (None,)):
            if direct is not None:
                monkeypatch.setenv("L2R_CHUNK_DIRECT", str(direct))
            w = []
            _run(oracle, af, reads, words=w, want=want, full_level=level)
            assert (w[24], w[25]) == (st, en), (w[24:27], st, en)
            if pipeline != "classic":
                assert w[23] == w[3] >= 1, w                       # every tile is one of the chunked kernels'
            if route is not None and pipeline == "tile":
                route(w, direct)
        wants.append(want)
    return st, en, wants


def _taken(w, direct):
    """k_tile_chunk took every tile (L2R_CHUNK_DIRECT=0: none)."""
    assert w[26] == (w[23] if direct else 0) and w[14] == 0, w


def _declined(w, direct):
    """tile_chunk_direct declined every tile: k_probe_slab_chunked took them."""
    assert w[26] == 0 and (1 <= w[14] <= w[23] if direct else w[14] == 0), w


def _taken_none_generic(w, direct):
    _taken(w, direct)
    assert w[0] == 0, w


# ---- the cases

@pytest.mark.parametrize("en", [511, 512, 513])
def test_end_slice_at_its_cap(oracle, en, pipeline, monkeypatch):
    """TC_EN_CAP: the END slot of "no entry" is entry number en_nk in a 9-bit field; at 512 it read as entry 0 with one part, whose
    donor mask (F_0's end, shared by block 0's cores in chunk 0) then stood in for every missing END key and every read's last exon:
    reads without a known site had one.  511 is taken, 512 and 513 go to k_probe_slab_chunked; nothing goes to the generic kernel."""
    txs, cores = _locus([18] * 5, en_target=en, seed=en)
    rows = _locus_rows(cores, 2500, en)

    def route(w, direct):
        (_taken if en < TC_EN_CAP else _declined)(w, direct)
        assert w[0] == 0, w
    st, got_en, wants = _check(oracle, txs, rows, pipeline, monkeypatch, route=route)
    assert got_en == en and st < TC_ST_CAP
    for want in wants:
        assert ((want.info & 3) == 0).sum() > 300                   # (reads without a known site: what the wrong donor mask flipped)


@pytest.mark.parametrize("st", [126, 127, 128, 129])
def test_start_slice_at_its_cap(oracle, st, pipeline, monkeypatch):
    """TC_ST_CAP: a tile with 127 START entries is k_tile_chunk's, one with 128 (its "no entry" slot would be the 129th) is not."""
    n = st - 8
    pools = [n // 4 + (1 if b < n % 4 else 0) for b in range(4)]
    txs, cores = _locus(pools, seed=st)
    rows = _locus_rows(cores, 2000, st)
    got_st, en, _ = _check(oracle, txs, rows, pipeline, monkeypatch, route=(lambda w, d: _taken(w, d) if st < TC_ST_CAP else _declined(w, d)))
    assert got_st == st and en < TC_EN_CAP


@pytest.mark.parametrize("parts", [1, 2, 3, 4, 15, 16])
def test_parts_of_one_key(oracle, parts, pipeline, monkeypatch):
    """A transcript P-A-X-W_m-Y-Z copied `parts` times, 64 transcripts apart in file order, each copy with an inner exon W_m of its own:
    the keys of A, X, Y, Z, A-X, Y-Z have that many parts (build_dict), and so have the junctions X-W_m (their donor is everybody's).
    P lies in front of the tiles' first bucket, so that a read beginning at A's first base meets an acceptor there (Q1,
    src/update_gtf.c:746): such a read over copy m is known through copy m alone, which only part m of the shared keys names.  A read that begins inside A, or
    has a novel donor on Y, is known nowhere; its strand comes from the last compatible copy.  tc_half takes one or two parts in its round of six
    reads and walks three or more in its loop; more than 15 parts do not fit the lookup word (TC_R_OVER): the reads with such a key,
    and only they, go to the generic kernel."""
    txs, cores = _locus([10, 10], seed=parts)
    pre = (LO_B * 512 - 300, LO_B * 512 - 200)
    head, tail = [(LO_B * 512 + 330, LO_B * 512 + 420), (110_000, 110_080)], [(112_000, 112_090), (HI_B * 512 + 330, HI_B * 512 + 420)]
    w = [(111_000 + 60 * m, 111_040 + 60 * m) for m in range(parts)]
    for m in range(parts):
        txs.append((0, m & 1, [pre] + head + [w[m]] + tail))
        if m + 1 < parts:
            txs += [_gap(1000 + 63 * m + g) for g in range(63)]
    rows = _locus_rows(cores, 1500, parts)
    rng = np.random.default_rng(parts)
    n_far = 600
    for i in range(n_far):
        ex = [list(x) for x in head + [w[(i // 3) % parts]] + tail]
        ex[-1][1] -= int(rng.integers(0, 60))
        if i % 3 == 1:
            ex[0][0] += int(rng.integers(1, 60))                     # (no acceptor at the read's first base)
        elif i % 3 == 2:
            ex[3][1] += 3                                             # (a novel donor on Y: the read is known nowhere)
        rows.append((0, *_chain([tuple(x) for x in ex])))

    def route(w, direct):
        assert w[0] == (n_far if direct and parts > 15 else 0), w     # (every read over the copies has X: over at 16 parts)
        _taken(w, direct)
    _, _, wants = _check(oracle, txs, rows, pipeline, monkeypatch, route=route)
    assert _dictionaries(txs)[0].count((0,) + head[1]) == parts
    copies = np.array([128 + 64 * m for m in range(parts)])
    for want in wants:                                                # (every copy decides some reads: known through each, compatible with the last)
        far = np.isin(want.ref_tx, copies)
        assert far.sum() == n_far and set(want.ref_tx[far & ((want.info & 1) != 0)].tolist()) == set(copies.tolist())
        assert (want.ref_tx[far & ((want.info & 1) == 0)] == copies[-1]).all()


@pytest.mark.parametrize("run", [0, 1, 2, 3, 4])
def test_entries_with_the_same_key_1_in_front_of_a_missing_pair(oracle, run, pipeline, monkeypatch):
    """A read's junction (X's end, Z's start) that the END dictionary does not have falls back to the first pair with key 1 = X's end
    (its donor mask says "known donor").  X is the first exon of the slice, so the `run` junctions from it -- to inner exons 2, 4, 6, 8
    of block 0 -- are the slice's first entries; the reads' Z begins before, between and behind them, or is one of them.  The slice's
    last entry (block 3's last inner exon to its last exon) is a pair the reads have too."""
    X = (LO_B * 512 + 10, LO_B * 512 + 40)
    nbk = 4
    ys = [2, 4, 6, 8][:run]
    extra = {0: [[X, _inner(0, y, nbk), _inner(0, 9, nbk), _last(0)] for y in ys]}
    txs, cores = _locus([10] * nbk, seed=40 + run, extra=extra)
    rows = _locus_rows(cores, 1500, run)
    for i in range(600):
        z = i % 9
        zs, ze = _inner(0, z, nbk)
        if z not in ys:
            zs += 2 + 4 * (i % 3)                                     # (a novel acceptor: the pair is missing, key 1 is not)
        rows.append((0, *_chain([X, (zs, ze), _inner(0, 9, nbk), _last(0)])))
    _, _, slc = _model(txs, sorted(rows, key=lambda r: (r[0], r[1])))
    assert [k for k in slc if k[1] == X[1]] == [(0, X[1], _inner(0, y, nbk)[0]) for y in ys] == slc[:run]
    assert slc[-1] == (0, _inner(nbk - 1, 9, nbk)[1], _last(nbk - 1)[0])
    _check(oracle, txs, rows, pipeline, monkeypatch, route=_taken_none_generic)


@pytest.mark.parametrize("chunks", [64, 65])
def test_chunks_with_members(oracle, chunks, pipeline, monkeypatch):
    """TC_CHUNKS: the window of 63 * 64 = 4032 members from the tile's cursor on is 64 chunks, one member more is 65: k_tile_chunk
    sends the locus' reads to the generic kernel (s_bad); k_probe_slab_chunked has no such cap."""
    txs, cores = _locus([10, 10], seed=chunks)
    n_members = MEMBERS * 64 + (chunks - 64)
    txs += [_gap(500 + g) for g in range(n_members - len(txs))]
    rows = _locus_rows(cores, 1200, chunks)

    def route(w, direct):
        assert w[0] == (len(rows) if direct and chunks > TC_CHUNKS else 0), w
        _taken(w, direct)
    _check(oracle, txs, rows, pipeline, monkeypatch, levels=(3,), route=route)


@pytest.mark.parametrize("trips", [256, 257])
def test_stretches_up_to_the_end_of_the_sweeps(oracle, trips, pipeline, monkeypatch):
    """TC_TRIPS: k_tile_chunk looks at 256 stretches of 63 transcripts from the tile's cursor on.  Transcripts that lie before every
    read fill them, one member lies in the last one and ends the annotation: stretch 256 is looked at, stretch 257 is not (no end of
    the sweeps in sight: the locus' reads go to the generic kernel)."""
    txs, cores = _locus([10, 10], seed=trips)
    n_tx = MEMBERS * (trips - 1) + 1
    txs += [(0, 0, [(1_000 + 2 * g, 1_001 + 2 * g)]) for g in range(n_tx - 1 - len(txs))] + [_gap(7)]
    rows = _locus_rows(cores, 1200, trips)

    def route(w, direct):
        assert w[0] == (len(rows) if direct and trips > TC_TRIPS else 0), w
        _taken(w, direct)
    _check(oracle, txs, rows, pipeline, monkeypatch, levels=(3,), route=route)
